"""CPU tests (no GPU) of the alternatives table (genotyper --alternatives, t1k_alt_batch): the restatement tests/alt_ref.py
against the definition read literally (sets of groups), the ranking rule with ties at every level, the `identical` count, the `.` line,
the rounding of the printed weights, the designed input's own coverage, the command line, and the C-ABI export and its binding."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import alt_cases as cases
import alt_ref as ref
import goldens
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags, kernel_metadata

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
EMPTY = ref.EMPTY


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_the_set_formulation_on_random_tables(seed):
    c = cases.random_case(seed, n_genes=1 + seed % 5, per=2 + seed % 7, n_groups=10 + 7 * seed, max_size=1 + seed)
    assert ref.tables(*c.args()) == ref.brute(*c.args())


def test_restatement_equals_the_set_formulation_on_the_designed_table():
    c = cases.designed()
    assert ref.tables(*c.args()) == ref.brute(*c.args())
    for n in (31, 32, 33, 150):
        w = cases.word_edge_case(n)
        assert ref.tables(*w.args()) == ref.brute(*w.args())


def test_designed_table_holds_the_cases():
    c = cases.designed()
    sizes = [len(g) for g in c.groups]
    assert set(sizes) == set(cases.SIZES) and min(sizes.count(n) for n in cases.SIZES) >= 8
    called = {int(s): a for a, s in enumerate(c.slot_of) if int(s) != EMPTY}
    assert sorted(called) == [0, 1, 2, 4, 5, 8, 9]                       # gene 1: slot 1 empty; gene 3: no call
    seen = set()
    for g in c.groups:
        pat = {}
        for a in g:
            if int(c.slot_of[a]) != EMPTY:
                pat.setdefault(int(c.slot_of[a]) >> 1, set()).add(int(c.slot_of[a]) & 1)
        seen.add(tuple(sorted((gene, tuple(sorted(k))) for gene, k in pat.items())))
        genes = set(int(c.allele_gene[a]) for a in g)
        if len(g) >= 63:
            assert len(genes) == 5                                          # a long group runs through every gene
    assert () in seen and ((0, (0,)),) in seen and ((0, (1,)),) in seen and ((0, (0, 1)),) in seen
    assert ((0, (0,)), (2, (1,))) in seen and ((0, (0, 1)), (1, (0,)), (2, (0,))) in seen   # two and three genes, patterns differ
    g65 = [g for g, t in zip(c.groups, c.tags) if t[0] == 65]
    assert any(g[0] == 0 and int(c.slot_of[0]) == 0 for g in g65) and any(g[-1] == 399 and int(c.slot_of[399]) == 9 for g in g65)
    t = ref.tables(*c.args())
    assert max(t[0]) > 1 << 40 and all(t[0][a] == t[1][a] + t[2][a] + t[3][a] - sum(  # inclusion-exclusion over the two slots
        int(c.q[i]) for i, g in enumerate(c.groups) if a in g and called.get(2 * (a % 5)) in g and called.get(2 * (a % 5) + 1) in g) for a in range(400))


def test_word_edge_cases_call_the_last_slots():
    for n, top in ((31, 61), (32, 63), (33, 65), (150, 299)):
        w = cases.word_edge_case(n)
        slots = sorted(int(s) for s in w.slot_of if int(s) != EMPTY)
        assert slots == [0, 1, top - 3, top - 2, top - 1, top] and 2 * w.n_genes == top + 1
        assert any(len(g) > 64 for g in w.groups)


# ---- ranking, identical, the `.` line ------------------------------------------------------------------------------------------------
def hand_tables():
    # gene 0: allele 0 called in slot 0 (total 100), allele 9 in slot 1 (total 7); gene 1: allele 10 called, nothing beside it
    A = 12
    gene = [0] * 10 + [1, 1]
    slot = [EMPTY] * A
    slot[0], slot[9], slot[10] = 0, 1, 2
    total = [100, 90, 95, 90, 100, 60, 0, 130, 100, 7, 50, 0]
    both0 = [100, 80, 80, 80, 100, 60, 0, 100, 100, 0, 0, 0]
    both1 = [0, 0, 0, 0, 0, 0, 0, 7, 0, 7, 0, 0]
    neither = [0, 10, 15, 10, 0, 0, 0, 23, 0, 0, 0, 0]
    return [total, both0, both1, neither], gene, slot


def test_ranking_rule_with_ties_at_every_level():
    tabs, gene, slot = hand_tables()
    rows = [r for r in ref.lines(tabs, gene, slot, top=1000) if r[1] == 0]
    # lost ascending (7: 0), then gained descending (2 before 1 and 3: 15 > 10), then the allele index (1 before 3), then lost 40 (5), 100 (9)
    assert [r[4] for r in rows] == [7, 2, 1, 3, 5, 9]
    assert [r[3] for r in rows] == [1, 2, 3, 4, 5, 6]
    assert [(r[8], r[9]) for r in rows] == [(0, 30), (20, 15), (20, 10), (20, 10), (40, 0), (100, 7)]
    assert [r[10] for r in rows] == [23, 15, 10, 10, 0, 0] and all(r[5] == 100 for r in rows)
    assert [r[4] for r in ref.lines(tabs, gene, slot, top=3) if r[1] == 0] == [7, 2, 1]


def test_identical_alleles_are_counted_not_listed_and_empty_ones_skipped():
    tabs, gene, slot = hand_tables()
    rows = ref.lines(tabs, gene, slot, top=1000)
    first = [r for r in rows if r[1] == 0]
    assert all(r[11] == 2 for r in first) and not any(r[4] in (4, 8, 6) for r in first)   # 4 and 8 hold exactly the groups of 0; 6 holds none
    # the other called allele of the gene is an ordinary candidate, on both sides
    assert 9 in [r[4] for r in first]
    second = [r for r in rows if r[1] == 9]
    assert [r[2] for r in second] == [1] * len(second) and second[0][4] == 7 and second[0][8:10] == (0, 123) and 0 in [r[4] for r in second]


def test_a_called_allele_without_alternatives_gets_the_dot_line():
    tabs, gene, slot = hand_tables()
    rows = [r for r in ref.lines(tabs, gene, slot, top=5) if r[1] == 10]
    assert rows == [(1, 10, 0, 0, None, 50, 0, 0, 0, 0, 0, 0)]
    names = ["a%d" % i for i in range(12)]
    t = ref.text(tabs, gene, slot, 5, ["G0", "G1"], names, [0.25] * 12)
    assert t.startswith(ref.HEADER) and t.endswith("G1\ta10\t0\t0\t.\t0.000\t0.000\t0.000\t0.000\t0.000\t0.000\t0.000000\t0\n")
    assert t.splitlines()[1] == "G0\ta0\t0\t1\ta7\t0.000\t0.000\t0.000\t0.000\t0.000\t0.000\t0.250000\t2"
    assert len(t.splitlines()) == 1 + 5 + 5 + 1 and all(len(l.split("\t")) == 13 for l in t.splitlines())


def test_file_order_is_gene_then_slot():
    c = cases.designed()
    rows = ref.lines(ref.tables(*c.args()), c.allele_gene, c.slot_of, top=2)
    keys = [(r[0], r[2]) for r in rows]
    assert keys == sorted(keys) and sorted(set(keys)) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (4, 0), (4, 1)]


# ---- numbers -------------------------------------------------------------------------------------------------------------------------
def test_printed_weights_round_as_printf_does():
    assert ref.fmt(0) == "0.000" and ref.fmt(1 << 20) == "1.000" and ref.fmt(3 << 19) == "1.500"
    assert ref.fmt(524) == "0.000" and ref.fmt(525) == "0.001"             # 0.0004997 / 0.0005007: the first weight that rounds up
    assert ref.fmt((1 << 20) - 1) == "1.000" and ref.fmt((1 << 20) - 525) == "0.999"
    assert ref.fmt(65536) == "0.062" and ref.fmt(196608) == "0.188"        # exact ties (0.0625, 0.1875) go to the even digit
    assert ref.fmt((1 << 62) + (1 << 61)) == "6597069766656.000"


def test_fixed_point_weight_is_llrint():
    assert ref.q_of(1.0) == 1 << 20 and ref.q_of(0.5) == 1 << 19 and ref.q_of(0.0) == 0
    assert ref.q_of(np.float32(0.1)) == 104858 and ref.q_of(np.float32(0.01)) == 10486   # 104857.6016, 10485.76
    assert ref.q_of(2.0 ** -21) == 0 and ref.q_of(3 * 2.0 ** -21) == 2 and ref.q_of(5 * 2.0 ** -21) == 2   # halves go to the even integer
    assert ref.q_of(np.float32(1234567.1)) == int(np.float32(1234567.1)) << 20 | int((float(np.float32(1234567.1)) % 1) * (1 << 20))


# ---- the command line, the build -----------------------------------------------------------------------------------------------------
def test_usage_names_the_option(built):
    r = subprocess.run([GENO], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--alternatives [INT]" in r.stderr and "prefix_alternatives.tsv" in r.stderr


@pytest.mark.parametrize("value", ["0", "x", "1001", "-3", "5x"])
def test_bad_counts_are_usage_errors_that_write_nothing(built, tmp_path, value):
    c = goldens.Case("cyp_rna_2x100", str(tmp_path / "in"))
    out = str(tmp_path / "o")
    arg = ["--alternatives=" + value] if value.startswith("-") else ["--alternatives", value]
    r = subprocess.run([GENO] + c.args() + ["-o", out] + arg, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "--alternatives takes an integer from 1 to 1000" in r.stderr and "./genotyper [OPTIONS]" in r.stderr
    assert glob.glob(out + "*") == []


def test_alt_symbols_declared_exported_and_bound(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    assert re.search(r"^int t1k_alt_batch\(t1k_ctx \*ctx, uint64_t nGroups, const uint64_t \*groupPtr", header, flags=re.M)
    for name in ("t1k_alt_batch", "t1k_alt_pieces", "t1k_job_alternatives_text", "t1k_job_allele_table"):
        assert name in header and hasattr(L, name), name
    assert hasattr(t1k_amd.Context, "alt_batch") and hasattr(t1k_amd.Job, "alternatives_text") and hasattr(t1k_amd.Job, "allele_table")
    assert t1k_amd.ALT_EMPTY == EMPTY == cases.EMPTY


def test_alt_kernel_uses_no_scratch(tmp_path):
    """k_alt_groups compiled for gfx950 with the Makefile's flags: no scratch memory, no spilled register, no static LDS (the bitsets are
    dynamic: 16 bytes per 32 slots), and the sums are native 64-bit atomic adds, not compare-and-swap loops"""
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_alt.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_alt.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    asm = open(out).read()
    kernels = kernel_metadata(asm)
    mine = [k for k in kernels if "k_alt_groups" in k]
    assert len(mine) == 1, sorted(kernels)
    k = kernels[mine[0]]
    print("%s: %s VGPRs, %s SGPRs, %s bytes of scratch" % (mine[0], k[".vgpr_count"], k[".sgpr_count"], k[".private_segment_fixed_size"]))
    assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".group_segment_fixed_size"]) == 0, k
    assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0 and int(k[".vgpr_count"]) <= 64, k
    assert asm.count("global_atomic_add_x2") >= 4 and "cmpswap" not in asm


def test_job_parameters_binding_has_the_size_of_the_structure(built):
    """t1k_job_params_default clears sizeof(t1k_job_params) bytes: the binding's structure must be exactly as long, and the new field 0"""
    n = C.sizeof(t1k_amd.JobParams)
    buf = (C.c_uint8 * (n + 64))(*([0xEE] * (n + 64)))
    f = t1k_amd.lib().t1k_job_params_default
    keep, f.argtypes = f.argtypes, [C.c_void_p]
    try:
        f(C.addressof(buf))
    finally:
        f.argtypes = keep
    p = t1k_amd.JobParams.from_buffer(buf)
    assert bytes(buf[n:]) == b"\xee" * 64 and p.alternatives == 0 and p.batch_fragments == 0 and p.filter_frac == 0.15
    at = t1k_amd.JobParams.alternatives.offset
    assert at + 4 <= n and bytes(buf[at:at + 4]) == b"\0\0\0\0"


def test_piece_count_follows_the_rule(built, monkeypatch):
    gp = np.array([0, 3, 3, 10, 11, 12, 40], dtype=np.uint64)
    for piece, want in ((1, 6), (2, 5), (3, 4), (7, 4), (9, 3), (12, 2), (39, 2), (40, 1), (1000, 1)):
        monkeypatch.setenv("T1K_ALT_PIECE", str(piece))
        assert t1k_amd.alt_pieces(gp) == want, piece
    monkeypatch.delenv("T1K_ALT_PIECE")
    assert t1k_amd.alt_pieces(gp) == 1 and t1k_amd.alt_pieces(np.array([0], dtype=np.uint64)) == 0
