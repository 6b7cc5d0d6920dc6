"""CPU tests (no GPU) of the diplotype table (genotyper --diplotypes, t1k_diplo_batch): the restatement tests/diplo_ref.py
against the definition read literally (sets of groups), the classes and the candidates the host forms, the order of the pairs with ties at
every level, the called pair at its true rank, the rounding of the printed weights, the designed inputs' own coverage, the command line,
and the C-ABI exports, their bindings and the kernel's resources."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import diplo_cases as cases
import diplo_ref as ref
import goldens
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags, kernel_metadata

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")


def blocks(p, mat):
    """the flat matrix as one {(i, j): M} per gene, i <= j, after checking that the cells i > j are 0"""
    out, base = [], 0
    for x in range(len(p.cand_ptr) - 1):
        n = p.cand_ptr[x + 1] - p.cand_ptr[x]
        assert all(mat[base + i * n + j] == 0 for i in range(n) for j in range(i))
        out.append({(i, j): mat[base + i * n + j] for i in range(n) for j in range(i, n)})
        base += n * n
    assert base == len(mat)
    return out


def check_against_brute(c, max_cand):
    p = ref.plan(*c.args(), max_cand)
    mat = ref.matrix(p.group_ptr, p.ent, p.q, p.cand_ptr)
    want = ref.brute(*c.args(), max_cand)
    assert len(want) == len(p.cand_ptr) - 1
    for x, ((cand, n_class, weight, M), got) in enumerate(zip(want, blocks(p, mat))):
        lo, hi = p.cand_ptr[x], p.cand_ptr[x + 1]
        assert [(p.rep[i], p.equiv[i], p.total[i]) for i in range(lo, hi)] == cand, x
        assert (p.n_class[x], p.weight[x]) == (n_class, weight) and got == M, x
        assert all(M[(i, i)] == cand[i][2] for i in range(len(cand)))      # the diagonal is T
    return p, mat


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_the_set_formulation_on_random_tables(seed):
    c = cases.host_random(seed, n_genes=1 + seed % 4, per=3 + seed % 7, n_groups=6 + 3 * seed)
    for max_cand in (2, 3, 512):
        check_against_brute(c, max_cand)


@pytest.mark.parametrize("max_cand", [2, 3, 4, 512])
def test_restatement_equals_the_set_formulation_on_the_designed_input(max_cand):
    check_against_brute(cases.host_designed(), max_cand)


def test_classes_of_the_designed_input():
    p, mat = check_against_brute(cases.host_designed(), 512)
    assert p.cand_ptr == [0, 6, 11, 15, 19, 19] and p.n_class == [6, 5, 4, 4, 0]
    # gene 0: the class of 40 is named by the called allele 17, not by its smallest index 5; allele 45 joins 0 and 1 because group 9 weighs nothing;
    # 2 and 4 weigh the same and stand in index order; 48 and 49 take no part
    assert list(zip(p.rep[0:6], p.equiv[0:6], p.total[0:6])) == [(17, 39, 1700), (0, 2, 1100), (2, 0, 600), (4, 0, 600), (3, 0, 100), (46, 1, 50)]
    assert p.called_cand[0:2] == [0, 4]
    # gene 1: both called alleles in one class, named by slot 0;  gene 2: slot 1 empty;  gene 3: no call, 66 and 67 tie;  gene 4: nothing
    assert [(p.rep[i], p.equiv[i], p.total[i]) for i in (6, 7)] == [(55, 0, 7070), (53, 1, 7000)] and p.called_cand[2:4] == [7, 7]
    assert p.called_cand[4:] == [p.rep.index(61), -1, -1, -1, -1, -1]
    assert [(p.rep[i], p.total[i]) for i in range(15, 19)] == [(68, 1280), (69, 940), (66, 640), (67, 640)]
    assert p.weight == [2050, 7070, 5410, 1580, 0]
    # a class is booked once per group: group 0 holds 43 alleles of gene 0 and two of gene 2, i.e. candidates 0 and 1 of gene 0 and two of gene 2
    assert p.ent[:p.group_ptr[1]] == [0, 1] + sorted(p.rep.index(a) for a in (60, 63)) and len(p.q) == 12 and 0 not in p.q


@pytest.mark.parametrize("max_cand,want", [(2, [17, 3]), (3, [17, 0, 3]), (4, [17, 0, 2, 3]), (5, [17, 0, 2, 4, 3])])
def test_called_classes_are_forced_among_the_candidates(max_cand, want):
    """slot 1 of gene 0 calls the class that ranks fifth by weight: it displaces the last candidate that is not called"""
    p = ref.plan(*cases.host_designed().args(), max_cand)
    assert p.rep[p.cand_ptr[0]:p.cand_ptr[1]] == want and p.n_class[0] == 6
    assert [p.rep[c] for c in p.called_cand[0:2]] == [17, 3]
    rows = [r for r in ref.lines(p, ref.matrix(p.group_ptr, p.ent, p.q, p.cand_ptr), 1) if r[0] == 0]
    assert all(r[12:] == (max_cand, 6) for r in rows) and [r for r in rows if r[11]][0][2:4] == (17, 3)


def test_both_called_classes_outside_displace_two():
    c = cases.host_designed()
    c.called[0:2] = [46, 3]                                       # the two lightest classes of gene 0
    p, _ = check_against_brute(c, 2)
    assert p.rep[0:2] == [3, 46] and [p.rep[i] for i in p.called_cand[0:2]] == [46, 3]
    p, _ = check_against_brute(c, 3)
    assert p.rep[0:3] == [5, 3, 46]                               # the big class is named by its smallest index now


# ---- the order, the called line --------------------------------------------------------------------------------------------------------
def hand_plan(called=(1, 3), scale=1):
    """one gene, four candidates with T = 100, 100, 80, 70 and W = 200 (times scale)"""
    p = ref.Plan()
    p.cand_ptr, p.rep, p.equiv, p.n_class, p.weight, p.called_cand = [0, 4], [10, 11, 12, 13], [0, 1, 0, 39], [9], [200 * scale], list(called)
    M = [[100, 50, 30, 20], [0, 100, 30, 70], [0, 0, 80, 0], [0, 0, 0, 70]]
    return p, [v * scale for row in M for v in row]


def test_order_with_ties_at_every_level():
    p, mat = hand_plan()
    rows = ref.lines(p, mat, 1000)
    # explained 150: (2,3) first, both contribute 70 and more; then four pairs whose smaller part is 50, by i, then by j; explained 100: two
    # homozygous pairs and (1,3), where 3 adds nothing to 1, all with a smaller part of 0, by i, then by j
    assert [(r[2] - 10, r[3] - 10) for r in rows] == [(2, 3), (0, 1), (0, 2), (0, 3), (1, 2), (0, 0), (1, 1), (1, 3), (2, 2), (3, 3)]
    assert [r[1] for r in rows] == list(range(1, 11))
    assert [r[4] for r in rows] == [150] * 5 + [100] * 3 + [80, 70] and [r[8] for r in rows] == [50] * 5 + [100] * 3 + [120, 130]
    assert [r[5:8] for r in rows[:5]] == [(80, 70, 0), (50, 50, 50), (70, 50, 30), (80, 50, 20), (70, 50, 30)]
    assert rows[7][5:8] == (30, 0, 70) and all(r[5:8] == (0, 0, r[4]) for r in rows if r[2] == r[3])
    assert [r[11] for r in rows] == [0] * 7 + [1, 0, 0] and all(r[12:] == (4, 9) for r in rows)
    assert rows[7][9:11] == (1, 39)


def test_called_pair_is_printed_at_its_true_rank():
    p, mat = hand_plan()
    assert [(r[1], r[11]) for r in ref.lines(p, mat, 3)] == [(1, 0), (2, 0), (3, 0), (8, 1)]
    assert [(r[1], r[11]) for r in ref.lines(p, mat, 8)] == [(k, int(k == 8)) for k in range(1, 9)]
    # slot 1 empty, or both slots in one class: the homozygous pair;  the slots in the other order: the same pair;  no call: no such line
    for called, rank in (((1, -1), 7), ((1, 1), 7), ((3, 1), 8), ((2, 3), 1)):
        p, mat = hand_plan(called)
        got = ref.lines(p, mat, 2)
        assert [(r[1], r[11]) for r in got] == ([(1, 1), (2, 0)] if rank == 1 else [(1, 0), (2, 0), (rank, 1)]), called
    p, mat = hand_plan((-1, -1))
    assert [(r[1], r[11]) for r in ref.lines(p, mat, 2)] == [(1, 0), (2, 0)]


def test_text_and_rounding():
    p, mat = hand_plan(scale=1 << 19)
    t = ref.text(p, mat, 2, ["G"], ["a%d" % i for i in range(14)])
    assert t == ref.HEADER + ("G\t1\ta12\ta13\t75.000\t40.000\t35.000\t0.000\t25.000\t0\t39\t0\t4\t9\n"
                              "G\t2\ta10\ta11\t75.000\t25.000\t25.000\t25.000\t25.000\t0\t1\t0\t4\t9\n"
                              "G\t8\ta11\ta13\t50.000\t15.000\t0.000\t35.000\t50.000\t1\t39\t1\t4\t9\n")
    assert len(ref.HEADER.split("\t")) == 14
    q = ref.Plan()                                             # 525 / 2^20 = 0.0005007 rounds up, 524 / 2^20 = 0.0004997 down
    q.cand_ptr, q.rep, q.equiv, q.n_class, q.weight, q.called_cand = [0, 0, 1], [0], [0], [0, 1], [0, 525 + 524], [-1, -1, 0, -1]
    assert ref.text(q, [525], 10, ["E", "G"], ["a"]) == ref.HEADER + "G\t1\ta\ta\t0.001\t0.000\t0.000\t0.001\t0.000\t0\t0\t1\t1\t1\n"


def test_a_gene_without_candidates_has_no_line():
    c = cases.host_designed()
    p = ref.plan(*c.args(), 512)
    rows = ref.lines(p, ref.matrix(p.group_ptr, p.ent, p.q, p.cand_ptr), 2)
    assert sorted(set(r[0] for r in rows)) == [0, 1, 2, 3]
    assert [r[1] for r in rows if r[0] == 3] == [1, 2] and not any(r[11] for r in rows if r[0] == 3)


# ---- the designed kernel inputs hold what they promise -----------------------------------------------------------------------------------
def test_designed_table_holds_the_cases():
    c = cases.designed()
    cp = c.cand_ptr.tolist()
    gene_of = lambda i: max(x for x in range(len(cases.COUNTS)) if cp[x] <= i)
    sizes = [len(g) for g in c.groups]
    assert set(cases.SIZES) <= set(sizes) and 70 in sizes and 71 in sizes
    g = dict(zip(c.tags, c.groups))
    assert [gene_of(i) for i in g["ends_at_63"]] == [4] * 64 + [5] * 30                     # a segment ends at lane 63, the next begins at lane 64
    assert [gene_of(i) for i in g["straddles"]] == [0] * 40 + [4] * 60 + [5] * 50           # 40 .. 99 and 100 .. 149 cross positions 64 and 128
    assert g["all_of_gene_0"] == c.ids(0) and g["single"] == c.ids(1) and len(g["two_tiles"]) == 128 and g["two_tiles_and_two"] == c.ids(5)
    held = set(i for grp in c.groups for i in grp)
    assert not held & set(c.ids(2)) and c.ids(3) == [] and set(c.ids(1)) <= held
    assert max(int(v) for v in c.q) > 1 << 40 and min(int(v) for v in c.q) == 1
    a = cases.adjacent_case()
    assert all(set(grp) & set(a.ids(0)) and set(grp) & set(a.ids(2)) for grp in a.groups)
    h = cases.hot_cell_case()
    assert len(h.groups) == 20000 and sum(int(v) for v in h.q) > 1 << 54


def test_matrix_restatement_on_a_table_by_hand():
    # gene 0: ids 0 1 2, gene 1: id 3;  groups {0, 2, 3} (q 5) and {1, 2} (q 7)
    gp, ent, q, cp = cases.refusals()["sound"][1]
    assert ref.matrix(gp, ent, q, cp) == [5, 0, 5, 0, 7, 7, 0, 0, 12] + [5]


# ---- the command line, the build -------------------------------------------------------------------------------------------------------
def test_usage_names_the_options(built):
    r = subprocess.run([GENO], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--diplotypes [INT]" in r.stderr and "prefix_diplotypes.tsv" in r.stderr and "--diploCandidates INT" in r.stderr


@pytest.mark.parametrize("option,value", [("--diplotypes", v) for v in ("0", "x", "1001", "-3", "5x")] + [("--diploCandidates", v) for v in ("1", "2049", "x", "-2", "7y")])
def test_bad_values_are_usage_errors_that_write_nothing(built, tmp_path, option, value):
    c = goldens.Case("cyp_rna_2x100", str(tmp_path / "in"))
    out = str(tmp_path / "o")
    arg = [option + "=" + value] if value.startswith("-") else [option, value]
    r = subprocess.run([GENO] + c.args() + ["-o", out, "--diplotypes"] + arg, stderr=subprocess.PIPE, text=True)
    limits = "--diplotypes takes an integer from 1 to 1000" if option == "--diplotypes" else "--diploCandidates takes an integer from 2 to 2048"
    assert r.returncode != 0 and limits in r.stderr and "./genotyper [OPTIONS]" in r.stderr
    assert glob.glob(out + "*") == []


def test_diplo_symbols_declared_exported_and_bound(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    assert re.search(r"^int t1k_diplo_batch\(t1k_ctx \*ctx, uint64_t nGroups, const uint64_t \*groupPtr", header, flags=re.M)
    for name in ("t1k_diplo_batch", "t1k_diplo_pieces", "t1k_job_diplotypes_text"):
        assert name in header and hasattr(L, name), name
    assert hasattr(t1k_amd.Context, "diplo_batch") and hasattr(t1k_amd.Job, "diplotypes_text") and callable(t1k_amd.diplo_pieces)
    assert [n for n, _ in t1k_amd.JobParams._fields_][-3:] == ["alternatives", "diplotypes", "diplo_candidates"]


def test_diplo_kernel_uses_no_scratch(tmp_path):
    """k_diplo_groups compiled for gfx950 with the Makefile's flags: no scratch memory, no spilled register, no LDS, and the sums are native
    64-bit atomic adds, not compare-and-swap loops"""
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_diplo.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_diplo.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    asm = open(out).read()
    kernels = kernel_metadata(asm)
    mine = [k for k in kernels if "k_diplo_groups" in k]
    assert len(mine) == 1, sorted(kernels)
    k = kernels[mine[0]]
    print("%s: %s VGPRs, %s SGPRs, %s bytes of scratch" % (mine[0], k[".vgpr_count"], k[".sgpr_count"], k[".private_segment_fixed_size"]))
    assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".group_segment_fixed_size"]) == 0, k
    assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0 and int(k[".vgpr_count"]) <= 64, k
    assert asm.count("global_atomic_add_x2") >= 2 and "cmpswap" not in asm and "v_readlane_b32" in asm


def test_job_parameters_binding_has_the_size_of_the_structure(built):
    """t1k_job_params_default clears sizeof(t1k_job_params) bytes: the binding's structure must be exactly as long; the new fields: 0 and 512"""
    n = C.sizeof(t1k_amd.JobParams)
    buf = (C.c_uint8 * (n + 64))(*([0xEE] * (n + 64)))
    f = t1k_amd.lib().t1k_job_params_default
    keep, f.argtypes = f.argtypes, [C.c_void_p]
    try:
        f(C.addressof(buf))
    finally:
        f.argtypes = keep
    p = t1k_amd.JobParams.from_buffer(buf)
    assert bytes(buf[n:]) == b"\xee" * 64 and p.diplotypes == 0 and p.diplo_candidates == 512 and p.alternatives == 0 and p.filter_frac == 0.15
    at = t1k_amd.JobParams.diplo_candidates.offset
    assert at == t1k_amd.JobParams.alternatives.offset + 8 and at + 4 <= n and bytes(buf[at:at + 4]) == (512).to_bytes(4, "little")


def test_piece_count_follows_the_rule(built, monkeypatch):
    gp = np.array([0, 3, 3, 10, 11, 12, 40], dtype=np.uint64)
    for piece, want in ((1, 6), (2, 5), (3, 4), (7, 4), (9, 3), (12, 2), (39, 2), (40, 1), (1000, 1)):
        monkeypatch.setenv("T1K_DIPLO_PIECE", str(piece))
        assert t1k_amd.diplo_pieces(gp) == want, piece
        monkeypatch.setenv("T1K_ALT_PIECE", str(piece))
        assert t1k_amd.diplo_pieces(gp) == t1k_amd.alt_pieces(gp) == want, piece     # the rule of t1k_alt_batch
        monkeypatch.delenv("T1K_ALT_PIECE")
    monkeypatch.delenv("T1K_DIPLO_PIECE")
    assert t1k_amd.diplo_pieces(gp) == 1 and t1k_amd.diplo_pieces(np.array([0], dtype=np.uint64)) == 0
