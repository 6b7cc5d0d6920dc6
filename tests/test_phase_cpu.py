"""CPU tests (no GPU) of the read-backed phasing of site pairs (analyzer --phase, t1k_phase_*): the command line, the C-ABI
export, the new kernels' resource figures from a cross-compile, and the sequential restatement (phase_ref) the GPU tests compare the
kernels and the analyzer against, with the cases its generated table has to cover."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import phase_ref as ref
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags, kernel_metadata

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ENTRY_POINTS = ("t1k_phase_begin", "t1k_phase_add", "t1k_phase_get", "t1k_phase_stats", "t1k_phase_end")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(*ref.table_args(table))


def test_vectorised_restatement_equals_the_loops():
    t = ref.generate(seed=3, records=200, bookings=300, clones=30)
    (a, sa), (b, sb) = ref.restate(*ref.table_args(t)), ref.restate_by_loops(*ref.table_args(t))
    assert len(a) > 1000 and ref.same(a, b) and vars(sa) == vars(sb) and sa.discordant > 10


def test_restatement_by_hand():
    """one allele ACGTACGTAC, sites at 1, 3, 4, 8; mate 1 reads positions 0 .. 4 (a deletion at 3), mate 2 positions 3 .. 9 with an insert
    behind position 3: (C, -, A) and (T, A, A).  Position 3 is discordant, position 4 agrees: the booking observes 1 = C, 4 = A, 8 = A"""
    off = np.array([0, 10], np.uint64)
    text = b"ACGA" + b"TXACGTAC"
    ops = np.array([0, 0, 0, 3, 0] + [0, 2, 0, 0, 0, 0, 0, 0], np.int8)
    aln = np.array([(0, 0, 0, 0, 5, 0, 0, 0), (0, 3, 4, 5, 8, 0, 0, 0)], t1k_amd.PILEUP_ALN_DTYPE)
    sa, sp = np.zeros(4, np.uint32), np.array([1, 3, 4, 8], np.uint32)
    ptr, site, state = ref.observations(off, aln, text, ops, sa, sp)
    assert ptr.tolist() == [0, 3, 6] and site.tolist() == [0, 1, 2, 1, 2, 3] and state.tolist() == [1, 5, 0, 3, 0, 0]
    for restate in (ref.restate, ref.restate_by_loops):
        cells, st = restate(off, aln, [[0, 1], [1, ref.NO_MATE], [0, 0]], [1, 0, 0], text, ops, sa, sp)
        assert {k: v.tolist() for k, v in cells.items()} == {
            (0, 2, 1, 0): [2, 1], (0, 3, 1, 0): [1, 1], (2, 3, 0, 0): [2, 1],                # booking 0 (uniq) and parts of the other two
            (1, 2, 3, 0): [1, 0], (1, 3, 3, 0): [1, 0],                                      # booking 1: mate 2 alone
            (0, 1, 1, 5): [1, 0], (1, 2, 5, 0): [1, 0]}                                      # booking 2: mate 1 with itself
        assert (st.observations, st.bookings, st.keys, st.discordant) == (6, 3, 9, 1)


def test_runs_round_trip(table, want):
    """the key layout of t1k_phase_get: a cell's uniq bookings under the even key, the others under the odd one"""
    n_sites = len(table.site_allele)
    keys, counts = [], []
    for (s, t, x, y), c in sorted(want[0].items()):
        for uniq, v in ((1, c[1]), (0, c[0] - c[1])):
            if v:
                keys.append(((((s * n_sites + t) * 36 + x * 6 + y) << 1) | (1 - uniq)))
                counts.append(v)
    assert keys == sorted(keys) and ref.same(ref.from_runs(keys, counts, n_sites), want[0])
    assert sum(counts) == want[1].keys


def test_table_covers_the_cases(table, want):
    cells, st = want
    assert 200000 <= st.keys <= 5000000                      # the keys the kernels emit: a few folds' worth, not a benchmark
    assert st.discordant > 1000
    assert any(k[2] == ref.DEL or k[3] == ref.DEL for k in cells) and any(k[2] == ref.N or k[3] == ref.N for k in cells)
    assert all(s < t and table.site_allele[s] == table.site_allele[t] for s, t, _, _ in cells)
    assert all(0 < c[0] and 0 <= c[1] <= c[0] for c in cells.values())
    assert any(c[1] == c[0] for c in cells.values()) and any(c[1] == 0 for c in cells.values()) and any(0 < c[1] < c[0] for c in cells.values())
    # an insert column at a site observes nothing: the per-barcode pileup books it there, the observations do not hold it
    hit = ref.sitepile_ref.hits(table.allele_off, table.aln, table.text, table.ops, table.site_allele, table.site_pos)
    ptr, site, state = ref.observations(table.allele_off, table.aln, table.text, table.ops, table.site_allele, table.site_pos)
    assert (hit.op == 2).sum() > 100 and len(site) == st.observations == (hit.op != 2).sum() and state.max() == 5
    assert all((np.diff(site[ptr[r]:ptr[r + 1]]) > 0).all() for r in range(0, len(table.aln), 37))     # ascending inside a record
    # bookings: without a mate, a record with itself, a record with its edited clone, two records of one allele; both uniq flags
    r1, r2 = table.book_rec[:, 0].astype(np.int64), table.book_rec[:, 1].astype(np.int64)
    assert (r2 == ref.NO_MATE).sum() > 1000 and (r2 == r1).sum() > 500 and sum(table.clone_of.get(int(b)) == int(a) for a, b in zip(r1, r2)) > 1000
    mate = r2 != ref.NO_MATE
    assert (table.aln["allele"][r1[mate]] == table.aln["allele"][r2[mate]]).all()
    assert 0.2 < table.book_uniq.mean() < 0.45
    # a booking's merged observations: 0, 1, 2, and beyond one 64-lane step (beyond two: the edge tests of test_gpu_phase)
    b, _, _, disc, _ = ref.merged(*ref.table_args(table))
    m = np.bincount(b, minlength=len(r1))
    assert all((m == v).sum() > 0 for v in (0, 1, 2)) and (m > 64).sum() > 0
    assert ((disc > 0) & (m == 0)).sum() > 0                 # every site both mates see is discordant
    h = np.diff(ptr)
    assert (h == 0).sum() > 100 and h.max() > 64
    assert st.bookings == (m >= 2).sum() and st.keys == (m * (m - 1) // 2).sum()


def test_table_text_round_trip(tmp_path):
    cells = {(0, 2, 1, 5): (3, 1), (0, 1, 0, 4): (2, 0), (3, 4, 2, 3): (7, 7), (0, 1, 0, 0): (1, 1)}
    text = ref.table_text(["X*01", "Y*02"], ["ACGT", "TNA"], [[1, 0, 1, 1], [0, 1, 1]], [0, 0, 0, 1, 1], [0, 2, 3, 1, 2], {(0, 2): "T", (1, 1): "A,C"}, cells)
    p = tmp_path / "t.tsv"
    p.write_text(text)
    header, rows = ref.parse(str(p))
    assert header == ref.HEADER
    assert rows == [("X*01", 1, 3, 1, 2, "A", "G", ".", "T", "A", "A", 1, 1), ("X*01", 1, 3, 1, 2, "A", "G", ".", "T", "A", "N", 2, 0),
                    ("X*01", 1, 4, 1, 3, "A", "T", ".", ".", "C", "-", 3, 1), ("Y*02", 2, 3, 1, 2, "N", "A", "A,C", ".", "G", "T", 7, 7)]


def test_analyzer_records():
    import pileup_ref
    ptr, asg, ops = pileup_ref.assignments([
        [(0, pileup_ref.overlap(0, 0, 3, 2, 5), [0, 0, 1, 0], pileup_ref.overlap(0, 0, 2, 7, 9), [0, 0, 0])],
        [(0, pileup_ref.overlap(0, 0, 3, 0, 3), [0] * 4), (1, pileup_ref.overlap(1, 0, 3, 1, 4), [0] * 4, pileup_ref.overlap(1, 0, 3, 9, 12), [0] * 4)]])
    aln, text, book_rec, book_uniq = ref.analyzer_records(ptr, asg, ["ACGT", "ACGT"], ["TTT", "GGGG"])
    assert len(aln) == 5 and book_rec.tolist() == [[0, 1], [2, ref.NO_MATE], [3, 4]] and book_uniq.tolist() == [1, 0, 0]


# ---- the build ---------------------------------------------------------------------------------------------------------------------------
def test_phase_symbols_declared_and_exported(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(t1k_ctx \*ctx" % name, header, flags=re.M), name
        assert hasattr(L, name), name
    assert all(hasattr(t1k_amd.Context, n) for n in ("phase", "phase_begin", "phase_add", "phase_get", "phase_stats", "phase_end"))


def test_phase_kernels_use_no_scratch(tmp_path):
    """the five kernels of t1k_phase.hip, compiled for gfx950 with the Makefile's flags: no scratch memory and no spilled register"""
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_phase.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_phase.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    kernels = kernel_metadata(open(out).read())
    for pattern in (r"_Z11k_phase_obsILb0EE", r"_Z11k_phase_obsILb1EE", r"_Z12k_phase_need", r"_Z13k_phase_merge", r"_Z13k_phase_pairs"):
        mine = [k for k in kernels if re.match(pattern, k)]
        assert len(mine) == 1, (pattern, sorted(kernels))
        k = kernels[mine[0]]
        print("%s: %s VGPRs, %s SGPRs, %s + %s spilled, %s bytes of scratch" % (mine[0], k[".vgpr_count"], k[".sgpr_count"], k[".vgpr_spill_count"], k[".sgpr_spill_count"],
                                                                                k[".private_segment_fixed_size"]))
        assert int(k[".private_segment_fixed_size"]) == 0, (mine[0], k)
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, (mine[0], k)


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_analyzer_usage_lists_the_flag(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--phase:" in r.stderr and "prefix_allele_phase.tsv" in r.stderr and "--sites FILE: more sites for --barcodePileup and --phase" in r.stderr


def _no_allele(tmp_path, extra):
    empty = tmp_path / "none_allele.tsv"
    empty.write_text("")
    o = str(tmp_path / "o")
    r = subprocess.run([ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(empty), "-u", str(tmp_path / "r.fq"), "-o", o] + extra, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return o, r.stderr


def test_no_allele_selected_gives_the_header_alone(built, tmp_path):
    o, _ = _no_allele(tmp_path, ["--phase"])                 # (no --barcode needed)
    assert open(o + "_allele_phase.tsv").read() == ref.HEADER + "\n"


def test_sites_warning_only_without_both_flags(built, tmp_path):
    sites = str(tmp_path / "sites.tsv")
    open(sites, "w").write("")
    _, err = _no_allele(tmp_path, ["--sites", sites])
    assert "--sites has no meaning without" in err and "ignored" in err
    o, err = _no_allele(tmp_path, ["--sites", sites, "--phase"])
    assert "--sites has no meaning" not in err and os.path.exists(o + "_allele_phase.tsv")
    _, err = _no_allele(tmp_path, ["--sites", sites, "--barcodePileup", "--barcode", str(tmp_path / "bc.fa")])
    assert "--sites has no meaning" not in err
