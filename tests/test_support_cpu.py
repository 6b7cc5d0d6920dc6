"""CPU tests (no GPU) of the support table at sites (analyzer --siteSupport, t1k_support_*): the command line, the C-ABI
export, and the sequential restatement (support_ref) the GPU tests compare the kernel and the analyzer against -- summed over strand, mate
and end distance it is the per-base pileup at the sites -- with the cases its generated table has to cover."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pileup_ref
import sitepile_ref
import support_ref as ref
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags, kernel_metadata

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ENTRY_POINTS = ("t1k_support_begin", "t1k_support_add", "t1k_support_get", "t1k_support_stats", "t1k_support_end")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=6000)


@pytest.fixture(scope="module")
def hit(table):
    return ref.hits(table.allele_off, table.aln, table.rec, table.text, table.ops, table.site_allele, table.site_pos)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(*ref.args(table))


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_analyzer_usage_lists_the_flags(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--siteSupport:" in r.stderr and "prefix_allele_support.tsv" in r.stderr and "--supportEnd INT:" in r.stderr


def _no_allele(tmp_path, extra):
    empty = tmp_path / "none_allele.tsv"
    empty.write_text("")
    o = str(tmp_path / "o")
    return o, subprocess.run([ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(empty), "-u", str(tmp_path / "r.fq"), "-o", o] + extra, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("value", ["512", "-1", "ten", "3x", ""])
def test_support_end_outside_its_range_is_refused_before_any_work(built, tmp_path, value):
    o, r = _no_allele(tmp_path, ["--siteSupport", "--supportEnd", value])
    assert r.returncode != 0 and "--supportEnd needs an integer from 0 to 511." in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o_")]               # not even the files of a run without a selected allele


def test_no_allele_selected_gives_the_header_alone(built, tmp_path):
    for extra in ([], ["--supportEnd", "0"], ["--supportEnd", "511"]):                     # (no --barcode needed)
        o, r = _no_allele(tmp_path, ["--siteSupport"] + extra)
        assert r.returncode == 0, r.stderr
        assert open(o + "_allele_support.tsv").read() == ref.HEADER + "\n"
        os.remove(o + "_allele_support.tsv")
    o, r = _no_allele(tmp_path, [])
    assert r.returncode == 0 and not os.path.exists(o + "_allele_support.tsv")             # without the flag the file is not written


def test_sites_are_taken_with_the_flag_alone(built, tmp_path):
    sites = str(tmp_path / "sites.tsv")
    open(sites, "w").write("")
    _, r = _no_allele(tmp_path, ["--sites", sites, "--siteSupport"])
    assert r.returncode == 0 and "--sites has no meaning" not in r.stderr


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_support_symbols_declared_exported_and_bound(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(t1k_ctx \*ctx" % name, header, flags=re.M), name
        assert hasattr(L, name), name
    assert "} t1k_support_rec;" in header and "} t1k_support_book;" in header
    assert all(hasattr(t1k_amd.Context, n) for n in ("support", "support_begin", "support_add", "support_get", "support_stats", "support_end"))
    assert t1k_amd.SUPPORT_REC_DTYPE.names == ("read_len", "clip_front", "strand") and t1k_amd.SUPPORT_BOOK_DTYPE.names == ("flags", "t_start", "t_end")
    assert t1k_amd.SUPPORT_REC_DTYPE.itemsize == 12 and t1k_amd.SUPPORT_BOOK_DTYPE.itemsize == 12


def test_support_kernels_use_no_scratch(tmp_path):
    """both instantiations of k_support, compiled for gfx950 with the Makefile's flags: no scratch memory, no spilled register, no LDS"""
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_support.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_support.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    kernels = kernel_metadata(open(out).read())
    for pattern in (r"_Z9k_supportILb0EE", r"_Z9k_supportILb1EE"):
        mine = [k for k in kernels if re.match(pattern, k)]
        assert len(mine) == 1, (pattern, sorted(kernels))
        k = kernels[mine[0]]
        print("%s: %s VGPRs, %s SGPRs, %s + %s spilled, %s bytes of scratch" % (mine[0], k[".vgpr_count"], k[".sgpr_count"], k[".vgpr_spill_count"], k[".sgpr_spill_count"],
                                                                                k[".private_segment_fixed_size"]))
        assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".group_segment_fixed_size"]) == 0, (mine[0], k)
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, (mine[0], k)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_vectorised_restatement_equals_the_loops():
    t = ref.generate(seed=3, records=250)
    a, b = ref.restate(*ref.args(t)), ref.restate_by_loops(*ref.args(t))
    assert len(a.a) > 1000 and len(a.b) > 1000 and ref.same(a, b)


def test_runs_round_trip_through_both_families(want, table):
    """the key layouts of t1k_support_get: a cell's uniq bookings under the even key of family A, the others under the odd one; family B from
    2^57 on, one run per template"""
    keys, counts = ref.expected_runs(want)
    assert keys == sorted(set(keys)) and min(counts) > 0
    n_a = sum(1 for k in keys if k < ref.FAMILY_B)
    assert 0 < n_a < len(keys) and max(keys[:n_a]) < 2 ** 57 <= min(keys[n_a:]) and max(keys) < 2 ** 58
    assert sum(counts[:n_a]) == sum(counts[n_a:])                                         # every (hit, booking) once in either family
    assert ref.same(ref.from_runs(keys, counts, len(table.site_allele)), want)
    # by hand: two uniq and one other booking of one cell, two of them from one template
    t = ref.from_runs([((((3 * 7 + 5) * 2 + 1) * 2 + 0) * 512 + 9) * 2, ((((3 * 7 + 5) * 2 + 1) * 2 + 0) * 512 + 9) * 2 + 1,
                       2 ** 57 | (((3 * 7 + 5) * 2 + 1) << 24) | (7 << 12) | 4095, 2 ** 57 | (((3 * 7 + 5) * 2 + 1) << 24) | (8 << 12) | 4095], [2, 1, 2, 1], 4)
    assert t.a == {(3, 5, 1, 0, 9): [3, 2]} and t.b == {(3, 5, 1, 7, 4095): 2, (3, 5, 1, 8, 4095): 1}
    assert ref.lines(t) == {(3, 5): (3, 2, 0, 3, 3, 0, 9, 9, 3, 2)} and ref.lines(t, end=9)[(3, 5)][8] == 0


def test_family_a_summed_is_the_pileup_at_the_sites(table, want):
    """with w_all / w_uniq = a record's bookings / its uniq bookings, family A summed over strand, mate and d is the per-base pileup -- at the
    sites; the restatement holds nothing anywhere else"""
    aln = table.aln.copy()
    bp = table.book_ptr.astype(np.int64)
    uq = np.concatenate([[0], np.cumsum(table.book["flags"] & 1)])
    aln["w_all"], aln["w_uniq"] = np.diff(bp), uq[bp[1:]] - uq[bp[:-1]]
    pile = pileup_ref.book(table.allele_off, aln, table.text, table.ops).astype(np.int64)
    g = sitepile_ref.site_cells(table.allele_off, table.site_allele, table.site_pos)
    got = np.zeros_like(pile)
    for (s, state, _, _, _), (n, u) in want.a.items():
        got[state, g[s]] += n
        got[7 + state, g[s]] += u
    at = np.zeros(pile.shape[1], bool)
    at[g] = True
    assert np.array_equal(got[:, at], pile[:, at]) and not got[:, ~at].any() and pile[:, ~at].any()
    rows = ref.lines(want)
    assert all(r[0] == r[2] + r[3] == r[4] + r[5] and r[1] <= r[0] and 1 <= r[9] <= r[0] and r[6] <= r[7] <= 511 and r[8] <= r[0] for r in rows.values())
    assert {k for k in rows} == {(s, state) for s, state in zip(*np.nonzero(pile[:7, g].T))}


def test_table_covers_the_cases(table, hit, want):
    off = table.allele_off.astype(np.int64)
    assert table.allele_len == [1, 63, 64, 65, 1000, 4097, 9000] and len(table.aln) == 6003 and table.records == 6000
    rec, book = table.rec, table.book
    length, clip = rec["read_len"].astype(np.int64), rec["clip_front"].astype(np.int64)
    # hits in the first and the last column of a 64-column step, and in steps behind the first
    assert ((hit.col % 64) == 0).sum() > 100 and ((hit.col % 64) == 63).sum() > 30 and (hit.col >= 128).sum() > 100
    # an insert as first op books at seq_start (nothing consumed yet)
    first_ins = (hit.col == 0) & (hit.op == 2)
    assert first_ins.sum() > 10 and (hit.pos[first_ins] == np.minimum(table.aln["seq_start"][hit.rec[first_ins]], np.diff(off)[table.aln["allele"][hit.rec[first_ins]]] - 1)).all()
    # deletion columns at c == 0 and at c == L: d = 0 from either side
    dele = hit.op == 3
    assert (dele & (hit.c == 0)).sum() > 10 and (dele & (hit.c == length[hit.rec])).sum() > 5 and (hit.d[dele & (hit.c == length[hit.rec])] == 0).all()
    # d == 0 at both read ends, on consumed bases
    base = hit.op != 3
    assert (base & (hit.c == 0)).sum() > 30 and (base & (hit.c == length[hit.rec] - 1) & (hit.c > 0)).sum() > 30
    # read-ends of 1100 bases and more with 520 and more in front of the window: d saturates
    deep = (length[hit.rec] >= 1100) & (clip[hit.rec] >= 520)
    assert deep.sum() > 1000 and (hit.raw_d[deep] > 511).sum() > 1000 and (hit.d[hit.raw_d > 511] == 511).all() and hit.raw_d.max() >= 520
    assert len(np.unique(hit.d)) > 500                                                   # nearly every stored distance occurs
    # templates on the 9000-base allele that reach more than 4095 bases to either side of a site: both clamps act
    rep, at = ref.bookings(hit, table.book_ptr)
    pos = hit.pos[rep]
    ds, de = pos - book["t_start"].astype(np.int64)[at], book["t_end"].astype(np.int64)[at] - pos
    assert (ds > 4095).sum() > 100 and (de > 4095).sum() > 100 and ((ds > 4095) & (de > 4095)).sum() > 100
    assert (ds < 0).sum() > 100 and (de < 0).sum() > 100                                 # and templates that do not hold the site: clamped at 0
    assert sum(1 for k in want.b if k[3] == 4095) > 10 and sum(1 for k in want.b if k[4] == 4095) > 10 and sum(1 for k in want.b if k[3] == 0 or k[4] == 0) > 10
    # the three special sites: 200 bookings of one template, 200 of 200, two templates that differ only beyond the clamp
    rows = ref.lines(want)
    ins = ref.STATES.index("+")
    assert rows[(table.special["one"], ins)][0] == 200 and rows[(table.special["one"], ins)][9] == 1
    assert rows[(table.special["all"], ins)][0] == 200 and rows[(table.special["all"], ins)][9] == 200
    far = table.book[int(table.book_ptr[-2]):]
    assert len(far) == 2 and (far["t_start"][0], far["t_end"][0]) != (far["t_start"][1], far["t_end"][1]) and far["flags"][0] == far["flags"][1]
    assert rows[(table.special["far"], ins)][0] == 2 and rows[(table.special["far"], ins)][9] == 1
    assert sum(1 for r in rows.values() if r[9] < r[0]) > 100 and sum(1 for r in rows.values() if r[9] == r[0] > 1) > 100
    # both strands, both mates, both orients and both uniq flags on one site
    full = {}
    for (s, _, strand, mate, _), (n, u) in want.a.items():
        full.setdefault(s, set()).update({("strand", strand), ("mate", mate)} | ({("uniq", 1)} if u else set()) | ({("uniq", 0)} if n > u else set()))
    for (s, _, orient, _, _) in want.b:
        full[s].add(("orient", orient))
    assert sum(1 for v in full.values() if len(v) == 8) > 100
    # bookings: records with hits and none, lists of 0 .. 5 and of 200
    per_rec = np.bincount(hit.rec, minlength=len(table.aln))
    n = np.diff(table.book_ptr.astype(np.int64))
    assert ((n == 0) & (per_rec > 0)).sum() > 100 and (n == 200).sum() == 8 and set(np.unique(n[n < 200])) == set(range(6))
    assert (per_rec == 0).sum() > 100 and per_rec.max() >= 48
    keys = 2 * int((per_rec * n).sum())
    assert keys == sum(v[0] for v in want.a.values()) + sum(want.b.values())
    assert 50000 <= keys <= 2000000                                                      # the keys the kernel emits


def test_table_text_round_trip(tmp_path):
    t = ref.Table()
    # four bookings at d = 2, 2, 7, 9: the lower median of an even count is the second; three of them from one template
    t.a = {(0, 2, 0, 0, 2): [2, 1], (0, 2, 1, 1, 7): [1, 0], (0, 2, 1, 0, 9): [1, 1], (2, 6, 0, 1, 511): [3, 3], (1, 5, 1, 1, 0): [1, 0]}
    t.b = {(0, 2, 0, 5, 9): 3, (0, 2, 1, 5, 9): 1, (2, 6, 0, 4095, 0): 3, (1, 5, 0, 1, 1): 1}
    rows = ref.lines(t, end=8)
    assert rows[(0, 2)] == (4, 2, 2, 2, 3, 1, 2, 2, 3, 2) and rows[(2, 6)] == (3, 3, 3, 0, 0, 3, 511, 511, 0, 1)
    text = ref.table_text(["X*01", "Y*02"], ["ACG", "TN"], [[1, 0, 1], [0, 1]], [0, 0, 1], [0, 2, 1], {(0, 2): "T", (1, 1): "A,C"}, rows)
    p = tmp_path / "t.tsv"
    p.write_text(text)
    header, got = ref.parse(str(p))
    assert header == ref.HEADER
    assert [r[:6] for r in got] == [("X*01", 1, 1, "A", ".", "G"), ("X*01", 3, 2, "G", "T", "-"), ("Y*02", 2, 1, "N", "A,C", "+")]
    assert got[0][6] == dict(zip(ref.COLUMNS, rows[(0, 2)])) and got[0][6]["end_med"] == 2 and got[0][6]["templates"] == 2 < got[0][6]["count"]
    assert got[2][6]["end_min"] == 511 and got[2][6]["near_end"] == 0


def test_analyzer_records():
    ptr, asg, ops = pileup_ref.assignments([
        [(0, pileup_ref.overlap(0, 1, 4, 2, 5, -1), [0, 0, 1, 0], pileup_ref.overlap(0, 0, 2, 7, 9), [0, 0, 0])],
        [(0, pileup_ref.overlap(0, 0, 3, 0, 3), [0] * 4), (1, pileup_ref.overlap(1, 0, 3, 1, 4), [0] * 4, None, [], 1)]])
    aln, text, rec, book_ptr, book = ref.analyzer_records(ptr, asg, ["ACGTA", "ACGT"], ["TTT", "GGGG"])
    assert len(aln) == 4 and book_ptr.tolist() == [0, 1, 2, 3, 4]
    assert rec.tolist() == [(5, 1, 1), (3, 0, 0), (4, 0, 0), (4, 0, 0)]
    # uniq | mate << 1 | orient << 2: a pair with file 1 on the reverse strand; a file-1 end alone; a file-2 end alone on the forward strand
    assert book.tolist() == [(1 | 4, 2, 9), (1 | 2 | 4, 2, 9), (0, 0, 3), (2 | 4, 1, 4)]
