"""CPU tests (no GPU) of the per-barcode pileup at sites (analyzer --barcodePileup, t1k_sitepile_*): the command line, the
C-ABI export, and the sequential restatement (sitepile_ref) the GPU tests compare the kernel and the analyzer against -- summed over
barcodes it is the per-base pileup at the sites -- with the cases its generated table has to cover."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pileup_ref
import sitepile_ref as ref
import util
import t1k_amd

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=30000)


@pytest.fixture(scope="module")
def hit(table):
    return ref.hits(table.allele_off, table.aln, table.text, table.ops, table.site_allele, table.site_pos)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(table.allele_off, table.aln, table.book_ptr, table.book, table.text, table.ops, table.site_allele, table.site_pos)


def test_analyzer_usage_lists_the_flags(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--barcodePileup:" in r.stderr and "prefix_barcode_pileup.tsv" in r.stderr and "--sites FILE:" in r.stderr


def test_barcode_pileup_needs_barcode(built, tmp_path):
    o = str(tmp_path / "o")
    r = subprocess.run([ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(tmp_path / "a.tsv"), "-u", str(tmp_path / "r.fq"), "-o", o, "--barcodePileup"],
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "--barcodePileup needs --barcode." in r.stderr
    assert not os.path.exists(o + "_barcode_pileup.tsv")


def test_no_allele_selected_gives_the_header_alone(built, tmp_path):
    empty = tmp_path / "none_allele.tsv"
    empty.write_text("")
    o = str(tmp_path / "o")
    r = subprocess.run([ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(empty), "-u", str(tmp_path / "r.fq"), "--barcode", str(tmp_path / "bc.fa"), "-o", o,
                        "--barcodePileup"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert open(o + "_barcode_pileup.tsv").read() == ref.HEADER + "\n"


def test_sitepile_symbols_exported(built):
    L = C.CDLL(t1k_amd.lib_path())
    for name in ("t1k_sitepile_begin", "t1k_sitepile_add", "t1k_sitepile_get", "t1k_sitepile_stats", "t1k_sitepile_end"):
        assert hasattr(L, name), name
    assert all(hasattr(t1k_amd.Context, n) for n in ("sitepile", "sitepile_begin", "sitepile_add", "sitepile_get", "sitepile_end"))


def test_sum_over_barcodes_is_the_pileup_at_the_sites(table, want):
    """with w_all / w_uniq = a record's bookings / its uniq bookings, the per-base pileup is the sum over barcodes -- at the sites; the
    restatement holds nothing anywhere else"""
    aln = table.aln.copy()
    bp = table.book_ptr.astype(np.int64)
    uq = np.concatenate([[0], np.cumsum(table.book & 1)])
    aln["w_all"], aln["w_uniq"] = np.diff(bp), uq[bp[1:]] - uq[bp[:-1]]
    pile = pileup_ref.book(table.allele_off, aln, table.text, table.ops).astype(np.int64)
    got = ref.dense(want, table.allele_off, table.site_allele, table.site_pos)
    g = ref.site_cells(table.allele_off, table.site_allele, table.site_pos)
    at = np.zeros(pile.shape[1], bool)
    at[g] = True
    assert np.array_equal(got[:, at], pile[:, at]) and not got[:, ~at].any() and pile[:, ~at].any()
    assert all(c[:7].sum() > 0 and (c[7:] <= c[:7]).all() for c in want.values())


def test_vectorised_restatement_equals_the_loops():
    t = ref.generate(seed=3, records=250)
    args = (t.allele_off, t.aln, t.book_ptr, t.book, t.text, t.ops, t.site_allele, t.site_pos)
    a, b = ref.restate(*args), ref.restate_by_loops(*args)
    assert len(a) > 100 and ref.same(a, b)


def test_runs_round_trip(want, table):
    """the key layout of t1k_sitepile_get: a cell's uniq bookings under the even key, the others under the odd one"""
    n_sites = len(table.site_allele)
    keys, counts = [], []
    for (b, s), c in sorted(want.items()):
        for plane in range(7):
            for uniq, v in ((1, c[7 + plane]), (0, c[plane] - c[7 + plane])):
                if v:
                    keys.append(((b * n_sites + s) * 7 + plane) * 2 + (1 - uniq))
                    counts.append(v)
    assert keys == sorted(keys) and ref.same(ref.from_runs(keys, counts, n_sites), want)


def test_table_covers_the_cases(table, hit, want):
    off = table.allele_off.astype(np.int64)
    assert table.allele_len == [1, 63, 64, 65, 1000, 4097] and len(table.aln) == 30000
    g = ref.site_cells(table.allele_off, table.site_allele, table.site_pos)
    sites = set(g.tolist())
    assert all(p in sites for p in range(0, 193))                                        # the four short alleles, whole
    assert all(int(off[a + 1]) - 1 in sites for a in range(6))                           # the last position of every allele
    assert all(int(off[5]) + p in sites for k in range(64, 4097, 64) for p in (k - 1, k, k + 1) if p < 4097)
    assert all(p in sites for p in range(table.full_word * 64, table.full_word * 64 + 64)) and all(p in sites for p in range(*table.dense))
    assert 0.1 < len(g) / off[-1] < 0.25 and any(off[a] % 64 for a in range(1, 6))      # sparse; allele boundaries inside bitmap words
    # hits in the first and the last column of a 64-column step, and in steps behind the first
    assert ((hit.col % 64) == 0).sum() > 100 and ((hit.col % 64) == 63).sum() > 100 and (hit.col >= 128).sum() > 100
    assert (hit.plane == ref.INS).sum() > 100 and (hit.plane == ref.DEL).sum() > 100 and (hit.plane == ref.N).sum() > 10
    # an insert as first op books at seq_start (nothing consumed yet)
    first_ins = (hit.col == 0) & (hit.op == 2)
    assert first_ins.sum() > 10 and (hit.cell[first_ins] == off[table.aln["allele"][hit.rec[first_ins]]] + table.aln["seq_start"][hit.rec[first_ins]]).sum() > 10
    per_rec = np.bincount(hit.rec, minlength=len(table.aln))
    assert (per_rec == 0).sum() > 100 and per_rec.max() >= 48                            # records that touch no site; a full dense stretch
    in_dense = (hit.cell >= table.dense[0]) & (hit.cell < table.dense[1])
    assert in_dense.mean() > 0.3
    # bookings: empty lists, lists of 200, one barcode with about half of all bookings, both uniq flags
    n = np.diff(table.book_ptr.astype(np.int64))
    assert (n == 0).sum() > 1000 and (n == 200).sum() == 12 and set(np.unique(n[n < 200])) == set(range(6))
    assert ((n == 0) & (per_rec > 0)).sum() > 100                                        # hits without a booking emit nothing
    bc = table.book >> 1
    assert 0.45 < (bc == table.hot_barcode).mean() < 0.55 and len(np.unique(bc)) == table.n_barcodes == 300
    assert 0.2 < (table.book & 1).mean() < 0.45
    assert len({b for b, _ in want}) == 300 and sum(int(c[:7].sum()) for c in want.values()) == int((per_rec * n).sum())
    assert 100000 < int((per_rec * n).sum()) < 4000000                                   # the keys the kernel emits: a few folds' worth, not a benchmark


def test_table_text_round_trip(tmp_path):
    cells = {(1, 0): np.arange(14), (0, 2): np.arange(14) + 3, (0, 1): np.arange(14) * 2}
    text = ref.table_text(["bcA", "bcB"], ["X*01", "Y*02"], ["ACG", "TN"], [[1, 0, 1], [0, 1]], [0, 0, 1], [0, 2, 1], {(0, 2): "T", (1, 1): "A,C"}, cells)
    p = tmp_path / "t.tsv"
    p.write_text(text)
    header, rows = ref.parse(str(p))
    assert header == ref.HEADER
    assert [r[:6] for r in rows] == [("bcA", "X*01", 3, 2, "G", "T"), ("bcA", "Y*02", 2, 1, "N", "A,C"), ("bcB", "X*01", 1, 1, "A", ".")]
    assert rows[0][6]["A"] == 0 and rows[0][6]["ins_uniq"] == 26 and rows[1][6]["C"] == 4
    assert ref.barcode_ids(["b", "a", "b", "c"]) == (["b", "a", "c"], [0, 1, 0, 2])
