"""CPU tests (no GPU) of the UMI collapse (analyzer --umi, t1k_umi_collapse): the analyzer's usage and argument checks, the
C-ABI export, and the invariants of the sequential restatement the GPU tests compare the kernels against (umi_ref)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import umi_ref as ref
import util
import t1k_amd

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
GENE = np.array([0, 0, 0, 1, 1, 1], np.uint32)   # six alleles of two genes


def test_analyzer_usage_lists_the_umi_flags(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--umi FILE" in r.stderr and "--umiMismatch INT" in r.stderr


def test_analyzer_umi_argument_errors(built, tmp_path):
    base = [ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(tmp_path / "a.tsv"), "-u", str(tmp_path / "r.fq"), "-o", str(tmp_path / "o")]
    umi = tmp_path / "umi.fa"
    umi.write_text(">r1\nACGTACGTACGT\n>r2\nACGTACGTACGA\n")
    r = subprocess.run(base + ["--umi", str(umi)], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--umi needs --barcode." in r.stderr
    r = subprocess.run(base + ["--barcode", str(tmp_path / "bc.fa"), "--umi", str(umi), "--umiMismatch", "2"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--umiMismatch" in r.stderr
    long = tmp_path / "long.fa"
    long.write_text(">r1\nACGTACGTACGTACGT\n>r2\nACGTACGTACGTACGTA\n")
    r = subprocess.run(base + ["--barcode", str(tmp_path / "bc.fa"), "--umi", str(long)], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "UMIs of up to 16 bases" in r.stderr and "r2" in r.stderr
    assert glob.glob(str(tmp_path / "o_*")) == []


def test_umi_symbol_exported(built):
    L = C.CDLL(t1k_amd.lib_path())
    assert hasattr(L, "t1k_umi_collapse")
    assert hasattr(t1k_amd.Context, "umi_collapse")


def test_codes_order_like_text():
    assert int(ref.encode("ACGT")) == (4 << 32) | 0b00011011
    assert ref.encode("ACNT") == ref.NONE and ref.encode("missing_barcode") == ref.NONE and ref.encode("") == ref.NONE and ref.encode("A" * 17) == ref.NONE
    assert ref.decode(ref.encode("GATTACA")) == "GATTACA"
    assert (int(ref.encode("AAC")) < int(ref.encode("AAG"))) and (int(ref.encode("CAA")) > int(ref.encode("ATT")))


def _distinct_table(seed=5, n=400, rows=7):
    rng = np.random.default_rng(seed)
    umis = ref.distinct_umis(n, 8)
    frags = []
    for i in range(n):
        g = int(rng.integers(0, 2))
        k = int(rng.integers(1, 4))
        frags.append((int(rng.integers(0, rows)), umis[i], (3 * g + rng.choice(3, k, replace=False)).tolist()))
    return frags, rows


def test_distinct_umis_give_the_fragment_table():
    frags, rows = _distinct_table()
    us = [f[1] for f in frags]
    assert min(sum(a != b for a, b in zip(us[i], us[j])) for i in range(60) for j in range(i)) >= 2
    t = ref.from_fragments(frags, rows, GENE, 2)
    want_frac, want_uniq = ref.even_split(t)
    for mm in (0, 1):
        r = ref.restate(t, mm)
        assert len(r.mol_row) == t.n_frag and r.stats["corrected"] == 0 and r.stats["split"] == 0
        assert np.allclose(r.frac, want_frac, rtol=1e-12, atol=0) and np.array_equal(r.uniq, want_uniq)


def test_copies_of_every_fragment_change_nothing():
    frags, rows = _distinct_table(seed=6)
    one = ref.restate(ref.from_fragments(frags, rows, GENE, 2))
    many = ref.restate(ref.from_fragments(frags * 3, rows, GENE, 2))
    assert np.array_equal(many.frac.view(np.uint64), one.frac.view(np.uint64)) and np.array_equal(many.uniq, one.uniq)
    assert many.mol_lists == one.mol_lists and (many.mol_frags == 3).all()


def test_hand_worked_bucket():
    """counts 5, 2, 1, 1.  AAAC joins AAAA; ACAC ties with AAAC (one fragment each) and joins it as the larger code: a chain of two hops.
    AAGC (2 fragments) has AAAC as its only neighbour, whose count 1 < 2 * 2 - 1: it stays alone -- and AAAC, for which AAGC is a
    candidate, prefers AAAA's larger count."""
    frags = [(0, "AAAA", [0])] * 5 + [(0, "AAGC", [0])] * 2 + [(0, "AAAC", [0]), (0, "ACAC", [0])]
    t = ref.from_fragments(frags, 1, GENE, 2)
    r = ref.restate(t, 1)
    parent = {ref.decode(r.keys[i] & np.uint64(0xFFFFFFFF) | np.uint64(4 << 32)): ref.decode(r.keys[p] & np.uint64(0xFFFFFFFF) | np.uint64(4 << 32)) for i, p in enumerate(r.parent)}
    assert parent == {"AAAA": "AAAA", "AAAC": "AAAA", "ACAC": "AAAC", "AAGC": "AAGC"}
    assert r.hops.max() == 2 and r.ties == 1
    assert r.stats == dict(distinct=4, keys=2, corrected=2, split=0, no_umi=0)
    assert sorted(r.mol_frags.tolist()) == [2, 7] and r.frac[0, 0] == 2.0 and r.uniq[0, 0] == 2
    r0 = ref.restate(t, 0)
    assert sorted(r0.mol_frags.tolist()) == [1, 1, 2, 5] and r0.frac[0, 0] == 4.0
    # another length, another gene or another row is another bucket
    far = ref.restate(ref.from_fragments([(0, "AAAA", [0])] * 5 + [(0, "AAAC", [3]), (1, "AAAC", [0]), (0, "AAACA", [0])], 2, GENE, 2), 1)
    assert far.stats["corrected"] == 0 and len(far.mol_row) == 4


def test_empty_intersection_splits_by_distinct_list():
    t = ref.from_fragments([(0, "ACGT", [0, 1]), (0, "ACGT", [2]), (0, "ACGT", [0, 1]), (0, "TTTT", [0, 1]), (0, "TTTT", [1, 2]), (0, None, [2]), (0, None, [2])], 1, GENE, 2)
    r = ref.restate(t, 1)
    assert r.stats["split"] == 1 and r.stats["keys"] == 2 and r.stats["no_umi"] == 2
    assert r.mol_lists == [(0, 1), (2,), (1,), (2,), (2,)] and r.mol_frags.tolist() == [2, 1, 2, 1, 1]
    assert r.frag_mol.tolist() == [0, 1, 0, 2, 2, 3, 4]
    assert r.frac[0].tolist() == [0.5, 1.5, 3.0, 0, 0, 0] and r.uniq[0].tolist() == [0, 1, 3, 0, 0, 0]


def test_molecules_never_exceed_fragments():
    t = ref.generate(seed=3, fragments=3000, rows=40)
    lists = t.lists()
    total = sum(len(l) for l in lists)
    r = {mm: ref.restate(t, mm) for mm in (0, 1)}
    for mm in (0, 1):
        assert 0 < len(r[mm].mol_row) <= t.n_frag and r[mm].mol_frags.sum() == t.n_frag
        assert sum(len(l) for l in r[mm].mol_lists) <= total
        assert all(set(r[mm].mol_lists[m]) <= set(lists[f]) for f, m in enumerate(r[mm].frag_mol))
    assert r[1].stats["corrected"] > 0 and len(r[1].mol_row) < len(r[0].mol_row)
