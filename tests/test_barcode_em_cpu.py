"""CPU tests (no GPU) of the per-barcode allele EM (analyzer --barcodeEM, t1k_barcode_em): the analyzer's usage and argument checks,
the C-ABI export, and the invariants of the sequential restatement the GPU tests compare the kernel against (barcode_em_ref)."""
import ctypes as C
import os
import subprocess

import numpy as np

import barcode_em_ref as ref
import goldens
import util
import t1k_amd

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")


def test_analyzer_usage_lists_the_barcode_em_flags(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--barcodeEM:" in r.stderr and "--barcodeEMPrior FLOAT" in r.stderr


def test_analyzer_barcode_em_usage_errors(built, tmp_path):
    base = [ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(tmp_path / "a.tsv"), "-u", str(tmp_path / "r.fq"), "-o", str(tmp_path / "o")]
    r = subprocess.run(base + ["--barcodeEM"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--barcode" in r.stderr
    r = subprocess.run(base + ["--barcode", str(tmp_path / "bc.fa"), "--barcodeEM", "--barcodeEMPrior", "-0.5"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--barcodeEMPrior" in r.stderr
    assert not os.path.exists(str(tmp_path / "o_barcode_em.tsv"))


def test_analyzer_barcode_em_nothing_genotyped(built, tmp_path):
    """no allele selected: the analyzer touches no GPU and writes header-only tables"""
    c = goldens.Case("hla_synth_2x150", str(tmp_path))
    empty = os.path.join(str(tmp_path), "empty_allele.tsv")
    open(empty, "w").close()
    o = os.path.join(str(tmp_path), "o")
    r = subprocess.run([ANALYZER, "-f", c.ref, "-a", empty, "-1", c.r1, "-2", c.r2, "--barcode", os.path.join(str(tmp_path), "bc.fa"), "-o", o, "--barcodeEM"],
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert open(o + "_barcode_em.tsv").read() == "#barcode\n" == open(o + "_barcode_expr.tsv").read()


def test_barcode_em_symbol_exported(built):
    L = C.CDLL(t1k_amd.lib_path())
    assert hasattr(L, "t1k_barcode_em")
    assert hasattr(t1k_amd.Context, "barcode_em")


def _small():
    rng = np.random.default_rng(11)
    bcs = ref.random_table(rng, 300, n_alleles=30, max_list=6, fragments=6000)
    bcs[5] = []                                          # N_b = 0
    bcs[6] = [((3,), 4), ((7,), 1), ((9,), 2)]            # single-allele groups only
    bcs[7] = [((2, 5), 1)]                               # one fragment
    return ref.from_lists(bcs)


def test_restatement_rows_sum_to_the_barcode_fragments():
    t = _small()
    n, iters = ref.restate(t)
    L, G, _ = t.sizes()
    N = np.bincount(np.repeat(np.arange(t.n_barcodes), G), weights=t.group_count, minlength=t.n_barcodes)
    rows = np.bincount(np.repeat(np.arange(t.n_barcodes), L), weights=n, minlength=t.n_barcodes)
    assert np.allclose(rows, N, rtol=1e-12, atol=0)
    assert (iters[N > 0] >= 1).all() and iters.max() <= 1000


def test_restatement_single_allele_groups_are_exact():
    t = _small()
    n, iters = ref.restate(t)
    a0 = int(t.bc_allele_ptr[6])
    assert n[a0:a0 + 3].tolist() == [4.0, 1.0, 2.0]
    a0 = int(t.bc_allele_ptr[7])
    assert n[a0:a0 + 2].tolist() == [0.5, 0.5] and iters[7] == 1   # a single group: the even split is already the fixed point


def test_restatement_alpha_zero_ignores_rho():
    t = _small()
    rng = np.random.default_rng(3)
    n0, i0 = ref.restate(t)
    n1, i1 = ref.restate(t, rho=rng.random(30), alpha=0.0)
    assert np.array_equal(n0, n1) and np.array_equal(i0, i1)
    n2, _ = ref.restate(t, rho=rng.random(30), alpha=2.0)
    assert not np.array_equal(n0, n2)


def test_restatement_counts_updates():
    t = _small()
    n, iters = ref.restate(t)
    assert iters[5] == 0 and not n[int(t.bc_allele_ptr[5]):int(t.bc_allele_ptr[6])].any()
    _, capped = ref.restate(t, max_iter=3)
    assert capped.max() == 3 and (capped <= np.minimum(iters, 3)).all() and (capped == np.minimum(iters, 3)).all()
