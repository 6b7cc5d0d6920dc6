"""GPU tests of the per-barcode allele EM (t1k_barcode_em, analyzer --barcodeEM): the kernel against the sequential
restatement bit for bit, the analyzer's new table on the golden chain, and the case the feature exists for -- a cell that lost an allele."""
import os
import subprocess

import numpy as np
import pytest

import barcode_em_ref as ref
import goldens
import util
import t1k_amd

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
N_ALLELES = 60


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(20)
    bcs = ref.random_table(rng, 20000, n_alleles=N_ALLELES, max_list=12, fragments=200000, big_share=0.3)
    bcs[1] = []                    # N_b = 0
    bcs[2] = [((17,), 1)]          # one fragment
    bcs[3] = [((4, 9), 1)]         # one fragment, two alleles
    return ref.from_lists(bcs)


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _run(ctx, t, monkeypatch, lds=None, **kw):
    if lds is None:
        monkeypatch.delenv("T1K_BARCODE_EM_LDS", raising=False)
    else:
        monkeypatch.setenv("T1K_BARCODE_EM_LDS", str(lds))
    rho = kw.pop("rho", None)
    return ctx.barcode_em(*t.args(), rho, N_ALLELES, **kw)


def test_table_covers_the_cases(table):
    L, G, E = table.sizes()
    N = np.bincount(np.repeat(np.arange(table.n_barcodes), G), weights=table.group_count, minlength=table.n_barcodes)
    assert N[0] >= 0.3 * N.sum() - 1 and N[1] == 0 and N[2] == 1
    _, iters = ref.restate(table)
    assert (iters == 1000).sum() >= 10 and iters[1] == 0


@pytest.mark.parametrize("alpha", [0.0, 0.5, 5.0])
def test_kernel_equals_restatement_bit_for_bit(ctx, table, monkeypatch, alpha):
    rho = np.random.default_rng(7).random(N_ALLELES)
    rho /= rho.sum()
    want_n, want_it = ref.restate(table, rho=rho, alpha=alpha)
    n, it, ms = _run(ctx, table, monkeypatch, rho=rho if alpha else None, alpha=alpha)
    assert np.array_equal(it, want_it)
    assert np.array_equal(n.view(np.uint64), want_n.view(np.uint64))
    # the global-memory shape for at least 10 % of the barcodes: the same doubles
    L, G, E = table.sizes()
    words = ref.lds_words(L, G, E)
    budget = int(np.percentile(words, 85))
    assert (words > budget).mean() >= 0.10
    n2, it2, _ = _run(ctx, table, monkeypatch, lds=budget, rho=rho if alpha else None, alpha=alpha)
    assert np.array_equal(it2, want_it) and np.array_equal(n2.view(np.uint64), want_n.view(np.uint64))


def test_kernel_max_iter_and_slices(ctx, table, monkeypatch):
    want_n, want_it = ref.restate(table, max_iter=4)
    n, it, _ = _run(ctx, table, monkeypatch, max_iter=4)
    assert it.max() == 4 and np.array_equal(it, want_it) and np.array_equal(n.view(np.uint64), want_n.view(np.uint64))
    # a slice of the barcodes: their offsets, every other array whole; the results land at the same absolute positions
    full_n, full_it = ref.restate(table)
    b0, b1 = 100, 2100
    ap, al, gp, gc, ep, el = table.args()
    out = np.full(len(al), -1.0)
    iters = np.zeros(b1 - b0, np.int32)
    import ctypes as C
    ms = C.c_double()
    sub_ap, sub_gp = np.ascontiguousarray(ap[b0:b1 + 1]), np.ascontiguousarray(gp[b0:b1 + 1])
    rc = t1k_amd.lib().t1k_barcode_em(ctx.h, b1 - b0, t1k_amd.capi._ptr(sub_ap), t1k_amd.capi._ptr(al), t1k_amd.capi._ptr(sub_gp), t1k_amd.capi._ptr(gc),
                                      t1k_amd.capi._ptr(ep), t1k_amd.capi._ptr(el), None, N_ALLELES, 0.0, 1e-7, 1000, t1k_amd.capi._ptr(out),
                                      t1k_amd.capi._ptr(iters), C.byref(ms))
    assert rc == 0
    lo, hi = int(ap[b0]), int(ap[b1])
    assert np.array_equal(out[lo:hi].view(np.uint64), full_n[lo:hi].view(np.uint64)) and (out[:lo] == -1).all() and (out[hi:] == -1).all()
    assert np.array_equal(iters, full_it[b0:b1])


def test_kernel_argument_errors(ctx):
    good = ref.from_lists([[((1, 3), 2), ((3,), 1)], [((0,), 1)]])
    ap, al, gp, gc, ep, el = good.args()
    assert ctx.barcode_em(ap, al, gp, gc, ep, el, None, 5, raw=True) == 0

    def rc(**over):
        a = dict(bc_allele_ptr=ap, bc_allele=al, bc_group_ptr=gp, group_count=gc, group_entry_ptr=ep, entry_local=el, rho=None, n_alleles=5)
        a.update(over)
        return ctx.barcode_em(a.pop("bc_allele_ptr"), a.pop("bc_allele"), a.pop("bc_group_ptr"), a.pop("group_count"), a.pop("group_entry_ptr"),
                              a.pop("entry_local"), a.pop("rho"), a.pop("n_alleles"), raw=True, **a)
    assert rc(n_alleles=3) < 0                                        # allele id out of range
    assert rc(bc_allele=np.array([3, 1, 0], np.uint32)) < 0           # not ascending
    assert rc(entry_local=np.array([1, 0, 1, 0], np.uint32)) < 0      # group list not ascending
    assert rc(entry_local=np.array([0, 2, 1, 0], np.uint32)) < 0      # outside U_b
    assert rc(group_count=np.array([2.0, 0.0, 1.0])) < 0               # count 0
    assert rc(group_count=np.array([2.0, np.nan, 1.0])) < 0
    assert rc(group_entry_ptr=np.array([0, 2, 2, 4], np.uint64)) < 0  # empty group
    assert rc(bc_group_ptr=np.array([0, 2, 1], np.uint64)) < 0        # offsets decrease
    assert rc(alpha=1.0) < 0                                          # alpha > 0 without rho
    assert rc(alpha=-1.0) < 0
    assert rc(max_iter=0) < 0
    assert rc(tol=float("nan")) < 0


# ---- the analyzer ------------------------------------------------------------------------------------------------------------------
def _table(path):
    lines = open(path).read().split("\n")
    head = lines[0].split("\t")
    rows = [l.split("\t") for l in lines[1:] if l]
    return head, rows


def _check_em_against_expr(em_path, expr_path):
    eh, er = _table(em_path)
    xh, xr = _table(expr_path)
    A = (len(xh) - 1) // 2
    assert eh == xh[:A + 1] and len(er) == len(xr) > 0
    uniq_rows = 0
    for e, x in zip(er, xr):
        assert e[0] == x[0] and len(e) == A + 1
        frac = np.array([float(v) for v in x[1:A + 1]])
        uniq = np.array([float(v) for v in x[A + 1:]])
        assert abs(sum(float(v) for v in e[1:]) - frac.sum()) <= 1e-5
        if np.array_equal(frac, uniq):   # every fragment of the barcode is unique: the EM has nothing to move
            assert e[1:] == x[1:A + 1]
            uniq_rows += 1
    return uniq_rows


@pytest.mark.parametrize("mode", [[], ["--varMaxGroup", "0"], ["--varMaxGroup", "0", "--barcodeEMPrior", "1"]])
def test_analyzer_barcode_em_on_the_golden_chain(built, tmp_path, mode):
    c = goldens.Case("hla_synth_2x150", str(tmp_path))
    g = os.path.join(str(tmp_path), "g")
    r = subprocess.run([GENO] + c.args() + ["-o", g], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    base = [ANALYZER, "-f", c.ref, "-a", g + "_allele.tsv", "-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa", "--barcode", g + "_aligned_bc.fa"] + c.flags + mode
    plain, flag, env = (os.path.join(str(tmp_path), x) for x in ("plain", "flag", "env"))
    r = subprocess.run(base + ["-o", plain], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(plain + "_barcode_em.tsv")
    r = subprocess.run(base + ["-o", flag, "--barcodeEM"], stderr=subprocess.PIPE, text=True, env=dict(os.environ, T1K_DEBUG_PHASES="1"))
    assert r.returncode == 0, r.stderr
    assert "barcode EM: groups built" in r.stderr
    r = subprocess.run(base + ["-o", env], stderr=subprocess.PIPE, text=True, env=dict(os.environ, T1K_BARCODE_EM="1"))
    assert r.returncode == 0, r.stderr
    for o in (flag, env):
        assert open(o + "_barcode_expr.tsv").read() == open(plain + "_barcode_expr.tsv").read()
        assert open(o + "_allele.vcf").read() == open(plain + "_allele.vcf").read()
    if not mode:
        assert open(flag + "_barcode_expr.tsv").read() == c.expected("analyzer_barcode_expr.tsv")
    assert open(flag + "_barcode_em.tsv").read() == open(env + "_barcode_em.tsv").read()
    assert _check_em_against_expr(flag + "_barcode_em.tsv", flag + "_barcode_expr.tsv") >= 1


# ---- loss of an allele -------------------------------------------------------------------------------------------------------------
def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def test_lost_allele_is_recovered_per_barcode(built, tmp_path):
    tmp = str(tmp_path)
    full = os.path.join(tmp, "full.fa")
    util.synth_ref("ref-rna", full, genes=2, scale=0.02, seed=4)
    recs = util.read_fa(full)
    x1 = max((r for r in recs if r[0].startswith("HLA-A*")), key=lambda r: len(r[2]))
    seq1 = x1[2]
    assert "N" not in seq1 and len(seq1) > 700
    # X2: X1's first half, then a copy of X1 with every 20th base changed (5 %): the fragments of the first half align to both
    mid = len(seq1) // 2
    swap = {"A": "C", "C": "G", "G": "T", "T": "A"}
    seq2 = seq1[:mid] + "".join(swap[b] if (i % 20 == 7) else b for i, b in enumerate(seq1[mid:]))
    name2 = "HLA-A*99:99:99:99"
    ref_fa = os.path.join(tmp, "ref.fa")
    with open(ref_fa, "w") as f:
        f.write(x1[1] + "\n" + seq1 + "\n")
        f.write(">" + name2 + x1[1][len(x1[0]) + 1:] + "\n" + seq2 + "\n")
    rng = np.random.default_rng(9)
    bcs = ["".join(rng.choice(list("ACGT"), 16)) for _ in range(200)]
    r1, r2, bc = open(os.path.join(tmp, "r_1.fq"), "w"), open(os.path.join(tmp, "r_2.fq"), "w"), open(os.path.join(tmp, "r_bc.fa"), "w")
    i = 0
    for b in range(200):
        mixed = b < 100
        for _ in range(24):
            src = seq2 if (mixed and rng.random() < 0.5) else seq1
            flen = int(rng.integers(280, 341))
            st = int(rng.integers(0, len(src) - flen + 1))
            frag = src[st:st + flen]
            e1, e2 = frag[:150], _revcomp(frag)[:150]
            r1.write("@r%d/1\n%s\n+\n%s\n" % (i, e1, "I" * len(e1)))
            r2.write("@r%d/2\n%s\n+\n%s\n" % (i, e2, "I" * len(e2)))
            bc.write(">r%d\n%s\n" % (i, bcs[b]))
            i += 1
    for h in (r1, r2, bc):
        h.close()
    g, a = os.path.join(tmp, "g"), os.path.join(tmp, "a")
    r = subprocess.run([GENO, "-f", ref_fa, "-1", os.path.join(tmp, "r_1.fq"), "-2", os.path.join(tmp, "r_2.fq"), "--barcode", os.path.join(tmp, "r_bc.fa"), "-o", g],
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    selected = [l.split()[0] for l in open(g + "_allele.tsv") if l.strip()]
    assert x1[0] in selected and name2 in selected, selected       # precondition: both alleles genotyped
    r = subprocess.run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv", "-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa", "--barcode", g + "_aligned_bc.fa",
                        "-o", a, "--barcodeEM"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    xh, xr = _table(a + "_barcode_expr.tsv")
    eh, er = _table(a + "_barcode_em.tsv")
    c1, c2 = xh.index(x1[0]), xh.index(name2)
    assert eh[c1] == x1[0] and eh[c2] == name2
    mixed_bcs = set(bcs[:100])
    sums = {True: np.zeros(4), False: np.zeros(4)}   # expr X1, expr X2, em X1, em X2
    for x, e in zip(xr, er):
        assert x[0] == e[0]
        sums[x[0] in mixed_bcs] += [float(x[c1]), float(x[c2]), float(e[c1]), float(e[c2])]
    lost, mixed = sums[False], sums[True]
    # precondition: at least 20 % of X1's fragments in the X1-only cells also align to X2 (each gives X2 half its weight in the even split)
    assert 2 * lost[1] >= 0.2 * (lost[0] + lost[1]), lost
    assert lost[3] <= 0.25 * lost[1], lost
    assert mixed[3] >= 0.5 * mixed[1], mixed
