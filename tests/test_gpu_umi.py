"""GPU tests of the UMI collapse (t1k_umi_collapse, analyzer --umi): the kernels against the sequential restatement --
partition, lists, unique counts and statistics exactly, frac bit for bit -- and the analyzer's molecule tables on the golden chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import umi_ref as ref
import util
import t1k_amd

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
COUNTS = ("distinct", "keys", "corrected", "split", "no_umi")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=11, fragments=200000, rows=2000, genes=6, per_gene=10)


@pytest.fixture(scope="module")
def want(table):
    return {mm: ref.restate(table, mm) for mm in (0, 1)}


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _same(got, w):
    assert np.array_equal(got["frag_mol"], w.frag_mol)                       # the partition, both sides in the canonical order
    assert np.array_equal(got["mol_row"], w.mol_row) and np.array_equal(got["mol_frags"], w.mol_frags)
    assert np.array_equal(np.diff(got["mol_list_ptr"].astype(np.int64)), [len(l) for l in w.mol_lists])
    assert np.array_equal(got["mol_list"], np.array([a for l in w.mol_lists for a in l], np.uint32))
    assert np.array_equal(got["uniq"], w.uniq)
    assert {k: got["stats"][k] for k in COUNTS} == w.stats
    assert np.array_equal(got["frac"].view(np.uint64), w.frac.view(np.uint64))


def test_table_covers_the_cases(table, want):
    w = want[1]
    assert w.buckets >= 5000 and w.stats["corrected"] > 0 and w.ties > 0 and w.stats["split"] > 0 and w.cross_gene > 0 and w.stats["no_umi"] > 0
    assert w.hops.max() >= 3 and w.max_bucket_fragments >= 8000 and w.lengths == [8, 10, 12]
    assert np.bincount(table.frag_row).max() >= 0.3 * table.n_frag - 1
    assert want[0].stats["corrected"] == 0 and want[0].stats["split"] > 0 and len(want[0].mol_row) > len(w.mol_row)
    # (one kernel shape per step: nothing to show in the statistics)


@pytest.mark.parametrize("mismatch", [0, 1])
def test_kernels_equal_restatement(ctx, table, want, mismatch):
    got = ctx.umi_collapse(*table.args(), mismatch=mismatch)
    _same(got, want[mismatch])
    assert got["stats"]["kernel_ms"] > 0


def test_slice_through_a_nonzero_offset(ctx):
    t = ref.generate(seed=4, fragments=6000, rows=60)
    f0, f1 = 1500, 5200
    lp = t.list_ptr.astype(np.int64)
    sub = ref.Table(t.frag_row[f0:f1], t.frag_umi[f0:f1], lp[f0:f1 + 1] - lp[f0], t.list_allele[lp[f0]:lp[f1]], t.n_rows, t.allele_gene, t.n_genes)
    w = ref.restate(sub, 1)
    assert w.stats["corrected"] > 0 and w.stats["split"] > 0
    got = ctx.umi_collapse(t.frag_row[f0:f1], t.frag_umi[f0:f1], t.list_ptr[f0:f1 + 1], t.list_allele, t.n_rows, t.allele_gene, t.n_genes)
    assert int(t.list_ptr[f0]) > 0
    _same(got, w)


# ---- the three run tables at their edges: one item, a block boundary, one long run, lone keys only -------------------------------------
def _edge_tables():
    """name -> (Table from the restatement's own builder, what the restatement must say of it for mismatch 1)"""
    one_gene, two_genes = np.zeros(2, np.uint32), np.array([0, 1], np.uint32)
    top = "T" * 16                                              # the largest code of the longest length: with the last row and gene, the largest real key
    # (both rows hold a pair at distance 1 that mismatch 1 joins: T..TG into T..TT by count, ACGT into ACGA by the smaller code)
    mix = [(1, top, [1]), (0, "ACGT", [0]), (1, None, [1]), (1, top, [1]), (0, "ACGA", [0, 1]), (1, None, [1]), (1, "T" * 15 + "G", [1]), (0, None, [0])]
    return {
        "one_umi": (ref.from_fragments([(0, "ACGT", [0])], 1, one_gene, 1), dict(distinct=1, keys=1, corrected=0, split=0, no_umi=0)),
        "one_none": (ref.from_fragments([(0, None, [0])], 1, one_gene, 1), dict(distinct=0, keys=0, corrected=0, split=0, no_umi=1)),
        "distinct_256": (ref.from_fragments([(i, "ACGT", [0]) for i in range(256)], 256, one_gene, 1), dict(distinct=256, keys=256, corrected=0, split=0, no_umi=0)),
        "distinct_257": (ref.from_fragments([(i, "ACGT", [0]) for i in range(257)], 257, one_gene, 1), dict(distinct=257, keys=257, corrected=0, split=0, no_umi=0)),
        "one_run_256": (ref.from_fragments([(0, "ACGT", [0])] * 256, 1, one_gene, 1), dict(distinct=1, keys=1, corrected=0, split=0, no_umi=0)),
        "none_300": (ref.from_fragments([(0, None, [0, 1])] * 300, 1, one_gene, 1), dict(distinct=0, keys=0, corrected=0, split=0, no_umi=300)),
        "none_behind_top_key": (ref.from_fragments(mix, 2, two_genes, 2), dict(distinct=4, keys=2, corrected=2, split=0, no_umi=3)),
    }


EDGES = _edge_tables()


@pytest.mark.parametrize("mismatch", [0, 1])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_run_table_edges_equal_restatement(ctx, name, mismatch):
    t, stats1 = EDGES[name]
    w = ref.restate(t, mismatch)
    if mismatch == 1:
        assert w.stats == stats1                                # the case is the one its name says
    if name == "none_behind_top_key":
        key = ((np.uint64(1 * 2 + 1) << np.uint64(4) | np.uint64(15)) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
        assert w.keys[-1] == key and w.counts[-1] == 2          # the run in front of the all-ones keys: real, low word all ones, two fragments
        assert w.frag_mol[0] == w.frag_mol[3] and len({int(w.frag_mol[f]) for f in (2, 5, 7)}) == 3
    if name == "none_300":
        assert len(w.mol_row) == 300 and w.frac[0].tolist() == [150.0, 150.0]
    if name == "one_run_256":
        assert w.mol_frags.tolist() == [256]
    _same(ctx.umi_collapse(*t.args(), mismatch=mismatch), w)


def test_argument_errors(ctx):
    gene = np.array([0, 0, 1, 1], np.uint32)
    good = ref.from_fragments([(0, "ACGT", [0, 1]), (1, "ACGA", [1]), (1, None, [2, 3])], 2, gene, 2)
    row, umi, ptr, al, n_rows, ag, ng = good.args()
    assert ctx.umi_collapse(row, umi, ptr, al, n_rows, ag, ng, raw=True) == 0

    def rc(**over):
        a = dict(frag_row=row, frag_umi=umi, list_ptr=ptr, list_allele=al, n_rows=n_rows, allele_gene=ag, n_genes=ng, mismatch=1)
        a.update(over)
        return ctx.umi_collapse(raw=True, **a)
    assert rc() == 0
    assert rc(list_allele=np.array([1, 0, 1, 2, 3], np.uint32)) < 0                 # list not ascending
    assert rc(list_allele=np.array([0, 0, 1, 2, 3], np.uint32)) < 0                 # ... not strictly
    assert rc(allele_gene=gene[:3]) < 0                                             # allele >= nAlleles
    assert rc(frag_row=np.array([0, 2, 1], np.uint32)) < 0                          # row >= nRows
    assert rc(list_ptr=np.array([0, 2, 1, 5], np.uint64)) < 0                       # offsets decrease
    assert rc(list_ptr=np.array([0, 2, 2, 5], np.uint64)) < 0                       # a fragment without a list
    assert rc(frag_umi=np.array([int(umi[0]), 0 << 32, int(umi[2])], np.uint64)) < 0            # UMI length 0
    assert rc(frag_umi=np.array([int(umi[0]), 17 << 32, int(umi[2])], np.uint64)) < 0           # UMI length 17
    assert rc(frag_umi=np.array([int(umi[0]), (2 << 32) | 0x10, int(umi[2])], np.uint64)) < 0   # a code beyond its length
    assert rc(allele_gene=np.array([0, 0, 1, 2], np.uint32)) < 0                    # gene >= nGenes
    assert rc(mismatch=2) < 0
    assert rc(n_genes=1 << 27) < 0                                                  # rows x genes beyond the key's 28 bits


# ---- the analyzer ------------------------------------------------------------------------------------------------------------------
class Chain:
    pass


@pytest.fixture(scope="module")
def chain(built, tmp_path_factory):
    """the genotyper on the golden case, once: its aligned reads are what every analyzer run below takes"""
    tmp = str(tmp_path_factory.mktemp("umi_chain"))
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    r = subprocess.run([GENO] + c.args() + ["-o", g], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    ch = Chain()
    ch.tmp, ch.case, ch.g = tmp, c, g
    ch.reads = [t1k_amd.read_fastx(g + s) for s in ("_aligned_1.fa", "_aligned_2.fa", "_aligned_bc.fa")]
    ch.names = [r[0] for r in ch.reads[0]]
    assert ch.names == [r[0] for r in ch.reads[2]] and len(ch.names) > 100
    ch.umis = ref.distinct_umis(len(ch.names), 12)
    ch.umi_file = os.path.join(tmp, "distinct_umi.fa")
    _write_fa(ch.umi_file, zip(ch.names, ch.umis))
    return ch


def _write_fa(path, recs):
    with open(path, "w") as f:
        for name, seq in recs:
            f.write(">%s\n%s\n" % (name, seq))


def _analyze(ch, out, extra, files=None, env=None, ok=True):
    a1, a2, bc = files or (ch.g + "_aligned_1.fa", ch.g + "_aligned_2.fa", ch.g + "_aligned_bc.fa")
    cmd = [ANALYZER, "-f", ch.case.ref, "-a", ch.g + "_allele.tsv", "-1", a1, "-2", a2, "--barcode", bc, "-o", out] + ch.case.flags + extra
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _table(path):
    lines = open(path).read().split("\n")
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:] if l]


def _same_table(umi_path, expr_path):
    """header, row names and _uniq columns as text; the %lf columns within 1e-6 (six decimals printed on both sides, the sums taken in
    different orders: half a unit each way)"""
    uh, ur = _table(umi_path)
    xh, xr = _table(expr_path)
    A = (len(xh) - 1) // 2
    assert uh == xh and len(ur) == len(xr) > 0
    for u, x in zip(ur, xr):
        assert u[0] == x[0] and u[A + 1:] == x[A + 1:] and len(u) == len(x)
        micro = [[int(v.replace(".", "")) for v in row[1:A + 1]] for row in (u, x)]   # six decimals: the text in units of 1e-6, exactly
        assert all("." in v and len(v.split(".")[1]) == 6 for v in u[1:A + 1] + x[1:A + 1])
        assert np.abs(np.array(micro[0]) - np.array(micro[1])).max() <= 1
    return sum(float(v) for x in xr for v in x[1:A + 1])


@pytest.mark.parametrize("both,umi_only", [([], []), ([], ["--umiMismatch", "0"]), (["--varMaxGroup", "0"], [])])
def test_analyzer_distinct_umis_give_the_fragment_table(chain, tmp_path, both, umi_only):
    plain, flag = os.path.join(str(tmp_path), "plain"), os.path.join(str(tmp_path), "flag")
    _analyze(chain, plain, both)
    assert glob.glob(plain + "_barcode_umi*") == []
    r = _analyze(chain, flag, both + umi_only + ["--umi", chain.umi_file], env={"T1K_DEBUG_PHASES": "1"})
    assert [l for l in r.stderr.split("\n") if l.startswith("umi:")] and " 0 corrected UMIs" in r.stderr
    assert open(flag + "_barcode_expr.tsv").read() == open(plain + "_barcode_expr.tsv").read()
    assert open(flag + "_allele.vcf").read() == open(plain + "_allele.vcf").read()
    assert _same_table(flag + "_barcode_umi.tsv", plain + "_barcode_expr.tsv") > 100
    assert not os.path.exists(flag + "_barcode_umi_em.tsv") and not os.path.exists(flag + "_barcode_em.tsv")


def test_analyzer_tripled_reads_collapse_to_the_fragment_table(chain, tmp_path):
    """every record three times under new names, one UMI per original fragment; raw rows (--varMaxGroup 0), so that the copies cannot
    move a variant call"""
    tmp = str(tmp_path)
    files = []
    for recs, s in zip(chain.reads, ("t_1.fa", "t_2.fa", "t_bc.fa")):
        files.append(os.path.join(tmp, s))
        _write_fa(files[-1], [(r[0] + c, r[2]) for r in recs for c in ("", "_c1", "_c2")])
    umi = os.path.join(tmp, "t_umi.fa")
    _write_fa(umi, [(n + c, u) for n, u in zip(chain.names, chain.umis) for c in ("", "_c1", "_c2")])
    one, three = os.path.join(tmp, "one"), os.path.join(tmp, "three")
    _analyze(chain, one, ["--varMaxGroup", "0"])
    _analyze(chain, three, ["--varMaxGroup", "0", "--umi", umi], files=files)
    assert _same_table(three + "_barcode_umi.tsv", one + "_barcode_expr.tsv") > 100


def test_analyzer_umi_em_rows_sum_to_the_molecules(chain, tmp_path):
    # UMIs that do collapse: one per barcode and eight fragments
    per = {}
    umis = []
    for rec in chain.reads[2]:
        k = per[rec[2]] = per.get(rec[2], 0) + 1
        umis.append(chain.umis[k // 8])
    umi = os.path.join(str(tmp_path), "umi.fa")
    _write_fa(umi, zip(chain.names, umis))
    o = os.path.join(str(tmp_path), "o")
    r = _analyze(chain, o, ["--umi", umi, "--barcodeEM"], env={"T1K_DEBUG_PHASES": "1"})
    assert "barcode EM on molecules: groups built" in r.stderr and "barcode EM: groups built" in r.stderr
    uh, ur = _table(o + "_barcode_umi.tsv")
    eh, er = _table(o + "_barcode_umi_em.tsv")
    xh, xr = _table(o + "_barcode_expr.tsv")
    A = (len(uh) - 1) // 2
    assert eh == uh[:A + 1] and len(er) == len(ur) == len(xr) > 0 and os.path.exists(o + "_barcode_em.tsv")
    fewer = 0
    for e, u, x in zip(er, ur, xr):
        assert e[0] == u[0] == x[0] and len(e) == A + 1
        mol, frag = sum(float(v) for v in u[1:A + 1]), sum(float(v) for v in x[1:A + 1])
        assert abs(sum(float(v) for v in e[1:]) - mol) <= 1e-5
        assert mol <= frag + 1e-5
        fewer += mol < frag - 0.5
    assert fewer >= 1


def test_analyzer_umi_file_is_a_superset_in_order(chain, tmp_path):
    tmp = str(tmp_path)
    exact, more, less = (os.path.join(tmp, x) for x in ("exact", "more", "less"))
    _analyze(chain, exact, ["--umi", chain.umi_file])
    recs = []
    for i, (n, u) in enumerate(zip(chain.names, chain.umis)):
        if i % 3 == 0:
            recs.append(("not_aligned_%d" % i, "ACGTNACGTACG" if i % 2 else "missing_barcode"))
        recs.append((n, u))
    recs.append(("not_aligned_last", "ACGTACGTACGT"))
    _write_fa(more + ".fa", recs)
    _analyze(chain, more, ["--umi", more + ".fa"])
    assert open(more + "_barcode_umi.tsv").read() == open(exact + "_barcode_umi.tsv").read()
    # a file without the records of one counted barcode (the one with the fewest reads among the rows that count anything)
    xh, xr = _table(exact + "_barcode_expr.tsv")
    counted = {x[0] for x in xr if any(float(v) > 0 for v in x[1:])}
    size = {}
    for rec in chain.reads[2]:
        size[rec[2]] = size.get(rec[2], 0) + 1
    drop = min(counted, key=lambda b: (size[b], b))
    gone = {rec[0] for rec in chain.reads[2] if rec[2] == drop}
    _write_fa(less + ".fa", [(n, u) for n, u in zip(chain.names, chain.umis) if n not in gone])
    r = _analyze(chain, less, ["--umi", less + ".fa"], ok=False)
    assert r.returncode == 1 and any(n in r.stderr for n in gone), r.stderr
    assert glob.glob(less + "_barcode_umi*") == []
