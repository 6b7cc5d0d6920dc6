"""GPU tests of the per-base pileup (t1k_pileup_*, analyzer --pileup): the kernel against the sequential restatement, every
counter exactly; the argument errors, none of which may book anything; the analyzer's table against the restatement fed with the CPU
oracle's alignments, line for line; every other output unchanged; the table joined to the VCF; the golden chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import pileup_ref as ref
import util
import t1k_amd
from test_variants_host import oracle_dump, parse_dump

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
BASES = ("A", "C", "G", "T", "N")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=30000)


@pytest.fixture(scope="module")
def want(table):
    w = ref.book(table.allele_off, table.aln, table.text, table.ops)
    w.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


# ---- 1. kernel = restatement ---------------------------------------------------------------------------------------------------------
def test_table_covers_the_cases(table, want):
    a = table.aln
    n = a["n_ops"]
    assert len(a) == 30000 and table.allele_len == [1, 63, 64, 65, 1000, 4097]
    assert all((n == k).sum() > 100 for k in (1, 63, 64, 65, 128)) and n.max() >= 295 and ((n > 128) & (n < 300)).sum() > 1000
    assert set(np.unique(a["w_all"])) == set(range(6)) and (a["w_uniq"] <= a["w_all"]).all() and (a["w_uniq"] < a["w_all"]).any()
    assert all(table.kinds.get(k, 0) > 100 for k in range(8))            # gaps at the first / last column, across the seams, all-insert
    first, last = table.ops[a["ops_at"].astype(np.int64)], table.ops[(a["ops_at"] + n - 1).astype(np.int64)]
    assert all(((first == op).sum() > 100 and (last == op).sum() > 100) for op in (2, 3))
    alen = np.array(table.allele_len)[a["allele"]]
    assert set(np.unique(a["allele"])) == set(range(6)) and (a["seq_start"] == 0).sum() > 100 and (a["seq_start"] == alen).sum() >= 1
    off = table.allele_off.astype(np.int64)
    assert all(want[:7, off[i]].sum() > 0 and want[:7, off[i + 1] - 1].sum() > 0 for i in range(6))      # position 0 and the last one of every allele
    big, (lo, hi) = table.region
    inside = (a["allele"] == big) & (a["seq_start"] >= lo) & (a["seq_start"] < hi)
    assert inside.mean() >= 0.68 and want[:7, off[big] + lo:off[big] + hi].sum() >= 0.6 * want[:7].sum()   # contention
    assert want[ref.N].sum() > 1000 and want[ref.INS].sum() > 1000 and want[ref.DEL].sum() > 1000 and (want[7:] <= want[:7]).all()


def test_kernel_equals_restatement(ctx, table, want):
    got, ms = ctx.pileup(table.allele_off, table.aln, table.text, table.ops)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert ms > 0


def test_three_calls_give_the_same_table(ctx, table, want):
    got, _ = ctx.pileup(table.allele_off, table.aln, table.text, table.ops, cuts=(7001, 19000))
    assert np.array_equal(got, want)


# ---- 2. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_book_nothing(built):
    c = t1k_amd.Context()
    try:
        off = ref.offsets([8, 5])
        text = b"ACGTACGTAC"
        ops = np.array([0, 0, 1, 0, 0, 4, 0, 0], np.int8)

        def rec(allele=0, seq_start=0, read_at=0, ops_at=0, n_ops=5, w_all=2, w_uniq=1):
            return np.array([(allele, seq_start, read_at, ops_at, n_ops, w_all, w_uniq, 0)], t1k_amd.PILEUP_ALN_DTYPE)
        assert c.pileup_add(rec(), text, ops, raw=True) < 0                      # add before begin
        assert c.pileup_end(raw=True) < 0
        c.pileup_begin(off)
        assert not c.pileup_get().any()
        assert c.pileup_begin(off, raw=True) < 0                                 # a table is open
        good = np.concatenate([rec(), rec(allele=1, seq_start=0, read_at=5, n_ops=5)])
        assert c.pileup_add(good, text, ops, raw=True) == 0
        before = c.pileup_get()
        assert np.array_equal(before, ref.book(off, good, text, ops)) and before.sum() == 30

        def refused(bad):
            assert c.pileup_add(np.concatenate([good, bad]), text, ops, raw=True) < 0     # the sound records of the call are not booked either
            assert np.array_equal(c.pileup_get(), before)
        refused(rec(ops_at=3, n_ops=5))                   # op value 4
        refused(rec(allele=1, seq_start=1, n_ops=5))      # a walk one base past the allele (5 bases from position 1 of 5)
        refused(rec(seq_start=4, n_ops=5))                # ... of the first allele (its table cells continue into the second's)
        refused(rec(read_at=6, n_ops=5))                  # a walk past `text`
        refused(rec(allele=2))                            # an allele id equal to nAlleles
        refused(rec(ops_at=4, n_ops=5))                   # an edit string that leaves `ops`
        refused(rec(w_all=1, w_uniq=2))
        assert c.pileup_add(rec(allele=1, seq_start=0, read_at=5), text, ops, raw=True) == 0        # and the table still takes sound calls
        assert np.array_equal(c.pileup_get(), before + ref.book(off, rec(allele=1, seq_start=0, read_at=5), text, ops))
        c.pileup_end()
        assert c.pileup_add(rec(), text, ops, raw=True) < 0
    finally:
        c.close()


# ---- the analyzer --------------------------------------------------------------------------------------------------------------------
def _run(cmd, env=None):
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _genotype(tmp, ref_fa, pfx, single=False):
    g = os.path.join(tmp, "g")
    reads = ["-u", pfx + "_1.fq"] if single else ["-1", pfx + "_1.fq", "-2", pfx + "_2.fq"]
    _run([GENO, "-f", ref_fa] + reads + ["--barcode", pfx + "_bc.fa", "-o", g])
    return g, (["-u", g + "_aligned.fa"] if single else ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"])


def _analyze(ref_fa, g, aligned, out, extra=(), env=None):
    return _run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv"] + aligned + ["--barcode", g + "_aligned_bc.fa", "-o", out, "-t", "4"] + list(extra), env)


# ---- 3. analyzer = restatement on the CPU oracle's alignments ------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True])
def test_analyzer_equals_restatement_on_the_oracles_alignments(built, tmp_path, single):
    tmp = str(tmp_path)
    ref_fa, pfx = util.several_snps_sample(tmp, 29, genes=3, pairs=2500) if single else util.several_snps_sample(tmp, 3)
    g, aligned = _genotype(tmp, ref_fa, pfx, single)
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--pileup"], env={"T1K_DEBUG_PHASES": "1"})
    assert [l for l in r.stderr.split("\n") if l.startswith("pileup: ") and "alignments walked" in l and "kernels" in l], r.stderr[-2000:]
    sel, out, names, _ = oracle_dump(tmp, ref_fa, g, aligned)
    r1 = [s for _, _, s in t1k_amd.read_fastx(aligned[1])]
    r2 = None if single else [s for _, _, s in t1k_amd.read_fastx(aligned[3])]
    ptr, asg, ops = parse_dump(out + "_fragdump.tsv", len(r1))
    assert len(asg) > 1000 and (np.diff(ptr.astype(np.int64)) > 1).any()
    ref_names, seqs, masks, _ = t1k_amd.load_reference_fasta(sel)
    assert ref_names == names
    counts = ref.restate(ptr, asg, ops, r1, r2, [len(s) for s in seqs])
    assert counts[7:].sum() > 0 and (counts[7:] < counts[:7]).any()
    want = ref.table_text(names, seqs, masks, counts).split("\n")
    got = open(a + "_allele_pileup.tsv").read().split("\n")
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    # the variant pass in several pieces, and with every alignment through the device: the same bytes
    for tag, env in (("piece", {"T1K_ANALYZER_PIECE": "600"}), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"})):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--pileup"], env=env)
        assert open(o + "_allele_pileup.tsv", "rb").read() == open(a + "_allele_pileup.tsv", "rb").read(), tag


# ---- 4. + 5. nothing else changes; the table joins the VCF ---------------------------------------------------------------------------
class Runs:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["homo", "het"])
def snp(request, built, tmp_path_factory):
    """the novel-SNP sample through this build's genotyper, then the analyzer four ways"""
    tmp = str(tmp_path_factory.mktemp("pileup_snp"))
    s = Runs()
    s.het = request.param
    s.ref, pfx = util.novel_snp_sample(tmp, s.het)
    g, aligned = _genotype(tmp, s.ref, pfx)
    s.plain, s.flag, s.plain0, s.flag0 = (os.path.join(tmp, x) for x in ("plain", "flag", "plain0", "flag0"))
    _analyze(s.ref, g, aligned, s.plain)
    _analyze(s.ref, g, aligned, s.flag, ["--pileup"])
    _analyze(s.ref, g, aligned, s.plain0, ["--varMaxGroup", "0"])
    _analyze(s.ref, g, aligned, s.flag0, ["--varMaxGroup", "0", "--pileup"])
    s.gold = os.path.join(util.GOLDEN, "analyzer_variants", "het" if s.het else "homo")
    return s


def _read(path):
    return open(path, "rb").read()


def test_nothing_else_changes(snp):
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(snp.flag + tail) == _read(snp.gold + tail) == _read(snp.plain + tail), tail
    assert not os.path.exists(snp.plain + "_allele_pileup.tsv") and not os.path.exists(snp.plain0 + "_allele_pileup.tsv")
    assert sorted(os.path.basename(p) for p in glob.glob(snp.flag + "_*")) == ["flag_allele.vcf", "flag_allele_pileup.tsv", "flag_barcode_expr.tsv"]
    # no variant calling: the empty VCF, the raw-list table, and the pileup of the default run
    assert _read(snp.flag0 + "_allele.vcf") == b"" and _read(snp.flag0 + "_barcode_expr.tsv") == _read(snp.plain0 + "_barcode_expr.tsv")
    assert _read(snp.flag0 + "_allele_pileup.tsv") == _read(snp.flag + "_allele_pileup.tsv")


def test_table_joins_the_vcf(snp):
    header, rows = ref.parse(snp.flag + "_allele_pileup.tsv")
    assert header == ref.HEADER
    at = {(r[0], r[1]): r for r in rows}
    vcf = [l.split(" ") for l in open(snp.flag + "_allele.vcf").read().split("\n") if l]
    assert len(vcf) >= 1
    for v in vcf:
        allele, exon_pos, ref_base, var, ref_pos = v[0], int(v[1]), v[3], v[4], int(v[-2])
        row = at[(allele, ref_pos + 1)]
        assert row[3] == ref_base and row[2] == exon_pos
        assert row[4][var] > 0
        if not snp.het:
            assert row[4][var] > row[4][ref_base]
    for r in rows:                                   # and on every line
        c = r[4]
        assert all(c[n + "_uniq"] <= c[n] for n in ref.COUNTERS[:7])
    assert sum(r[4]["A"] + r[4]["C"] + r[4]["G"] + r[4]["T"] for r in rows) > 100000


# ---- 6. the golden chain -------------------------------------------------------------------------------------------------------------
def test_golden_chain(built, tmp_path):
    tmp = str(tmp_path)
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    _run([GENO] + c.args() + ["-o", g])
    aligned = ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"]
    plain, flag = os.path.join(tmp, "plain"), os.path.join(tmp, "flag")
    _analyze(c.ref, g, aligned, plain, c.flags)
    _analyze(c.ref, g, aligned, flag, c.flags + ["--pileup"])
    header, rows = ref.parse(flag + "_allele_pileup.tsv")
    assert header == ref.HEADER
    selected = [l.split()[0] for l in open(g + "_allele.tsv") if l.strip()]
    seq = {name: s for name, _, s in util.read_fa(c.ref)}
    assert len(selected) >= 4
    want = [(a, p + 1, b) for a in selected for p, b in enumerate(seq[a])]       # one line per base of every selected allele, in order
    assert [(r[0], r[1], r[3]) for r in rows] == want
    depth = 0
    for r in rows:
        n = r[4]
        assert all(n[k + "_uniq"] <= n[k] for k in ref.COUNTERS[:7]) and all(v >= 0 for v in n.values())
        depth += sum(n[k] for k in BASES) + n["del"]
    cols = sum(len(s) for s in (x[2] for f in aligned[1::2] for x in t1k_amd.read_fastx(f)))
    assert 0 < depth and sum(r[4]["A_uniq"] + r[4]["C_uniq"] + r[4]["G_uniq"] + r[4]["T_uniq"] for r in rows) > 0
    assert depth >= 0.5 * cols                                                    # most read bases of the aligned reads are booked at least once
    outs = sorted(os.path.basename(p)[len("plain"):] for p in glob.glob(plain + "_*"))
    assert outs == ["_allele.vcf", "_barcode_expr.tsv"]
    for tail in outs:
        assert _read(flag + tail) == _read(plain + tail), tail
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
