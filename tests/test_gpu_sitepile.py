"""GPU tests of the per-barcode pileup at sites (t1k_sitepile_*, analyzer --barcodePileup): the kernel and the fold against the
sequential restatement, every cell and counter exactly; the argument errors, none of which may emit anything; the analyzer's file
against the restatement fed with the CPU oracle's alignments, line for line; its sum over barcodes against --pileup; every other output
unchanged; the golden chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import pileup_ref
import sitepile_ref as ref
import util
import t1k_amd
from test_variants_host import oracle_dump, parse_dump

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -3, -5


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=30000)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(table.allele_off, table.aln, table.book_ptr, table.book, table.text, table.ops, table.site_allele, table.site_pos)


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _kernel(ctx, t, cuts=()):
    keys, counts, ms, folds = ctx.sitepile(t.allele_off, t.site_allele, t.site_pos, t.n_barcodes, t.aln, t.book_ptr, t.book, t.text, t.ops, cuts=cuts)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (counts > 0).all()         # runs ascending by key, one per key
    return ref.from_runs(keys, counts, len(t.site_allele)), ms, folds


# ---- 1. kernel = restatement ---------------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement(ctx, table, want):
    got, ms, folds = _kernel(ctx, table)
    assert len(want) > 50000 and ref.same(got, want)
    assert ms > 0 and folds == 1


def test_three_calls_give_the_same_table(ctx, table, want):
    got, _, _ = _kernel(ctx, table, cuts=(7001, 19000))
    assert ref.same(got, want)


def test_several_folds_give_the_same_table(ctx, table, want, monkeypatch):
    monkeypatch.setenv("T1K_SITEPILE_PENDING", "1000")        # every one of the six calls emits more: a fold behind each
    got, _, folds = _kernel(ctx, table, cuts=(5000, 10000, 15000, 20000, 25000))
    assert folds >= 3 and ref.same(got, want)


def test_no_sites_gives_no_runs(ctx, table):
    none = np.zeros(0, np.uint32)
    keys, counts, _, folds = ctx.sitepile(table.allele_off, none, none, table.n_barcodes, table.aln, table.book_ptr, table.book, table.text, table.ops)
    assert len(keys) == 0 and len(counts) == 0 and folds == 0


# ---- the fold's run table and count differences at their edges -------------------------------------------------------------------------
def _edge(books):
    """one allele of 8 bases with a site at position 3; a record of five matches from position 0 per booking list (it hits the site once)"""
    off = pileup_ref.offsets([8])
    aln = np.array([(0, 0, 0, 0, 5, 0, 0, 0)] * len(books), t1k_amd.PILEUP_ALN_DTYPE)
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in books])]).astype(np.uint64)
    book = np.array([e for b in books for e in b], np.uint32)
    return (off, np.array([0], np.uint32), np.array([3], np.uint32), 3, aln, ptr, book, b"ACGTACGT", np.zeros(5, np.int8))


def _edge_want(args):
    off, sa, sp, _, aln, ptr, book, text, ops = args
    return ref.restate(off, aln, ptr, book, text, ops, sa, sp)


def test_fold_of_one_key(ctx):
    args = _edge([[(2 << 1) | 1]])
    keys, counts, _, folds = ctx.sitepile(*args)
    assert len(keys) == 1 and counts.tolist() == [1] and folds == 1
    assert ref.same(ref.from_runs(keys, counts, 1), _edge_want(args))


def test_fold_of_one_run_of_256(ctx):
    args = _edge([[(1 << 1) | 0] * 256])
    keys, counts, _, folds = ctx.sitepile(*args)
    assert len(keys) == 1 and counts.tolist() == [256] and folds == 1
    assert ref.same(ref.from_runs(keys, counts, 1), _edge_want(args))


def test_fold_merges_a_folded_count_with_pending_keys(ctx, monkeypatch):
    monkeypatch.setenv("T1K_SITEPILE_PENDING", "1")           # a fold behind each of the two calls
    args = _edge([[(1 << 1) | 0] * 256, [(1 << 1) | 0] * 256 + [(2 << 1) | 0]])
    keys, counts, _, folds = ctx.sitepile(*args, cuts=(1,))
    assert counts.tolist() == [512, 1] and folds == 2         # (count 256 + 256 pending keys) in one run, then a run of one
    assert ref.same(ref.from_runs(keys, counts, 1), _edge_want(args))


def test_a_second_session_holds_no_more_device_memory(ctx):
    """_end frees every block of the stage: what the context holds behind one begin / add / get / end (its scan and sort scratch stays, by
    design) is what it holds behind the next"""
    args = _edge([[(2 << 1) | 1]])
    ctx.sitepile(*args)
    held = ctx.mem_bytes()
    ctx.sitepile(*args)
    assert ctx.mem_bytes() == held


# ---- 2. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_emit_nothing(built):
    c = t1k_amd.Context()
    try:
        off = pileup_ref.offsets([8, 5])
        sa, sp = np.array([0, 0, 1, 1], np.uint32), np.array([1, 7, 0, 4], np.uint32)
        text = b"ACGTACGTAC"
        ops = np.array([0, 0, 1, 0, 0, 4, 0, 0], np.int8)

        def rec(allele=0, seq_start=0, read_at=0, ops_at=0, n_ops=5):
            return np.array([(allele, seq_start, read_at, ops_at, n_ops, 0, 0, 0)], t1k_amd.PILEUP_ALN_DTYPE)

        def table():
            return ref.from_runs(*c.sitepile_get(), len(sa))
        one = (np.array([0, 1], np.uint64), np.array([(2 << 1) | 1], np.uint32))
        assert c.sitepile_add(rec(), one[0], one[1], text, ops, raw=True) == ERR_STATE and c.last_error().startswith("t1k_sitepile_add: ")   # add / get / end before begin
        assert c.sitepile_get(raw=True) == ERR_STATE and c.sitepile_end(raw=True) == ERR_STATE
        # sites: unsorted, duplicate, behind their allele, on an unknown allele; a key space that is too large
        for bad_a, bad_p in (([0, 0], [7, 1]), ([1, 0], [0, 1]), ([0, 0], [3, 3]), ([0], [8]), ([2], [0])):
            assert c.sitepile_begin(off, np.array(bad_a, np.uint32), np.array(bad_p, np.uint32), 3, raw=True) == ERR_ARG
        assert c.sitepile_begin(off, sa, sp, (1 << 31) + 1, raw=True) == ERR_CAPACITY
        assert c.sitepile_begin(off, sa, sp, 1 << 62, raw=True) == ERR_CAPACITY
        assert c.sitepile_get(raw=True) == ERR_STATE                                          # none of them opened a table
        c.sitepile_begin(off, sa, sp, 3)
        assert table() == {}
        assert c.sitepile_begin(off, sa, sp, 3, raw=True) == ERR_STATE                        # a table is open
        good = np.concatenate([rec(), rec(allele=1, seq_start=0, read_at=5, n_ops=5)])
        gp, gb = np.array([0, 2, 3], np.uint64), np.array([(2 << 1) | 1, 0 << 1, (1 << 1) | 0], np.uint32)
        assert c.sitepile_add(good, gp, gb, text, ops, raw=True) == 0
        before = table()
        assert ref.same(before, ref.restate(off, good, gp, gb, text, ops, sa, sp)) and sum(int(v[:7].sum()) for v in before.values()) == 4

        def refused(bad, ptr=(3, 4), book=(1 << 1,), code=ERR_ARG):
            p = np.concatenate([gp, np.array(ptr[1:], np.uint64)])
            b = np.concatenate([gb, np.array(book, np.uint32)])
            assert c.sitepile_add(np.concatenate([good, bad]), p, b, text, ops, raw=True) == code    # the sound records of the call emit nothing either
            assert c.last_error().startswith("t1k_sitepile_add: ")                                    # whoever refused it, host or device
            assert ref.same(table(), before)
        refused(rec(ops_at=3, n_ops=5))                   # op value 4
        refused(rec(allele=1, seq_start=1, n_ops=5))      # a walk one base past the allele (5 bases from position 1 of 5)
        refused(rec(seq_start=4, n_ops=5))                # ... of the first allele (the site bitmap continues into the second's)
        refused(rec(read_at=6, n_ops=5))                  # a walk past `text`
        refused(rec(allele=2))                            # an allele id equal to nAlleles
        refused(rec(ops_at=4, n_ops=5))                   # an edit string that leaves `ops`
        refused(rec(), book=(3 << 1,))                    # a barcode id equal to nBarcodes
        refused(rec(), ptr=(3, 2))                        # bookPtr decreases
        refused(rec(ops_at=3, n_ops=5), ptr=(3, 3), book=())   # a bad record is refused even when it has no booking
        more = (rec(allele=1, seq_start=0, read_at=5), np.array([0, 2], np.uint64), np.array([(1 << 1) | 1, (1 << 1) | 1], np.uint32))
        assert c.sitepile_add(*more, text, ops, raw=True) == 0                                # and the table still takes sound calls
        both = ref.restate(off, np.concatenate([good, more[0]]), np.array([0, 2, 3, 5], np.uint64), np.concatenate([gb, more[2]]), text, ops, sa, sp)
        assert ref.same(table(), both) and both[(1, 2)][7:].sum() == 2
        c.sitepile_end()
        assert c.sitepile_add(rec(), one[0], one[1], text, ops, raw=True) == ERR_STATE
    finally:
        c.close()


# ---- the analyzer --------------------------------------------------------------------------------------------------------------------
def _run(cmd, env=None, ok=True):
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def _genotype(tmp, ref_fa, pfx, single=False):
    g = os.path.join(tmp, "g")
    reads = ["-u", pfx + "_1.fq"] if single else ["-1", pfx + "_1.fq", "-2", pfx + "_2.fq"]
    _run([GENO, "-f", ref_fa] + reads + ["--barcode", pfx + "_bc.fa", "-o", g])
    return g, (["-u", g + "_aligned.fa"] if single else ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"])


def _analyze(ref_fa, g, aligned, out, extra=(), env=None, ok=True):
    return _run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv"] + aligned + ["--barcode", g + "_aligned_bc.fa", "-o", out, "-t", "4"] + list(extra), env, ok)


def _read(path):
    return open(path, "rb").read()


def _vcf(path):
    """rows of _allele.vcf: (allele name, 0-based ref_pos, ref base, var base)"""
    return [(v[0], int(v[-2]), v[3], v[4]) for v in (l.split(" ") for l in open(path).read().split("\n") if l)]


def _sum_over_barcodes_is_the_pileup(bp_path, pile_path, sites):
    """for every site (allele name, 1-based pos): the 14 column sums over the barcode lines = the line of _allele_pileup.tsv"""
    header, rows = ref.parse(bp_path)
    assert header == ref.HEADER
    _, pile = pileup_ref.parse(pile_path)
    line = {(r[0], r[1]): r for r in pile}
    total = {}
    for r in rows:
        assert (r[1], r[2]) in sites, r[:3]
        assert sum(r[6][k] for k in ref.COUNTERS[:7]) > 0 and all(r[6][k + "_uniq"] <= r[6][k] for k in ref.COUNTERS[:7])
        assert r[3] == line[(r[1], r[2])][2] and r[4] == line[(r[1], r[2])][3]                 # exon_pos and ref as in _allele_pileup.tsv
        t = total.setdefault((r[1], r[2]), dict.fromkeys(ref.COUNTERS, 0))
        for k in ref.COUNTERS:
            t[k] += r[6][k]
    for s in sites:
        assert total.get(s, dict.fromkeys(ref.COUNTERS, 0)) == line[s][4], s
    return rows


# ---- 3. analyzer = restatement on the CPU oracle's alignments ------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True])
def test_analyzer_equals_restatement_on_the_oracles_alignments(built, tmp_path, single):
    tmp = str(tmp_path)
    ref_fa, pfx = util.several_snps_sample(tmp, 29, genes=3, pairs=2500) if single else util.several_snps_sample(tmp, 3)
    g, aligned = _genotype(tmp, ref_fa, pfx, single)
    sel, out, names, _ = oracle_dump(tmp, ref_fa, g, aligned)
    ref_names, seqs, masks, _ = t1k_amd.load_reference_fasta(sel)
    assert ref_names == names
    r1 = [s for _, _, s in t1k_amd.read_fastx(aligned[1])]
    r2 = None if single else [s for _, _, s in t1k_amd.read_fastx(aligned[3])]
    ptr, asg, ops = parse_dump(out + "_fragdump.tsv", len(r1))
    assert len(asg) > 1000 and (np.diff(ptr.astype(np.int64)) > 1).any()
    lens = [len(s) for s in seqs]
    off = pileup_ref.offsets(lens).astype(np.int64)
    depth = pileup_ref.restate(ptr, asg, ops, r1, r2, lens)[:7].sum(axis=0)
    # about 40 sites of the file: both ends and evenly spaced positions of every selected allele, up to six positions no alignment touches
    # (they get no line), a name that is not selected, one that does not exist, comments, a blank line and a duplicate
    other = next(n for n, _, _ in util.read_fa(ref_fa) if n not in names)
    lines, file_sites = ["# allele\tpos", ""], set()
    empty = np.nonzero(depth == 0)[0]
    for g0 in empty[np.linspace(0, len(empty) - 1, min(6, len(empty))).astype(np.int64)] if len(empty) else []:
        a0 = int(np.searchsorted(off, g0, side="right")) - 1
        file_sites.add((a0, int(g0 - off[a0])))
    n_empty = len(file_sites)
    print("%d positions without an alignment, %d of them in the sites file" % (len(empty), n_empty))
    per = max(2, round(40 / len(seqs)))                                                    # about 40 in all, whatever the number of selected alleles
    for a, s in enumerate(seqs):
        file_sites |= {(a, (len(s) - 1) * k // (per - 1)) for k in range(per)}
    lines += ["%s\t%d" % (names[a], p + 1) for a, p in sorted(file_sites, key=lambda x: (x[1], x[0]))]     # in no particular order
    lines[5:5] = ["%s\t3" % other, "#" + names[0] + "\t1", "NOT*AN:ALLELE\t100000"]
    lines.append(lines[3])                                                                 # a duplicate
    sites_file = os.path.join(tmp, "sites.tsv")
    open(sites_file, "w").write("\n".join(lines) + "\n")
    assert 30 <= len(file_sites) <= 70
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--barcodePileup", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"})
    assert [l for l in r.stderr.split("\n") if l.startswith("barcode pileup: ") and "keys emitted" in l and "folds" in l], r.stderr[-2000:]
    assert [l for l in r.stderr.split("\n") if l.startswith("--sites: ") and " 2 lines name an allele that is not selected" in l], r.stderr[-2000:]
    bc_names, bc_of = ref.barcode_ids([s for _, _, s in t1k_amd.read_fastx(g + "_aligned_bc.fa")])
    assert len(bc_of) == len(r1) and len(bc_names) > 1
    var_of, idx = {}, {n: i for i, n in enumerate(names)}
    for name, pos, _, var in _vcf(a + "_allele.vcf"):
        var_of[(idx[name], pos)] = var_of[(idx[name], pos)] + "," + var if (idx[name], pos) in var_of else var
    assert len(var_of) >= 1
    sites = sorted(file_sites | set(var_of))
    sa, sp = np.array([s[0] for s in sites], np.uint32), np.array([s[1] for s in sites], np.uint32)
    aln, text, book_ptr, book = ref.analyzer_records(ptr, asg, r1, r2, bc_of)
    cells = ref.restate(off, aln, book_ptr, book, text, ops, sa, sp)
    assert any(c[7:].sum() > 0 for c in cells.values()) and any((c[7:] < c[:7]).any() for c in cells.values())
    assert len(set(range(len(sites))) - {s for _, s in cells}) >= n_empty                  # a site without a read has no line
    want = ref.table_text(bc_names, names, seqs, masks, sa, sp, var_of, cells).split("\n")
    got = open(a + "_barcode_pileup.tsv").read().split("\n")
    assert len(got) == len(want) > 100
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    # the variant pass in several pieces, and with every alignment through the device: the same bytes
    for tag, env in (("piece", {"T1K_ANALYZER_PIECE": "600"}), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"})):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--barcodePileup", "--sites", sites_file], env=env)
        assert _read(o + "_barcode_pileup.tsv") == _read(a + "_barcode_pileup.tsv"), tag


# ---- 4. + 5. the sum over barcodes is the pileup; nothing else changes ---------------------------------------------------------------
class Runs:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["homo", "het"])
def snp(request, built, tmp_path_factory):
    """the novel-SNP sample through this build's genotyper, then the analyzer five ways"""
    tmp = str(tmp_path_factory.mktemp("sitepile_snp"))
    s = Runs()
    s.tmp, s.het = tmp, request.param
    s.ref, pfx = util.novel_snp_sample(tmp, s.het)
    s.g, s.aligned = _genotype(tmp, s.ref, pfx)
    s.plain, s.pile, s.both, s.flag, s.flag0 = (os.path.join(tmp, x) for x in ("plain", "pile", "both", "flag", "flag0"))
    _analyze(s.ref, s.g, s.aligned, s.plain)
    _analyze(s.ref, s.g, s.aligned, s.pile, ["--pileup"])
    _analyze(s.ref, s.g, s.aligned, s.both, ["--pileup", "--barcodePileup"])
    _analyze(s.ref, s.g, s.aligned, s.flag, ["--barcodePileup"])
    _analyze(s.ref, s.g, s.aligned, s.flag0, ["--varMaxGroup", "0", "--barcodePileup"])
    s.gold = os.path.join(util.GOLDEN, "analyzer_variants", "het" if s.het else "homo")
    return s


def test_sum_over_barcodes_is_the_pileup(snp):
    vcf = _vcf(snp.both + "_allele.vcf")
    assert len(vcf) >= 1
    rows = _sum_over_barcodes_is_the_pileup(snp.both + "_barcode_pileup.tsv", snp.both + "_allele_pileup.tsv", {(v[0], v[1] + 1) for v in vcf})
    for name, pos, ref_base, var in vcf:
        at = [r for r in rows if (r[1], r[2]) == (name, pos + 1)]
        assert len({r[0] for r in at}) >= 2                                    # at least two barcodes have a line at the called site
        assert all(var in r[5].split(",") and r[4] == ref_base for r in at)
        n_var, n_ref = sum(r[6][var] for r in at), sum(r[6][ref_base] for r in at)
        assert n_var > 0
        if not snp.het:
            assert n_var > n_ref
    assert _read(snp.flag + "_barcode_pileup.tsv") == _read(snp.both + "_barcode_pileup.tsv")      # with or without --pileup beside it


def test_nothing_else_changes(snp):
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(snp.flag + tail) == _read(snp.both + tail) == _read(snp.gold + tail) == _read(snp.plain + tail), tail
    assert _read(snp.both + "_allele_pileup.tsv") == _read(snp.pile + "_allele_pileup.tsv")
    assert not os.path.exists(snp.plain + "_barcode_pileup.tsv") and not os.path.exists(snp.pile + "_barcode_pileup.tsv")
    assert sorted(os.path.basename(p) for p in glob.glob(snp.flag + "_*")) == ["flag_allele.vcf", "flag_barcode_expr.tsv", "flag_barcode_pileup.tsv"]
    # no variant calling and no --sites: no site, the header alone
    assert _read(snp.flag0 + "_barcode_pileup.tsv").decode() == ref.HEADER + "\n" and _read(snp.flag0 + "_allele.vcf") == b""


def test_sites_without_variant_calling_and_a_bad_sites_line(snp):
    length = {n: len(sq) for n, _, sq in util.read_fa(snp.ref)}
    name, pos, _, _ = _vcf(snp.both + "_allele.vcf")[0]
    f = os.path.join(snp.tmp, "one_site.tsv")
    open(f, "w").write("%s\t%d\n" % (name, pos + 1))
    o = os.path.join(snp.tmp, "sites0")
    _analyze(snp.ref, snp.g, snp.aligned, o, ["--varMaxGroup", "0", "--barcodePileup", "--sites", f])
    _, rows = ref.parse(o + "_barcode_pileup.tsv")
    _, called = ref.parse(snp.both + "_barcode_pileup.tsv")
    assert _read(o + "_allele.vcf") == b"" and len(rows) >= 2
    # the alignments are made although no variant is called: the same counters, the var column empty
    assert [r[:5] + (r[6],) for r in rows] == [r[:5] + (r[6],) for r in called if (r[1], r[2]) == (name, pos + 1)] and all(r[5] == "." for r in rows)
    bad = os.path.join(snp.tmp, "bad_sites.tsv")
    open(bad, "w").write("# sites\n%s\t1\n%s\t%d\n" % (name, name, length[name] + 1))
    o = os.path.join(snp.tmp, "refused")
    r = _analyze(snp.ref, snp.g, snp.aligned, o, ["--barcodePileup", "--sites", bad], ok=False)
    assert bad in r.stderr and "line 3" in r.stderr and not glob.glob(o + "_*")
    open(bad, "w").write("%s\t1\n%s 12\n" % (name, name))                                  # a malformed line: no tab
    r = _analyze(snp.ref, snp.g, snp.aligned, o, ["--barcodePileup", "--sites", bad], ok=False)
    assert bad in r.stderr and "line 2" in r.stderr and not glob.glob(o + "_*")


# ---- 6. the golden chain -------------------------------------------------------------------------------------------------------------
def test_golden_chain(built, tmp_path):
    tmp = str(tmp_path)
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    _run([GENO] + c.args() + ["-o", g])
    aligned = ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"]
    selected = [l.split()[0] for l in open(g + "_allele.tsv") if l.strip()]
    seq = {name: s for name, _, s in util.read_fa(c.ref)}
    assert len(selected) >= 4
    sites_file = os.path.join(tmp, "sites.tsv")
    file_sites = [(a, p) for a in selected for p in range(50, len(seq[a]) + 1, 50)]          # every 50th position, 1-based
    open(sites_file, "w").write("".join("%s\t%d\n" % s for s in file_sites))
    flag = os.path.join(tmp, "flag")
    r = _analyze(c.ref, g, aligned, flag, c.flags + ["--pileup", "--barcodePileup", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"})
    print("\n".join(l for l in r.stderr.split("\n") if l.startswith("barcode pileup: ")))
    sites = set(file_sites) | {(v[0], v[1] + 1) for v in _vcf(flag + "_allele.vcf")}
    rows = _sum_over_barcodes_is_the_pileup(flag + "_barcode_pileup.tsv", flag + "_allele_pileup.tsv", sites)
    assert len(rows) > 100 and len({r[0] for r in rows}) >= 2
    # line order: the barcodes of _barcode_expr.tsv, then the alleles in the order of _allele_pileup.tsv, then pos
    bc_rank = {l.split("\t")[0]: i for i, l in enumerate(open(flag + "_barcode_expr.tsv").read().split("\n")[1:-1])}
    al_rank = {}
    for row in pileup_ref.parse(flag + "_allele_pileup.tsv")[1]:
        al_rank.setdefault(row[0], len(al_rank))
    order = [(bc_rank[r[0]], al_rank[r[1]], r[2]) for r in rows]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
