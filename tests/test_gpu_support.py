"""GPU tests of the support table at sites (t1k_support_*, analyzer --siteSupport): the kernel and the fold against the
sequential restatement, every run of both key families exactly; the argument errors, none of which may emit anything; the analyzer's file
against the restatement fed with the CPU oracle's alignments, line for line; its counts against --pileup; every other output unchanged;
the golden chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import pileup_ref
import support_ref as ref
import util
import t1k_amd
from test_variants_host import oracle_dump, parse_dump

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -3, -5


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=6000)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(*ref.args(table))


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _kernel(ctx, t, cuts=()):
    keys, counts, ms, folds = ctx.support(t.allele_off, t.site_allele, t.site_pos, t.aln, t.rec, t.book_ptr, t.book, t.text, t.ops, cuts=cuts)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (counts > 0).all()         # runs ascending by key, one per key
    return keys, counts, ms, folds


def _same_runs(keys, counts, want, n_sites):
    """every run of both families: the keys and counts themselves, and through from_runs"""
    wk, wc = ref.expected_runs(want)
    return keys.tolist() == wk and counts.tolist() == wc and ref.same(ref.from_runs(keys, counts, n_sites), want)


# ---- 1. kernel = restatement ---------------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement(ctx, table, want):
    keys, counts, ms, folds = _kernel(ctx, table)
    assert len(want.a) > 10000 and len(want.b) > 10000 and _same_runs(keys, counts, want, len(table.site_allele))
    assert ms > 0 and folds == 1


def test_three_calls_give_the_same_table(ctx, table, want):
    keys, counts, _, _ = _kernel(ctx, table, cuts=(1401, 3800))
    assert _same_runs(keys, counts, want, len(table.site_allele))


def test_several_folds_give_the_same_table(ctx, table, want, monkeypatch):
    monkeypatch.setenv("T1K_SUPPORT_PENDING", "1000")          # every one of the six calls emits more: a fold behind each
    keys, counts, _, folds = _kernel(ctx, table, cuts=(1000, 2000, 3000, 4000, 5000))
    assert folds >= 3 and _same_runs(keys, counts, want, len(table.site_allele))


def test_no_sites_gives_no_runs(ctx, table):
    none = np.zeros(0, np.uint32)
    keys, counts, _, folds = ctx.support(table.allele_off, none, none, table.aln, table.rec, table.book_ptr, table.book, table.text, table.ops)
    assert len(keys) == 0 and len(counts) == 0 and folds == 0


# ---- the fold's run table and count differences at their edges -------------------------------------------------------------------------
def _edge(books):
    """one allele of 8 bases with a site at position 3; a record of five matches from position 0 per booking list (it hits the site once),
    the whole of a read-end of five bases"""
    off = pileup_ref.offsets([8])
    aln = np.array([(0, 0, 0, 0, 5, 0, 0, 0)] * len(books), t1k_amd.PILEUP_ALN_DTYPE)
    rec = np.array([(5, 0, 0)] * len(books), t1k_amd.SUPPORT_REC_DTYPE)
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in books])]).astype(np.uint64)
    book = np.array([e for b in books for e in b], t1k_amd.SUPPORT_BOOK_DTYPE)
    return (off, np.array([0], np.uint32), np.array([3], np.uint32), aln, rec, ptr, book, b"ACGTACGT", np.zeros(5, np.int8))


def _edge_want(args):
    off, sa, sp, aln, rec, ptr, book, text, ops = args
    return ref.restate(off, aln, rec, ptr, book, text, ops, sa, sp)


KEY_A = ((((0 * 7 + 3) * 2 + 0) * 2 + 0) * 512 + 1) * 2         # site 0, T, forward, file 1, d = min(3, 5 - 1 - 3) = 1; + 1: not uniq


def test_fold_of_one_key(ctx):
    args = _edge([[(1, 0, 4)]])
    keys, counts, _, folds = ctx.support(*args)
    assert keys.tolist() == [KEY_A, ref.FAMILY_B | ((3 * 2) << 24) | (3 << 12) | 1] and counts.tolist() == [1, 1] and folds == 1
    assert ref.same(ref.from_runs(keys, counts, 1), _edge_want(args))


def test_fold_of_one_run_of_256(ctx):
    args = _edge([[(0, 1, 7)] * 256])
    keys, counts, _, folds = ctx.support(*args)
    assert keys.tolist() == [KEY_A + 1, ref.FAMILY_B | ((3 * 2) << 24) | (2 << 12) | 4]          # family A: count 256; family B: one run
    assert counts.tolist() == [256, 256] and folds == 1
    want = _edge_want(args)
    assert ref.same(ref.from_runs(keys, counts, 1), want) and ref.lines(want) == {(0, 3): (256, 0, 256, 0, 256, 0, 1, 1, 256, 1)}


def test_fold_merges_a_folded_count_with_pending_keys(ctx, monkeypatch):
    monkeypatch.setenv("T1K_SUPPORT_PENDING", "1")             # a fold behind each of the two calls
    args = _edge([[(0, 1, 7)] * 256, [(0, 1, 7)] * 256 + [(2, 1, 7)]])
    keys, counts, _, folds = ctx.support(*args, cuts=(1,))
    assert counts.tolist() == [512, 1, 513] and folds == 2     # (count 256 + 256 pending keys) in one run, a run of one (file 2); one template
    assert ref.same(ref.from_runs(keys, counts, 1), _edge_want(args))


def test_a_second_session_holds_no_more_device_memory(ctx):
    """_end frees every block of the stage: what the context holds behind one begin / add / get / end (its scan and sort scratch stays, by
    design) is what it holds behind the next"""
    args = _edge([[(1, 0, 4)]])
    ctx.support(*args)
    held = ctx.mem_bytes()
    ctx.support(*args)
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

        def end(read_len=9, clip_front=2, strand=0):
            return np.array([(read_len, clip_front, strand)], t1k_amd.SUPPORT_REC_DTYPE)

        def books(*e):
            return np.array(list(e), t1k_amd.SUPPORT_BOOK_DTYPE).reshape(-1)

        def table():
            return ref.from_runs(*c.support_get(), len(sa))
        one = (np.array([0, 1], np.uint64), books((1, 0, 4)))
        assert c.support_add(rec(), end(), one[0], one[1], text, ops, raw=True) == ERR_STATE and c.last_error().startswith("t1k_support_add: ")   # add / get / end before begin
        assert c.support_get(raw=True) == ERR_STATE and c.support_end(raw=True) == ERR_STATE
        # sites: unsorted, duplicate, behind their allele, on an unknown allele; more than 2^28 of them
        for bad_a, bad_p in (([0, 0], [7, 1]), ([1, 0], [0, 1]), ([0, 0], [3, 3]), ([0], [8]), ([2], [0])):
            assert c.support_begin(off, np.array(bad_a, np.uint32), np.array(bad_p, np.uint32), raw=True) == ERR_ARG
        many = np.zeros((1 << 28) + 1, np.uint32)                                                # (never touched: the count alone is refused)
        assert c.support_begin(off, many, many, raw=True) == ERR_CAPACITY
        del many
        assert c.support_get(raw=True) == ERR_STATE                                              # none of them opened a table
        c.support_begin(off, sa, sp)
        assert table().a == {} and table().b == {}
        assert c.support_begin(off, sa, sp, raw=True) == ERR_STATE                               # a table is open
        good = np.concatenate([rec(), rec(allele=1, seq_start=0, read_at=5, n_ops=5)])
        ge = np.concatenate([end(), end(read_len=5, clip_front=0, strand=1)])
        gp, gb = np.array([0, 2, 3], np.uint64), books((1, 0, 7), (6, 0, 4), (2, 0, 4))
        assert c.support_add(good, ge, gp, gb, text, ops, raw=True) == 0
        before = table()
        assert ref.same(before, ref.restate(off, good, ge, gp, gb, text, ops, sa, sp)) and sum(v[0] for v in before.a.values()) == 4 == sum(before.b.values())

        def refused(bad, bad_end=None, ptr=(3, 4), book=((0, 0, 4),), code=ERR_ARG):
            p = np.concatenate([gp, np.array(ptr[1:], np.uint64)])
            b = np.concatenate([gb, books(*book)])
            e = np.concatenate([ge, end() if bad_end is None else bad_end])
            assert c.support_add(np.concatenate([good, bad]), e, p, b, text, ops, raw=True) == code    # the sound records of the call emit nothing either
            assert c.last_error().startswith("t1k_support_add: ")                                        # whoever refused it, host or device
            assert ref.same(table(), before)
        # what t1k_sitepile_add refuses
        refused(rec(ops_at=3, n_ops=5))                   # op value 4
        refused(rec(allele=1, seq_start=1, n_ops=5))      # a walk one base past the allele (5 bases from position 1 of 5)
        refused(rec(seq_start=4, n_ops=5))                # ... of the first allele (the site bitmap continues into the second's)
        refused(rec(read_at=6, n_ops=5))                  # a walk past `text`
        refused(rec(allele=2))                            # an allele id equal to nAlleles
        refused(rec(ops_at=4, n_ops=5))                   # an edit string that leaves `ops`
        refused(rec(), ptr=(3, 2))                        # bookPtr decreases
        refused(rec(ops_at=3, n_ops=5), ptr=(3, 3), book=())   # a bad record is refused even when it has no booking
        # the read-end
        refused(rec(), end(strand=2))                     # a strand other than 0 or 1
        refused(rec(), end(read_len=0, clip_front=0))     # no read-end
        refused(rec(), end(read_len=65536))               # ... and one too long
        refused(rec(), end(read_len=6, clip_front=2))     # the window leaves its read: 2 + 5 bases of 6
        refused(rec(), end(read_len=9, clip_front=5))     # ... by one: 5 + 5 of 9
        refused(rec(), end(read_len=9, clip_front=10))    # ... from its first base on
        refused(rec(), end(read_len=6, clip_front=2), ptr=(3, 3), book=())   # ... even without a booking
        # the bookings
        refused(rec(), book=((8, 0, 4),))                 # flags outside 0 .. 7
        refused(rec(), book=((0, 5, 4),))                 # a template that ends in front of its start
        refused(rec(), book=((0, 0, 8),))                 # ... that leaves its allele of 8 bases
        refused(rec(allele=1, read_at=5), book=((0, 0, 5),))   # ... of 5 bases
        more = (rec(allele=1, seq_start=0, read_at=5), end(read_len=5, clip_front=0), np.array([0, 2], np.uint64), books((3, 0, 4), (3, 1, 4)))
        assert c.support_add(*more, text, ops, raw=True) == 0                                    # and the table still takes sound calls
        both = ref.restate(off, np.concatenate([good, more[0]]), np.concatenate([ge, more[1]]), np.array([0, 2, 3, 5], np.uint64), np.concatenate([gb, more[3]]), text, ops, sa, sp)
        assert ref.same(table(), both) and sum(v[1] for v in both.a.values()) == 5 and len(both.b) > len(before.b)
        c.support_end()
        assert c.support_add(rec(), end(), one[0], one[1], text, ops, raw=True) == ERR_STATE
        assert c.support_get(raw=True) == ERR_STATE and c.support_end(raw=True) == ERR_STATE
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


def _analyze(ref_fa, g, aligned, out, extra=(), env=None, ok=True, barcode=True):
    return _run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv"] + aligned + (["--barcode", g + "_aligned_bc.fa"] if barcode else []) + ["-o", out, "-t", "4"] + list(extra), env, ok)


def _read(path):
    return open(path, "rb").read()


def _vcf(path):
    """rows of _allele.vcf: (allele name, 0-based ref_pos, ref base, var base)"""
    return [(v[0], int(v[-2]), v[3], v[4]) for v in (l.split(" ") for l in open(path).read().split("\n") if l)]


def _var_of(path, idx):
    var_of = {}
    for name, pos, _, var in _vcf(path):
        var_of[(idx[name], pos)] = var_of[(idx[name], pos)] + "," + var if (idx[name], pos) in var_of else var
    return var_of


PILE_COLUMN = dict(zip(ref.STATES, pileup_ref.COUNTERS[:7]))


def _counts_are_the_pileup(sup_path, pile_path, sites):
    """every line's count and count_uniq = the counter of its position and state in _allele_pileup.tsv, every non-zero counter at a site
    has a line, and the sums every line has to keep"""
    header, rows = ref.parse(sup_path)
    assert header == ref.HEADER
    line = {(r[0], r[1]): r for r in pileup_ref.parse(pile_path)[1]}
    seen = set()
    for r in rows:
        v, p = r[6], line[(r[0], r[1])]
        assert (r[0], r[1]) in sites, r[:2]
        assert r[2] == p[2] and r[3] == p[3]                                                    # exon_pos and ref as in _allele_pileup.tsv
        assert v["count"] == p[4][PILE_COLUMN[r[5]]] > 0 and v["count_uniq"] == p[4][PILE_COLUMN[r[5]] + "_uniq"], r
        assert v["fwd"] + v["rev"] == v["mate1"] + v["mate2"] == v["count"] and 1 <= v["templates"] <= v["count"], r
        assert 0 <= v["end_min"] <= v["end_med"] <= 511 and 0 <= v["near_end"] <= v["count"], r
        seen.add((r[0], r[1], r[5]))
    assert len(seen) == len(rows)
    assert seen == {(s[0], s[1], obs) for s in sites for obs, k in PILE_COLUMN.items() if line[s][4][k] > 0}
    return rows


# ---- 7. analyzer = restatement on the CPU oracle's alignments ------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
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
    # about 40 sites of the file: both ends and evenly spaced positions of every selected allele, a name that is not selected, one that does
    # not exist, comments, a blank line and a duplicate
    other = next(n for n, _, _ in util.read_fa(ref_fa) if n not in names)
    per = max(2, round(40 / len(seqs)))
    file_sites = {(a, (len(s) - 1) * k // (per - 1)) for a, s in enumerate(seqs) for k in range(per)}
    lines = ["# allele\tpos", ""] + ["%s\t%d" % (names[a], p + 1) for a, p in sorted(file_sites, key=lambda x: (x[1], x[0]))]     # in no particular order
    lines[5:5] = ["%s\t3" % other, "#" + names[0] + "\t1", "NOT*AN:ALLELE\t100000"]
    lines.append(lines[3])                                                                 # a duplicate
    sites_file = os.path.join(tmp, "sites.tsv")
    open(sites_file, "w").write("\n".join(lines) + "\n")
    assert 30 <= len(file_sites) <= 70
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--siteSupport", "--pileup", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"}, barcode=False)
    line = [l for l in r.stderr.split("\n") if l.startswith("site support: ")]
    assert len(line) == 1 and all(w in line[0] for w in (" sites", " records", " bookings", " keys emitted", " folds", " ms")), r.stderr[-2000:]
    print(line[0])
    assert [l for l in r.stderr.split("\n") if l.startswith("--sites: ") and " 2 lines name an allele that is not selected" in l], r.stderr[-2000:]
    var_of = _var_of(a + "_allele.vcf", {n: i for i, n in enumerate(names)})
    assert len(var_of) >= 1
    sites = sorted(file_sites | set(var_of))
    sa, sp = np.array([s[0] for s in sites], np.uint32), np.array([s[1] for s in sites], np.uint32)
    aln, text, rec, book_ptr, book = ref.analyzer_records(ptr, asg, r1, r2)
    assert set(np.unique(rec["strand"])) == {0, 1} and set(np.unique(book["flags"] & 1)) == {0, 1} and set(np.unique(book["flags"] >> 2)) == {0, 1}
    assert set(np.unique((book["flags"] >> 1) & 1)) == ({0} if single else {0, 1})
    table = ref.restate(off, aln, rec, book_ptr, book, text, ops, sa, sp)
    rows = ref.lines(table, end=10)
    assert any(v[9] < v[0] for v in rows.values()) and any(v[8] > 0 for v in rows.values()) and any(v[1] < v[0] for v in rows.values())
    want = ref.table_text(names, seqs, masks, sa, sp, var_of, rows).split("\n")
    got = open(a + "_allele_support.tsv").read().split("\n")
    assert len(got) == len(want) > 50                       # (the floor only keeps the comparison from being empty)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    if single:
        assert all(r[6]["mate2"] == 0 for r in ref.parse(a + "_allele_support.tsv")[1])
    _counts_are_the_pileup(a + "_allele_support.tsv", a + "_allele_pileup.tsv", {(names[x], p + 1) for x, p in sites})
    # the variant pass in several pieces, and with every alignment through the device: the same bytes
    for tag, env in (("piece", {"T1K_ANALYZER_PIECE": "600"}), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"})):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--siteSupport", "--sites", sites_file], env=env, barcode=False)
        assert _read(o + "_allele_support.tsv") == _read(a + "_allele_support.tsv"), tag
    # --supportEnd 3: near_end alone differs, and is the restatement's
    o = os.path.join(tmp, "end3")
    _analyze(ref_fa, g, aligned, o, ["--siteSupport", "--supportEnd", "3", "--sites", sites_file], barcode=False)
    got3 = open(o + "_allele_support.tsv").read().split("\n")
    assert got3 == ref.table_text(names, seqs, masks, sa, sp, var_of, ref.lines(table, end=3)).split("\n")
    cut = lambda l: l.split("\t")[:14] + l.split("\t")[15:]
    assert [cut(l) for l in got3] == [cut(l) for l in got] and got3 != got


# ---- 8. cross-checks; nothing else changes -------------------------------------------------------------------------------------------
class Runs:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["homo", "het"])
def snp(request, built, tmp_path_factory):
    """the novel-SNP sample through this build's genotyper, then the analyzer five ways"""
    tmp = str(tmp_path_factory.mktemp("support_snp"))
    s = Runs()
    s.tmp, s.het = tmp, request.param
    s.ref, pfx = util.novel_snp_sample(tmp, s.het)
    s.g, s.aligned = _genotype(tmp, s.ref, pfx)
    s.plain, s.pile, s.both, s.flag, s.flag0, s.nobc = (os.path.join(tmp, x) for x in ("plain", "pile", "both", "flag", "flag0", "nobc"))
    _analyze(s.ref, s.g, s.aligned, s.plain)
    _analyze(s.ref, s.g, s.aligned, s.pile, ["--pileup"])
    _analyze(s.ref, s.g, s.aligned, s.both, ["--pileup", "--siteSupport"])
    _analyze(s.ref, s.g, s.aligned, s.flag, ["--siteSupport"])
    _analyze(s.ref, s.g, s.aligned, s.flag0, ["--varMaxGroup", "0", "--siteSupport"])
    _analyze(s.ref, s.g, s.aligned, s.nobc, ["--siteSupport"], barcode=False)
    s.gold = os.path.join(util.GOLDEN, "analyzer_variants", "het" if s.het else "homo")
    return s


def test_counts_are_the_pileup_and_the_variant_is_supported(snp):
    vcf = _vcf(snp.both + "_allele.vcf")
    assert len(vcf) >= 1
    rows = _counts_are_the_pileup(snp.both + "_allele_support.tsv", snp.both + "_allele_pileup.tsv", {(v[0], v[1] + 1) for v in vcf})
    for name, pos, ref_base, var in vcf:
        at = [r for r in rows if (r[0], r[1], r[5]) == (name, pos + 1, var)]
        assert len(at) == 1 and var in at[0][4].split(",") and at[0][3] == ref_base
        v = at[0][6]
        assert v["fwd"] > 0 and v["rev"] > 0 and v["templates"] >= 2, v                          # seen on both strands, by more than one molecule
    # with or without --pileup or --barcode beside it
    assert _read(snp.flag + "_allele_support.tsv") == _read(snp.both + "_allele_support.tsv") == _read(snp.nobc + "_allele_support.tsv")


def test_nothing_else_changes(snp):
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(snp.flag + tail) == _read(snp.both + tail) == _read(snp.gold + tail) == _read(snp.plain + tail), tail
    assert _read(snp.nobc + "_allele.vcf") == _read(snp.plain + "_allele.vcf")
    assert _read(snp.both + "_allele_pileup.tsv") == _read(snp.pile + "_allele_pileup.tsv")     # (the goldens hold no pileup: the run without the flag)
    assert not os.path.exists(snp.plain + "_allele_support.tsv") and not os.path.exists(snp.pile + "_allele_support.tsv")
    assert sorted(os.path.basename(p) for p in glob.glob(snp.flag + "_*")) == ["flag_allele.vcf", "flag_allele_support.tsv", "flag_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.both + "_*")) == ["both_allele.vcf", "both_allele_pileup.tsv", "both_allele_support.tsv", "both_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.nobc + "_*")) == ["nobc_allele.vcf", "nobc_allele_support.tsv"]
    # no variant calling and no --sites: no site, the header alone
    assert _read(snp.flag0 + "_allele_support.tsv").decode() == ref.HEADER + "\n" and _read(snp.flag0 + "_allele.vcf") == b""


def test_sites_without_variant_calling(snp):
    """--varMaxGroup 0 --siteSupport --sites: the alignments are made although nothing is called -- the same lines, the var column empty"""
    name, pos, _, _ = _vcf(snp.both + "_allele.vcf")[0]
    f = os.path.join(snp.tmp, "one_site.tsv")
    open(f, "w").write("%s\t%d\n" % (name, pos + 1))
    o = os.path.join(snp.tmp, "sites0")
    _analyze(snp.ref, snp.g, snp.aligned, o, ["--varMaxGroup", "0", "--siteSupport", "--sites", f], barcode=False)
    _, rows = ref.parse(o + "_allele_support.tsv")
    _, called = ref.parse(snp.both + "_allele_support.tsv")
    assert _read(o + "_allele.vcf") == b"" and len(rows) >= 1
    assert [r[:4] + r[5:] for r in rows] == [r[:4] + r[5:] for r in called if (r[0], r[1]) == (name, pos + 1)] and all(r[4] == "." for r in rows)


# ---- 9. the golden chain -------------------------------------------------------------------------------------------------------------
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
    r = _analyze(c.ref, g, aligned, flag, c.flags + ["--pileup", "--siteSupport", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"})
    print("\n".join(l for l in r.stderr.split("\n") if l.startswith("site support: ")))
    sites = set(file_sites) | {(v[0], v[1] + 1) for v in _vcf(flag + "_allele.vcf")}
    rows = _counts_are_the_pileup(flag + "_allele_support.tsv", flag + "_allele_pileup.tsv", sites)
    assert len(rows) > 100 and len({r[5] for r in rows}) >= 4
    # line order: the alleles in the order of _allele_pileup.tsv, then pos, then obs in the order A C G T N - +
    al_rank = {}
    for row in pileup_ref.parse(flag + "_allele_pileup.tsv")[1]:
        al_rank.setdefault(row[0], len(al_rank))
    order = [(al_rank[r[0]], r[1], ref.STATES.index(r[5])) for r in rows]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
