"""GPU tests of the indel table (t1k_indel_*, analyzer --indels): the kernel and the fold against the sequential restatement,
every key, count and statistic exactly; hand-made edit strings at the kernel's edges with their keys written out; the argument errors, none
of which may emit anything; the analyzer's file against the restatement fed with the CPU oracle's alignments, line for line; its counts
against --pileup; every other output unchanged; the golden chain."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import goldens
import indel_ref as ref
import pileup_ref
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
    keys, counts, ms, stats = ctx.indel(*ref.args(t), cuts=cuts)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (counts > 0).all()             # runs ascending by key, one per key
    return keys, counts, ms, stats


def _same(keys, counts, stats, want):
    """every key and count, the table through from_runs, and the four integers of t1k_indel_stats"""
    wk, wc = ref.expected_runs(want)
    return keys.tolist() == wk and counts.tolist() == wc and ref.from_runs(keys, counts) == want.ev and tuple(stats[:4]) == ref.stats(want)


# ---- 1. kernel = restatement ---------------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement(ctx, table, want):
    keys, counts, ms, stats = _kernel(ctx, table)
    print("events %d, shifted %d, edge del %d, edge ins %d, keys %d, folds %d; kernels %.3f ms, fold %.3f ms" % (stats[:6] + (ms, stats[6])))
    assert len(want.ev) > 3000 and want.shifted > 300 and _same(keys, counts, stats, want)
    assert stats[4] == sum(v[0] for v in want.ev.values()) and ms > 0 and stats[5] == 1


# ---- 2. several calls, several folds -------------------------------------------------------------------------------------------------
def test_three_calls_give_the_same_table(ctx, table, want):
    keys, counts, _, stats = _kernel(ctx, table, cuts=(1401, 3800))
    assert _same(keys, counts, stats, want)


def test_several_folds_give_the_same_table(ctx, table, want, monkeypatch):
    monkeypatch.setenv("T1K_INDEL_PENDING", "1000")            # every one of the six calls emits more: a fold behind each
    keys, counts, _, stats = _kernel(ctx, table, cuts=(1000, 2000, 3000, 4000, 5000))
    assert stats[5] >= 3 and _same(keys, counts, stats, want)


# ---- 3. hand-made edges --------------------------------------------------------------------------------------------------------------
# one allele of 140 bases: GGGGGG at 0, AAAA at 20 .. 23 (a C in front of it and behind it)
FILL = "GTATCGGCTACCGCAAAAATAGTACCCTATTTACGCGGGATGTCCTAACGATCAGTTTCATGTAAGCCTAGCCTACAACGGCATTAACATGGCGTATACTTATTCCTTGCATCGG"
ALLELE = "GGGGGGT" + "CAGTCGATCTGAC" + "AAAA" + "C" + FILL
OFF = np.array([0, 140], np.uint64)


def _key(g, typ, payload, strand, uniq):
    return ((((g << 2 | typ) << 27 | payload) << 1 | strand) << 1) | (1 - uniq)


def _edge(recs, books, strand=None):
    """recs: (seq_start, [("M", n) | ("D", n) | ("I", bases)]) on ALLELE, the read copied from it -> the arguments of Context.indel"""
    aln, ops, text = [], [], b""
    for start, parts in recs:
        e, read, t = [], b"", start
        for kind, v in parts:
            if kind == "M":
                e += [0] * v
                read += ALLELE[t:t + v].encode()
                t += v
            elif kind == "D":
                e += [3] * v
                t += v
            else:
                e += [2] * len(v)
                read += v
        assert t <= len(ALLELE)
        aln.append((0, start, len(text), len(ops), len(e), 0, 0, 0))
        ops += e
        text += read
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in books])]).astype(np.uint64)
    uniq = np.array([u for b in books for u in b], np.uint8)
    strand = np.zeros(len(aln), np.uint8) if strand is None else np.array(strand, np.uint8)
    return (OFF, ALLELE.encode(), np.array(aln, t1k_amd.PILEUP_ALN_DTYPE), strand, ptr, uniq, text, np.array(ops, np.int8))


def _edge_run(ctx, recs, books, strand=None, cuts=()):
    args = _edge(recs, books, strand)
    keys, counts, _, stats = ctx.indel(*args, cuts=cuts)
    want = ref.restate(*args)
    assert ref.from_runs(keys, counts) == want.ev and tuple(stats[:4]) == ref.stats(want)    # (beside the keys written out by the caller)
    return keys.tolist(), counts.tolist(), stats


def test_deletions_against_the_step_seam(ctx):
    assert len(ALLELE) == 140 and ALLELE[89] != ALLELE[93] and ALLELE[91] != ALLELE[94]     # neither shifts
    # columns 60 .. 63 and 62 .. 64 of records from position 30: detected by lane 0 of the second step and by lane 1
    keys, counts, stats = _edge_run(ctx, [(30, [("M", 60), ("D", 4), ("M", 10)]), (30, [("M", 62), ("D", 3), ("M", 10)])], [[1], [0]])
    assert keys == [_key(90, 0, 4, 0, 1), _key(92, 0, 3, 0, 0)] and counts == [1, 1] and stats[:4] == (2, 0, 0, 0)


def test_insertion_of_70_columns_is_a_long_key(ctx):
    keys, counts, stats = _edge_run(ctx, [(30, [("M", 10), ("I", b"ACGTTGCA" * 8 + b"ACGTTG"), ("M", 10)])], [[1]])
    assert keys == [_key(40, 2, 70, 0, 1)] and counts == [1] and stats[:4] == (1, 0, 0, 0)


def test_insertions_of_13_and_of_14_bases(ctx):
    # ACGTACGTACGTA in front of position 40, behind an A: one shift, AACGTACGTACGT in front of 39 -- the longest short key; 14 bases: a long key
    assert ALLELE[39] == "A" and ALLELE[38] != "T" and ALLELE[41] != "C"
    keys, counts, stats = _edge_run(ctx, [(30, [("M", 10), ("I", b"ACGTACGTACGTA"), ("M", 10)]), (30, [("M", 12), ("I", b"ACGTACGTACGTAC"), ("M", 10)])], [[0], [0]])
    assert keys == [_key(39, 1, (1 << 26) | int("0012301230123", 4), 0, 0), _key(42, 2, 14, 0, 0)] and counts == [1, 1] and stats[:4] == (2, 1, 0, 0)


def test_one_deletion_at_three_offsets_of_a_homopolymer_is_one_key(ctx):
    assert ALLELE[19:25] == "CAAAAC"
    keys, counts, stats = _edge_run(ctx, [(10, [("M", k - 10), ("D", 1), ("M", 20)]) for k in (20, 21, 22)], [[1], [0], [0]])
    assert keys == [_key(20, 0, 1, 0, 1), _key(20, 0, 1, 0, 0)] and counts == [1, 2] and stats[:4] == (3, 2, 0, 0)


def test_insertion_shifted_to_the_first_base(ctx):
    keys, counts, stats = _edge_run(ctx, [(0, [("M", 6), ("I", b"G"), ("M", 10)])], [[1]], strand=[1])
    assert keys == [_key(0, 1, (1 << 2) | 2, 1, 1)] and counts == [1] and stats[:4] == (1, 1, 0, 0)


def test_edge_runs_alone_give_no_key(ctx):
    keys, counts, stats = _edge_run(ctx, [(30, [("D", 2), ("M", 10), ("I", b"AC")]), (30, [("D", 5)]), (30, [("I", b"ACG")])], [[1, 0, 0], [1], [0, 0]])
    assert keys == [] and counts == [] and stats[:4] == (0, 0, 2 * 3 + 5, 2 * 3 + 3 * 2) and stats[4] == 0 and stats[5] == 0


def test_256_bookings_of_one_event(ctx):
    keys, counts, stats = _edge_run(ctx, [(30, [("M", 60), ("D", 4), ("M", 10)])], [[0] * 256])
    assert keys == [_key(90, 0, 4, 0, 0)] and counts == [256] and stats[:6] == (1, 0, 0, 0, 256, 1)


def test_fold_merges_a_folded_count_with_pending_keys(ctx, monkeypatch):
    monkeypatch.setenv("T1K_INDEL_PENDING", "1")               # a fold behind each of the two calls
    rec = (30, [("M", 60), ("D", 4), ("M", 10)])
    keys, counts, stats = _edge_run(ctx, [rec, rec], [[0] * 256, [0] * 256 + [1]], cuts=(1,))
    assert keys == [_key(90, 0, 4, 0, 1), _key(90, 0, 4, 0, 0)] and counts == [1, 512] and stats[:6] == (2, 0, 0, 0, 513, 2)


def test_a_second_session_holds_no_more_device_memory(ctx):
    """_end frees every block of the stage: what the context holds behind one begin / add / get / end (its scan and sort scratch stays, by
    design) is what it holds behind the next"""
    args = _edge([(30, [("M", 60), ("D", 4), ("M", 10)])], [[1]])
    ctx.indel(*args)
    held = ctx.mem_bytes()
    ctx.indel(*args)
    assert ctx.mem_bytes() == held


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_emit_nothing(built):
    c = t1k_amd.Context()
    try:
        off = pileup_ref.offsets([8, 5])
        alleles = b"ACGTACGT" + b"GGNCC"
        text = b"ACGACGTAC" + b"GTNCC"
        #               record A: M M D M I M (an event each way)   an op 4         record B on the second allele: M I M M
        ops = np.array([0, 0, 3, 0, 2, 0,                             0, 4, 0,        0, 2, 0, 0], np.int8)

        def rec(allele=0, seq_start=0, read_at=0, ops_at=0, n_ops=6):
            return np.array([(allele, seq_start, read_at, ops_at, n_ops, 0, 0, 0)], t1k_amd.PILEUP_ALN_DTYPE)

        def u8(*v):
            return np.array(v, np.uint8)

        def table():
            return ref.from_runs(*c.indel_get())
        one = (u8(0), np.array([0, 1], np.uint64), u8(1))
        assert c.indel_add(rec(), *one, text, ops, raw=True) == ERR_STATE and c.last_error().startswith("t1k_indel_add: ")   # add / get / end before begin
        assert c.indel_get(raw=True) == ERR_STATE and c.indel_end(raw=True) == ERR_STATE
        assert c.indel_begin(off, b"ACGTACGT" + b"GGnCC", raw=True) == ERR_ARG                     # a byte outside ACGTN
        assert c.indel_begin(off, b"ACGTACGT" + b"GG-CC", raw=True) == ERR_ARG
        assert c.indel_begin(np.array([0, 8, 5], np.uint64), alleles[:5], raw=True) == ERR_ARG      # the offsets decrease
        assert c.indel_get(raw=True) == ERR_STATE                                                  # none of them opened a table
        c.indel_begin(off, alleles)
        assert table() == {}
        assert c.indel_begin(off, alleles, raw=True) == ERR_STATE                                  # a table is open
        good = np.concatenate([rec(), rec(allele=1, seq_start=0, read_at=9, ops_at=9, n_ops=4)])
        gs, gp, gu = u8(0, 1), np.array([0, 2, 3], np.uint64), u8(1, 0, 1)
        assert c.indel_add(good, gs, gp, gu, text, ops, raw=True) == 0
        before = table()
        sound = ref.restate(off, alleles, good, gs, gp, gu, text, ops)
        assert before == sound.ev and len(before) == 3 and sum(v[0] for v in before.values()) == 5 and c.indel_stats()[:5] == ref.stats(sound) + (5,)

        def refused(bad, strand=0, ptr=(3, 4), uniq=(0,), code=ERR_ARG):
            p = np.concatenate([gp, np.array(ptr[1:], np.uint64)])
            assert c.indel_add(np.concatenate([good, bad]), np.concatenate([gs, u8(strand)]), p, np.concatenate([gu, u8(*uniq)]), text, ops, raw=True) == code
            assert c.last_error().startswith("t1k_indel_add: ")                                   # whoever refused it, host or device
            assert table() == before and c.indel_stats()[:5] == ref.stats(sound) + (5,)          # the sound records of the call emit nothing either
        # what pileupRecordFault and the device check refuse
        refused(rec(ops_at=6, n_ops=3))                   # op value 4
        refused(rec(allele=1, seq_start=3, ops_at=9, n_ops=4, read_at=9))   # a walk one base past the allele (3 bases from position 3 of 5)
        refused(rec(seq_start=4))                         # ... of the first allele: 5 bases from position 4 of 8
        refused(rec(read_at=10))                          # a walk past `text`: 5 bases from 10 of 14
        refused(rec(allele=2))                            # an allele id equal to nAlleles
        refused(rec(ops_at=8, n_ops=6))                   # an edit string that leaves `ops`
        refused(rec(read_at=15))                          # a read window that starts behind `text`
        refused(rec(seq_start=9))                         # a record that starts behind its allele
        refused(rec(), ptr=(3, 2))                        # bookPtr decreases
        refused(rec(ops_at=6, n_ops=3), ptr=(3, 3), uniq=())   # a bad record is refused even when it has no booking
        # the strand and the bookings
        refused(rec(), strand=2)
        refused(rec(), uniq=(2,))
        refused(rec(), ptr=(3, 5), uniq=(1, 255))
        refused(rec(), ptr=(3, 3 + 2 ** 31), code=ERR_CAPACITY)   # 2^31 bookings on one record (refused before any of them is read)
        more = (rec(allele=1, seq_start=0, read_at=9, ops_at=9, n_ops=4), u8(0), np.array([0, 2], np.uint64), u8(1, 0))
        assert c.indel_add(*more, text, ops, raw=True) == 0                                      # and the table still takes sound calls
        both = ref.restate(off, alleles, np.concatenate([good, more[0]]), np.concatenate([gs, more[1]]), np.array([0, 2, 3, 5], np.uint64), np.concatenate([gu, more[3]]), text, ops)
        assert table() == both.ev and len(both.ev) == 4 and c.indel_stats()[:5] == ref.stats(both) + (7,)
        c.indel_end()
        assert c.indel_add(rec(), *one, text, ops, raw=True) == ERR_STATE
        assert c.indel_get(raw=True) == ERR_STATE and c.indel_end(raw=True) == ERR_STATE
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


def _phase_line(r):
    """the numbers of the `indels:` line of T1K_DEBUG_PHASES: {records, events, shifted, edge_del, edge_ins, keys, folds}"""
    line = [l for l in r.stderr.split("\n") if l.startswith("indels: ")]
    assert len(line) == 1, r.stderr[-2000:]
    print(line[0])
    m = re.match(r"indels: (\d+) records, (\d+) events, (\d+) shifted, (\d+) \+ (\d+) edge columns, (\d+) keys emitted, (\d+) folds, .* ms", line[0])
    assert m, line[0]
    return dict(zip(("records", "events", "shifted", "edge_del", "edge_ins", "keys", "folds"), (int(v) for v in m.groups())))


def _counts_are_the_pileup(indel_path, pile_path, stats):
    """per plane: sum of count x len over the DEL lines + the booked edge deletion columns = the sum of the `del` column of the pileup; the
    same for INS; count_uniq <= count and fwd + rev == count on every line.  (Run with --indelMinCount 1: every event has its line)"""
    header, rows = ref.parse(indel_path)
    assert header == ref.HEADER
    _, pile = pileup_ref.parse(pile_path)
    for typ, col, edge in (("DEL", "del", "edge_del"), ("INS", "ins", "edge_ins")):
        mine = [r for r in rows if r[3] == typ]
        assert sum(r[6]["count"] * r[4] for r in mine) + stats[edge] == sum(p[4][col] for p in pile), typ
    # (_uniq: the edge columns of uniq bookings are not reported apart, so the uniq planes bound the lines from above)
    assert sum(r[6]["count_uniq"] * r[4] for r in rows if r[3] == "DEL") <= sum(p[4]["del_uniq"] for p in pile)
    assert sum(r[6]["count_uniq"] * r[4] for r in rows if r[3] == "INS") <= sum(p[4]["ins_uniq"] for p in pile)
    for r in rows:
        v = r[6]
        assert 0 <= v["count_uniq"] <= v["count"] and v["fwd"] + v["rev"] == v["count"] > 0 and r[4] >= 1, r
        assert (r[5] == "*") or len(r[5]) == r[4], r
    return rows


def _in_file_order(rows, pile_path):
    """by allele in the order of _allele_pileup.tsv, then pos, then DEL before INS, then len, then seq; no key twice"""
    rank = {}
    for row in pileup_ref.parse(pile_path)[1]:
        rank.setdefault(row[0], len(rank))
    order = [(rank[r[0]], r[1], 0 if r[3] == "DEL" else 1, r[4], r[5]) for r in rows]
    return order == sorted(order) and len(set(order)) == len(order)


# ---- 5. analyzer = restatement on the CPU oracle's alignments; 6. counts are the pileup ------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
def test_analyzer_equals_restatement_on_the_oracles_alignments(built, tmp_path, single):
    """(the same seeds for both runs: with the reference genotyper and the restatement alone, one record per assignment overlap, the paired run
    shows 20 shifted events, 13 of them deletions, the single-end run 7, 5 of them deletions)"""
    tmp = str(tmp_path)
    ref_fa, pfx, runs = ref.planted_deletion_sample(tmp)
    g, aligned = _genotype(tmp, ref_fa, pfx, single)
    sel, out, names, _ = oracle_dump(tmp, ref_fa, g, aligned)
    ref_names, seqs, masks, _ = t1k_amd.load_reference_fasta(sel)
    assert ref_names == names
    r1 = [s for _, _, s in t1k_amd.read_fastx(aligned[1])]
    r2 = None if single else [s for _, _, s in t1k_amd.read_fastx(aligned[3])]
    ptr, asg, ops = parse_dump(out + "_fragdump.tsv", len(r1))
    assert len(asg) > 1000 and (np.diff(ptr.astype(np.int64)) > 1).any()
    off = pileup_ref.offsets([len(s) for s in seqs])
    aln, text, strand, book_ptr, book_uniq = ref.analyzer_records(ptr, asg, r1, r2)
    assert set(np.unique(strand)) == {0, 1} and set(np.unique(book_uniq)) == {0, 1}
    table = ref.restate(off, "".join(seqs).encode(), aln, strand, book_ptr, book_uniq, text, ops)
    assert table.shifted > 0 and any(e[3] == 3 and e[5] < e[4] for e in table.trace)         # the normalisation is at work, on deletions too
    rows = ref.lines(table.ev, off, seqs)
    want = ref.table_text(names, seqs, masks, rows).split("\n")
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--indels", "--pileup"], env={"T1K_DEBUG_PHASES": "1"}, barcode=False)
    stats = _phase_line(r)
    got = open(a + "_allele_indel.tsv").read().split("\n")
    assert len(got) == len(want) > 200                      # (the floor only keeps the comparison from being empty)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    # the analyzer walks a shared alignment once: fewer events than one per assignment overlap, the booked numbers the same
    assert 0 < stats["shifted"] <= table.shifted and 0 < stats["events"] <= table.events and stats["records"] <= len(aln)
    assert (stats["edge_del"], stats["edge_ins"]) == (table.edge_del, table.edge_ins) and stats["keys"] == sum(v[0] for v in table.ev.values())
    # the planted deletion: on both selected alleles of the gene, at the first base of the run, on both strands; nothing of its length inside the run
    parsed = _counts_are_the_pileup(a + "_allele_indel.tsv", a + "_allele_pileup.tsv", stats)
    assert _in_file_order(parsed, a + "_allele_pileup.tsv")
    planted = [n for n in names if n in runs]
    assert len(planted) == 2
    for n in planted:
        lo, hi = runs[n]
        assert hi - lo >= 2
        inside = [x for x in parsed if x[0] == n and x[3] == "DEL" and x[4] == 1 and lo + 1 <= x[1] <= hi]
        assert len(inside) == 1 and inside[0][1] == lo + 1 and inside[0][6]["fwd"] > 0 and inside[0][6]["rev"] > 0 and inside[0][6]["count"] >= 50, inside
    # the variant pass in several pieces, and with every alignment through the device: the same bytes
    for tag, env in (("piece", {"T1K_ANALYZER_PIECE": "600"}), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"})):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--indels"], env=env, barcode=False)
        assert _read(o + "_allele_indel.tsv") == _read(a + "_allele_indel.tsv"), tag
    # 7. --indelMinCount 3: exactly the lines with count >= 3
    o = os.path.join(tmp, "min3")
    _analyze(ref_fa, g, aligned, o, ["--indels", "--indelMinCount", "3"], barcode=False)
    got3 = open(o + "_allele_indel.tsv").read().split("\n")
    keep = [l for l in got[1:-1] if int(l.split("\t")[6]) >= 3]
    assert got3 == [got[0]] + keep + [""] and 2 <= len(keep) < len(got) - 2
    assert got3 == ref.table_text(names, seqs, masks, ref.lines(table.ev, off, seqs, min_count=3)).split("\n")


# ---- 8. nothing else changes ---------------------------------------------------------------------------------------------------------
class Runs:
    pass


@pytest.fixture(scope="module")
def snp(built, tmp_path_factory):
    """the novel-SNP sample (homozygous) through this build's genotyper, then the analyzer several ways"""
    tmp = str(tmp_path_factory.mktemp("indel_snp"))
    s = Runs()
    s.tmp = tmp
    s.ref, pfx = util.novel_snp_sample(tmp, False)
    s.g, s.aligned = _genotype(tmp, s.ref, pfx)
    s.plain, s.pile, s.both, s.flag, s.flag0, s.nobc, s.sup = (os.path.join(tmp, x) for x in ("plain", "pile", "both", "flag", "flag0", "nobc", "sup"))
    _analyze(s.ref, s.g, s.aligned, s.plain)
    _analyze(s.ref, s.g, s.aligned, s.pile, ["--pileup"])
    _analyze(s.ref, s.g, s.aligned, s.both, ["--pileup", "--indels"])
    _analyze(s.ref, s.g, s.aligned, s.flag, ["--indels"])
    _analyze(s.ref, s.g, s.aligned, s.flag0, ["--varMaxGroup", "0", "--indels"])
    _analyze(s.ref, s.g, s.aligned, s.nobc, ["--indels"], barcode=False)
    _analyze(s.ref, s.g, s.aligned, s.sup, ["--siteSupport", "--indels"], barcode=False)
    s.gold = os.path.join(util.GOLDEN, "analyzer_variants", "homo")
    return s


def test_nothing_else_changes(snp):
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(snp.flag + tail) == _read(snp.both + tail) == _read(snp.gold + tail) == _read(snp.plain + tail), tail
    assert _read(snp.nobc + "_allele.vcf") == _read(snp.plain + "_allele.vcf") == _read(snp.sup + "_allele.vcf")
    assert _read(snp.both + "_allele_pileup.tsv") == _read(snp.pile + "_allele_pileup.tsv")
    assert not os.path.exists(snp.plain + "_allele_indel.tsv") and not os.path.exists(snp.pile + "_allele_indel.tsv")
    assert sorted(os.path.basename(p) for p in glob.glob(snp.plain + "_*")) == ["plain_allele.vcf", "plain_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.flag + "_*")) == ["flag_allele.vcf", "flag_allele_indel.tsv", "flag_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.both + "_*")) == ["both_allele.vcf", "both_allele_indel.tsv", "both_allele_pileup.tsv", "both_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.nobc + "_*")) == ["nobc_allele.vcf", "nobc_allele_indel.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.sup + "_*")) == ["sup_allele.vcf", "sup_allele_indel.tsv", "sup_allele_support.tsv"]
    # the file with and without --barcode, with --pileup or --siteSupport beside it, and without variant calling (an empty VCF)
    one = _read(snp.flag + "_allele_indel.tsv")
    assert one.decode().split("\n")[0] == ref.HEADER
    assert one == _read(snp.both + "_allele_indel.tsv") == _read(snp.nobc + "_allele_indel.tsv") == _read(snp.sup + "_allele_indel.tsv") == _read(snp.flag0 + "_allele_indel.tsv")
    assert _read(snp.flag0 + "_allele.vcf") == b""


# ---- 9. the golden chain -------------------------------------------------------------------------------------------------------------
def test_golden_chain(built, tmp_path):
    tmp = str(tmp_path)
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    _run([GENO] + c.args() + ["-o", g])
    aligned = ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"]
    flag = os.path.join(tmp, "flag")
    r = _analyze(c.ref, g, aligned, flag, c.flags + ["--pileup", "--indels"], env={"T1K_DEBUG_PHASES": "1"})
    stats = _phase_line(r)
    rows = _counts_are_the_pileup(flag + "_allele_indel.tsv", flag + "_allele_pileup.tsv", stats)
    assert _in_file_order(rows, flag + "_allele_pileup.tsv")
    assert stats["records"] > 0 and len(rows) >= 1 and stats["keys"] == sum(x[6]["count"] for x in rows)   # (the floors only keep the run from being empty)
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
