"""The read-group fold (t1k_rowset_coalesce: k_co_reduce and k_co_reduce_long) against a plain restatement of
Genotyper::CoalesceReadAssignments (tests/coalesce_ref.py), entry by entry, at its run-length edges (pytest -m gpu).

Rows come from the real path -- host-made overlap lists (t1k_overlaps_upload), paired into a rowset by t1k_pair_into -- and are first
checked against the oracle fragment by fragment, as test_gpu_pair.py does.  The expected table is coalesce_ref on the rows the rowset
returned; the GPU's table must equal it exactly: group numbering, group_ptr, first fragments, alleles, start, the order-dependent `end`
(Genotyper.hpp:893-894) and both float32 sums as bit patterns.  The sizes at which the fold changes its route come from
t1k_coalesce_limits (B rows per batch, L = first run length of the four-wavefront kernel, T slots per tile); every case asserts from L
and its own run lengths which kernel folds each group.  For every group of three or more fragments the test asserts on the CPU that the
restatement itself gives other weight bits and another `end` when the fold order is reversed, and other weight bits in every slot when
the last fragment is dropped: a wrong order, a lost or a doubled row cannot pass.

Value-only mutants of t1k_coalesce.hip these tests were seen to fail on (each built and run once):
  * `acc.end = e.y` in k_co_reduce: cases a, b, c, d, the child process, the exchange;
  * `a.y = e[u].y` in k_co_reduce_long's full batch, `cnt` from `total - b * CO_B - 1`, `loadPtrs(b + 7)`: both case-c tests and the child process;
  * `a.y = e[u].y` in k_co_reduce_long's batch that is not full: the runs of cases c and d whose last row lowers the group's `end` (low_last).
No value test can catch: the clamped slot `nSlots - 1` -> `0` (idle lanes' results are dropped); `<` for `<=` in `j + 2 * CO_B <= j1` at the
loop's entry or in `more` (the last full batch moves to the scalar loop: same rows, same order).  Ignoring `act` at the final store would write
behind the group's entries -- behind the table for its last group -- and was reasoned from the code, not run."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import t1k_amd
import util
import coalesce_ref as cr
import test_gpu_pair as tp   # World (the synthetic reference of 8 300 alleles, contexts, oracles), as_list, compare

pytestmark = pytest.mark.gpu

# The library reads T1K_CO_LONG_RUN once per process.  test_d_... runs cases a, b and d again in a process that has it at 34: there the same
# groups are folded by k_co_reduce_long.
LOWERED = os.environ.get("T1K_CO_LONG_RUN") is not None
CHILD_LIMIT = 60   # seconds for the child process, which takes about 2.2 s on an MI355X (a hang of the long fold's barriers ends there)
READ = "ACGTACGTACGTACGTACGTACGTACGTACGTACGT"  # (the reads' text is irrelevant to pairing)


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = tp.World(str(tmp_path_factory.mktemp("coalesce")))
    lo, hi = cr.POOL
    assert not any(lo <= a < hi for a in list(tp.SEPS) + list(tp.SHORT)) and cr.Fragments(0).separator == (5, tp.SEPS[5]) and hi <= tp.N_ALLELES
    w.verified = {}  # rows of a case that compare() has passed, for the second fold of the same lists
    w.rank_thread_left = False
    yield w
    if not w.rank_thread_left:  # (a rank thread that never came back sits inside a collective: nothing more is started on the GPU)
        w.close()


@pytest.fixture(scope="module")
def lim(built):
    B, L, T = t1k_amd.coalesce_limits()
    assert B >= 2 and T == 64 and L >= 2 * B + 2
    if LOWERED:
        assert L == max(2 * B + 2, int(os.environ["T1K_CO_LONG_RUN"]))
    else:
        assert L == 4096, "the production threshold of k_co_reduce_long"
    return B, L, T


def route(run, L):
    return "k_co_reduce_long" if run >= L else "k_co_reduce"


def check_table(label, want, got, got_counts, row_counts, L):
    """the GPU's table against the restatement's; the first differing (group, slot) is reported with its run length, slot count and kernel"""
    ptr, ent, first, runs = want
    assert got_counts == (len(first), len(ent), int((np.asarray(row_counts) > 0).sum())), "%s: counts of t1k_rowset_coalesce %s" % (label, got_counts)
    diff = cr.same_table(want, got)
    if diff is not None:
        what, g, q = diff
        k = int(ptr[g]) + q
        show = lambda e: "-" if k >= len(e) else "allele %d start %d end %d weight %r (0x%08x) adjust %r (0x%08x)" % (
            e["allele"][k], e["start"][k], e["end"][k], float(e["weight"][k]), e["weight"][k:k + 1].view(np.uint32)[0], float(e["adjust_weight"][k]),
            e["adjust_weight"][k:k + 1].view(np.uint32)[0])
        raise AssertionError("%s: %s differs first in group %d, slot %d: run of %d fragments, %d slots, folded by %s\n  expected %s\n  gpu      %s" % (
            label, what, g, q, runs[g], int(ptr[g + 1] - ptr[g]), route(runs[g], L), show(ent), show(got[1])))


def fold(w, L, label, fr, calls=None, key=None):
    """uploads the lists of `fr`, pairs them into a rowset (calls: [(first, behind)] fragment ranges, one t1k_pair_into each, in that order),
    checks every row against the oracle, coalesces, checks the table.  Returns (row counts, rows, expected table, the rowset's device bytes
    and row entries)."""
    ctx, orc = w.ctx(0.8, 0, 0)  # single ends, -n 0: no limit on the kept fragments
    counts, rec, has_n = fr.lists()
    ovl = cr.overlap_lists(rec, w.alen)
    F = len(counts)
    ctx.reads_upload([READ] * F)
    ctx.overlaps_upload(counts, ovl)
    rs = t1k_amd.Rowset(ctx, F)
    try:
        for lo, hi in calls or [(0, F)]:
            rs.pair_into(ctx, np.arange(lo, hi), None, has_n[lo:hi], frag_base=lo)
        rc, rows = rs.rows()
        assigned = rs.assigned()
        if key is not None and key in w.verified:   # the same lists once more: the rows compare() passed the first time
            vc, va, vr = w.verified[key]
            assert np.array_equal(rc, vc) and np.array_equal(assigned, va) and rows.tobytes() == vr.tobytes(), label + ": rows differ from the first fold's"
        else:
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            tp.compare(label, [(ovl[off[f]:off[f + 1]], None) for f in range(F)], has_n, orc, rc, assigned, rows)
            if key is not None:
                w.verified[key] = (rc, assigned, rows)
        assert int((rc > 0).sum()) == sum(fr.runs) and int(assigned.sum()) > sum(fr.runs), label  # (the separator fragments are assigned and have no row)
        want = cr.coalesce_ref(rc, rows)
        assert sorted(want[3].tolist()) == sorted(fr.runs), label
        got_counts = rs.coalesce()
        check_table(label, want, rs.groups(), got_counts, rc, L)
        assert rs.coalesce() == got_counts   # a second call: the same table
        check_table(label + ", coalesced again", want, rs.groups(), got_counts, rc, L)
        return rc, rows, want, rs.device_bytes()
    finally:
        rs.close()


def visible(label, fr, rc, rows):
    """the conditions under which the fold's errors change bits, on the CPU: for every group of three fragments or more (one fragment has
    no order; two floats add commutatively) the restatement gives other weight bits and another `end` in reversed order, and other weight
    bits in every slot without the run's last fragment"""
    for g, n in enumerate(fr.runs):
        fs = fr.fragments_of(g)
        assert len(fs) == n and (n < 2 or np.any(np.diff(fs) > 1)), "%s: group %d is contiguous in fragment order" % (label, g)
        if n >= 3:
            assert cr.order_conditions(rc, rows, fs) == (True, True, True), "%s: group %d (run %d, %d slots) would hide a wrong fold order" % (label, g, n, len(fr.patterns[g]))


def test_a_run_lengths_of_k_co_reduce(world, lim):
    """case a: one rowset with groups of 1, 2, 3, B, B + 1, 2 B, 2 B + 1, 2 B + 2, 3 B, 3 B + 1, 3 B + 2, 4 B + 1, 5 B, 6 B + 1 and 7 B + 5 fragments
    (those below L), three alleles each, all interleaved by a fixed shuffle with a fragment without a row at about every fifth place: group
    ids follow first appearance and no run is contiguous.  k_co_reduce's way through each run is restated from its loop (short_trace): no
    fold, the scalar loop alone up to 2 B, the pipelined loop from 2 B + 1 with one, two, three, five and six trips, scalar tails of 0, 1, B - 1 and more rows.
    (The pipelined loop always ends through `!more`: its loop condition is the previous trip's `more` and never fails.)"""
    B, L, T = lim
    fr = cr.case_a(B, L)
    assert fr.runs == cr.case_a_runs(B, L) and {route(n, L) for n in fr.runs} == {"k_co_reduce"} and {1, 2, 3, 2 * B, 2 * B + 1} <= set(fr.runs)
    trace = {n: cr.short_trace(n, B) for n in fr.runs}
    assert not trace[2 * B][0] and trace[2 * B][3] == 2 * B - 1 and trace[2 * B + 1] == (True, 1, "break", 0)
    if not LOWERED:
        assert len(fr.runs) == 15
        piped = [t for t in trace.values() if t[0]]
        assert {t[1] for t in piped} == {1, 2, 3, 5, 6} and {0, 1, B - 1} <= {t[3] for t in piped} and {t[2] for t in piped} == {"break"}
    rc, rows, want, _ = fold(world, L, "case a", fr)
    visible("case a", fr, rc, rows)
    first = want[2]
    assert np.array_equal(first, np.sort(first)) and len(set(first.tolist())) == len(fr.runs)


def test_b_slot_counts(world, lim):
    """case b: groups of 2 B + 3 fragments with 1, T - 1, T, T + 1 (twice), 2 T and 2 T + 1 alleles: the tile map, `q >= n` in a group's last tile,
    two and three tiles a group.  The pattern of T alleles is a strict prefix of one of T + 1; the two of T + 1 differ in their last allele
    only; every fragment lists its alleles in an order of its own and still lands in its pattern's one group."""
    B, L, T = lim
    fr = cr.case_b(B, T)
    sizes = [len(p) for p in fr.patterns]
    assert sizes == [1, T - 1, T, T + 1, T + 1, 2 * T, 2 * T + 1] and set(fr.runs) == {2 * B + 3}
    assert {route(n, L) for n in fr.runs} == ({"k_co_reduce_long"} if LOWERED else {"k_co_reduce"})
    s = [np.sort(p) for p in fr.patterns]
    assert np.array_equal(s[2], s[3][:T]) and np.array_equal(s[3][:T], s[4][:T]) and s[3][T] != s[4][T]
    for g, d in enumerate(fr.drawn[1:], 1):
        assert len(set(l.tobytes() for l in d["lists"])) > 1, "group %d: every fragment lists the alleles in the same order" % g
    rc, rows, want, _ = fold(world, L, "case b", fr)
    visible("case b", fr, rc, rows)
    assert len(want[2]) == len(sizes)  # one group a pattern, whatever the order of the lists
    assert sorted(np.diff(want[0].astype(np.int64)).tolist()) == sorted(sizes)


def case_c_expectations(B, L, T, fr):
    runs = fr.runs
    assert runs[:5] == [L - 1, L, L + 1, L + B + 1, L + 2 * B + 9], "the issue's five run lengths"
    assert [route(n, L) for n in runs] == ["k_co_reduce"] + ["k_co_reduce_long"] * (len(runs) - 1)
    batches = [cr.long_batches(n, B) for n in runs[1:]]
    # L = 4096, B = 16: 256 batches with a last one of 15 rows, 256 / 16, 257 / 16, 259 / 8, and the two added runs 258 / 1 and 259 / 9
    assert [b for b, _ in batches] == [(n - 2) // B + 1 for n in runs[1:]]
    assert {b % 4 for b, _ in batches} == {0, 1, 2, 3}, batches
    assert {B - 1, B, 1, 9} <= {last for _, last in batches}, batches
    assert [len(p) for p in fr.patterns] == [T + 1 if n == L else 3 for n in runs]


def last_third_first(F, pieces=1):
    """the fragments as t1k_pair_into calls: the last third first, then the first and the second; every third in `pieces` calls"""
    cut = [0, F // 3, 2 * F // 3, F]
    out = []
    for t in (2, 0, 1):
        edges = [cut[t] + (cut[t + 1] - cut[t]) * k // pieces for k in range(pieces + 1)]
        out += list(zip(edges[:-1], edges[1:]))
    return out


def test_c_long_fold_at_the_production_threshold(world, lim):
    """case c: runs of 4095 (the last of k_co_reduce), 4096 (the first of k_co_reduce_long), 4097, 4096 + B + 1 and 4096 + 2 B + 9 fragments, plus
    4096 + B + 2 and 4096 + 2 B + 10: the rows to fold are the run less its first fragment, so the five lengths alone give batch counts of
    256, 256, 257 and 259 (no residue 2 mod 4) and last batches of B - 1, B, B and 8 rows; the two added runs bring 258 batches and the last
    batches of 1 and 9 rows.  The run of 4096 has T + 1 alleles (a last tile with one active lane and 63 clamped ones), the others 3.  The
    groups are interleaved, and the fragments enter by three t1k_pair_into calls, the last third first: the order of the rows in device
    memory is not fragment order."""
    B, L, T = lim
    if LOWERED:
        pytest.skip("T1K_CO_LONG_RUN is set: the production threshold is not in force in this process")  # (the child process does not select this test)
    fr = cr.case_c(B, L, T)
    case_c_expectations(B, L, T, fr)
    F = len(fr.order)
    rc, rows, want, (nbytes, entries) = fold(world, L, "case c", fr, calls=last_third_first(F), key="c")
    visible("case c", fr, rc, rows)
    for g, n in enumerate(fr.runs):   # the runs whose last batch has 1 and 9 rows: its last row lowers the group's `end`
        assert fr.low_last[g] == (n in (L + B + 2, L + 2 * B + 10)) and (not fr.low_last[g] or cr.last_row_fires(rc, rows, fr.fragments_of(g)))
    assert entries >= int(rc.sum())   # (the chunk cursors count what the calls reserved: no less than the rows kept)


def test_c_long_fold_over_several_row_chunks(world, lim, monkeypatch):
    """case c once more with row chunks of 65 536 entries (T1K_ROW_CHUNK, read when the rowset is made): the rows of a group lie in several chunks"""
    B, L, T = lim
    if LOWERED:
        pytest.skip("T1K_CO_LONG_RUN is set: the production threshold is not in force in this process")  # (the child process does not select this test)
    chunk = 65536
    monkeypatch.setenv("T1K_ROW_CHUNK", str(chunk))
    fr = cr.case_c(B, L, T)
    case_c_expectations(B, L, T, fr)
    F = len(fr.order)
    # A call whose rows do not fit the open chunk is run again into the next one, so a call must fit one chunk, as the job's windows do.  It
    # takes more than its rows: up to 1 024 workgroups reserve 32 entries at a time and leave what they hold unused when the launch ends, and
    # a row of 32 entries or more is reserved on its own.  24 calls of about 14 000 rows stay below that.
    calls = last_third_first(F, pieces=8)
    counts = fr.lists()[0].astype(np.int64)
    assert len(calls) == 24 and max(int(counts[lo:hi].sum()) for lo, hi in calls) * 3 // 2 + 32 * 1024 <= chunk
    rc, rows, want, (nbytes, entries) = fold(world, L, "case c, small chunks", fr, calls=calls, key="c")
    # every chunk holds at most `chunk` entries, so the rows lie in at least rows / chunk of them; the rowset's own account of its memory says
    # that it holds that many chunks of this size and not one of the default size (64 Mi entries)
    n_rows, esz = int(rc.sum()), t1k_amd.ROW_DTYPE.itemsize
    assert n_rows > 5 * chunk and entries >= n_rows
    assert (n_rows // chunk + 1) * chunk * esz <= nbytes < 64 * chunk * esz


def test_d_long_fold_on_short_runs(world, lim):
    """case d: runs of 2 B + 2 (with L = 34: 3 batches -- the fourth wavefront never folds and the prologue's second request is clamped), 2 B + 3,
    3 B + 1 (3 full batches), 4 B + 1 (4: one round exactly), 4 B + 2 (5: a second round of one batch), 8 B + 1, 8 B + 2, 9 B + 1 and 12 B + 7
    fragments, each with 1, T and T + 1 alleles.  In this process they are k_co_reduce's unless T1K_CO_LONG_RUN is lowered; the next test runs
    them in a process where it is 34.  Four more runs of three alleles end in last batches of 1, 2, 1 and 6 rows whose LAST row lowers the
    group's `end`: the fold of a batch that is not full has to apply the `end` rule too."""
    B, L, T = lim
    fr = cr.case_d(B, T)
    main = 3 * len(cr.case_d_runs(B))
    assert fr.runs[:main] == [n for n in cr.case_d_runs(B) for _ in range(3)] and [len(p) for p in fr.patterns[:main]] == [1, T, T + 1] * len(cr.case_d_runs(B))
    assert fr.runs[main:] == cr.case_d_tail_runs(B) and [cr.long_batches(n, B)[1] for n in fr.runs[main:]] == [1, 2, 1, 6] and fr.low_last[main:] == [True] * 4
    batches = [cr.long_batches(n, B) for n in cr.case_d_runs(B)]
    assert batches == [(3, 1), (3, 2), (3, B), (4, B), (5, 1), (8, B), (9, 1), (9, B), (13, 6)]
    assert {route(n, L) for n in fr.runs} == ({"k_co_reduce_long"} if LOWERED else {"k_co_reduce"})
    rc, rows, want, _ = fold(world, L, "case d", fr)
    visible("case d", fr, rc, rows)
    for g in range(main, len(fr.runs)):
        assert cr.last_row_fires(rc, rows, fr.fragments_of(g)), "group %d: the last row folded does not lower the group's `end`" % g


def test_d_in_a_child_process_with_the_long_fold_from_34(built):
    """cases a, b and d in a fresh process with T1K_CO_LONG_RUN=34: t1k_coalesce_limits reports the lowered threshold there, so case a keeps its
    runs below 34, and the groups of b (2 B + 3 fragments, up to three tiles) and d are asserted to be k_co_reduce_long's"""
    if LOWERED:
        pytest.skip("T1K_CO_LONG_RUN is set: this process already folds the cases with the lowered threshold")
    env = dict(os.environ, T1K_CO_LONG_RUN="34")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_a_run_lengths or test_b_slot_counts or test_d_long_fold_on_short_runs"],
                       env=env, cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0 and "3 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-6000:]


def small_rowset(w, L, label, lists, has_n=None):
    """a rowset of len(lists) single-end fragments (each a list of tp.ov tuples): rows against the oracle, table against the restatement;
    returns (counts of t1k_rowset_coalesce, group_ptr, entries, first fragments, expected table)"""
    ctx, orc = w.ctx(0.8, 0, 0)
    F = len(lists)
    ls = [tp.as_list(l, w.alen) for l in lists]
    has_n = np.zeros(F, dtype=np.uint8) if has_n is None else np.asarray(has_n, dtype=np.uint8)
    ctx.reads_upload([READ] * F)
    ctx.overlaps_upload([len(l) for l in ls], np.concatenate(ls) if ls else np.zeros(0, dtype=t1k_amd.OVERLAP_DTYPE))
    rs = t1k_amd.Rowset(ctx, F)
    try:
        if F:
            rs.pair_into(ctx, np.arange(F), None, has_n)
        rc, rows = rs.rows()
        tp.compare(label, [(l, None) for l in ls], has_n, orc, rc, rs.assigned(), rows)
        want = cr.coalesce_ref(rc, rows)
        got_counts = rs.coalesce()
        got = rs.groups()
        check_table(label, want, got, got_counts, rc, L)
        return got_counts, got[0], got[1], got[2], want
    finally:
        rs.close()


def test_e_degenerate_tables(world, lim):
    """case e: no fragments; fragments without any row (M == 0); one fragment; 255, 256 and 257 fragments with a row on the last only (the
    block edge of the flag and compaction kernels); every fragment a group of its own (G == M == 1 000)"""
    B, L, T = lim
    w = world
    one = lambda a, s=50: [tp.ov(a, s, 1, 300)]
    counts, ptr, ent, first, _ = small_rowset(w, L, "no fragments", [])
    assert counts == (0, 0, 0) and ptr.tolist() == [0] and len(ent) == 0 and len(first) == 0
    counts, ptr, ent, first, _ = small_rowset(w, L, "no rows", [[] for _ in range(9)] + [[tp.ov(5, 150, 1, 200, rlen=100)]])  # (the last: across a separator)
    assert counts == (0, 0, 0) and ptr.tolist() == [0] and len(ent) == 0 and len(first) == 0
    counts, ptr, ent, first, _ = small_rowset(w, L, "one fragment", [one(77) + one(33)], has_n=[1])
    assert counts == (1, 2, 1) and ptr.tolist() == [0, 2] and first.tolist() == [0] and ent["allele"].tolist() == [33, 77]
    assert ent["weight"].tolist() == [np.float32(0.1)] * 2 and ent["start"].tolist() == [50, 50] and ent["end"].tolist() == [199, 199]
    for F in (255, 256, 257):
        counts, ptr, ent, first, _ = small_rowset(w, L, "%d fragments, the last has the row" % F, [[] for _ in range(F - 1)] + [one(F)])
        assert counts == (1, 1, 1) and first.tolist() == [F - 1] and ent["allele"].tolist() == [F]
    # 1 000 distinct patterns of one to three alleles, in an order that is not the patterns' own
    rng = np.random.default_rng(5)
    pats = [[int(a) for a in (1000 + k, 3000 + (k * 7) % 1000, 5000 + (k * 13) % 1000)[:1 + k % 3]] for k in range(1000)]
    rng.shuffle(pats)
    lists = [[tp.ov(a, 20 + (k + a) % 200, 1, 300) for a in (p if k % 2 else p[::-1])] for k, p in enumerate(pats)]
    counts, ptr, ent, first, want = small_rowset(w, L, "every fragment its own group", lists, has_n=[k % 3 == 0 for k in range(1000)])
    assert counts == (1000, sum(len(p) for p in pats), 1000) and first.tolist() == list(range(1000)) and set(want[3].tolist()) == {1}


@pytest.mark.parametrize("ranks", [2, 3])
def test_f_exchange_does_not_change_the_groups(world, lim, ranks):
    """t1k_rowset_exchange: the fragments of case a plus one run of 12 B + 7 lie on `ranks` ranks (threads of this process on one GPU, the
    in-process transport), rank r holding the fragments [F r / R, F (r + 1) / R) in a rowset of its own; every row moves to the rank that
    owns its pattern, each rank folds its groups, the tables are gathered.  Ordered by first fragment they must be the one table of the
    restatement over all fragments, bit for bit, on every rank."""
    B, L, T = lim
    w = world
    fr = cr.case_a(B, L, extra=(12 * B + 7,))
    counts, rec, has_n = fr.lists()
    ovl = cr.overlap_lists(rec, w.alen)
    F = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ctx0, orc = w.ctx(0.8, 0, 0)
    cut = [F * r // ranks for r in range(ranks + 1)]
    ctxs, sets, parts = [], [], []
    group = t1k_amd.CommGroup(ranks)
    for r in range(ranks):  # everything that is not collective happens here, one rank after the other
        lo, hi = cut[r], cut[r + 1]
        c = t1k_amd.Context(ref_seq_similarity=0.8, max_assign_cnt=-1)
        c.ref_share(ctx0)
        c.reads_upload([READ] * (hi - lo))
        c.overlaps_upload(counts[lo:hi], ovl[off[lo]:off[hi]])
        rs = t1k_amd.Rowset(c, hi - lo)
        rs.pair_into(c, np.arange(hi - lo), None, has_n[lo:hi])   # local fragment indices
        ctxs.append(c)
        sets.append(rs)
        parts.append(rs.rows() + (rs.assigned(),))
    rc, rows, assigned = (np.concatenate([p[k] for p in parts]) for k in (0, 1, 2))
    tp.compare("exchange, %d ranks" % ranks, [(ovl[off[f]:off[f + 1]], None) for f in range(F)], has_n, orc, rc, assigned, rows)
    want = cr.coalesce_ref(rc, rows)
    visible("exchange", fr, rc, rows)
    out, errs, comms = [None] * ranks, [], [None] * ranks

    def rank_thread(r):
        try:
            # (collective: the ranks meet in it; a communicator that cannot be made aborts the meeting point itself before Comm raises)
            comms[r] = t1k_amd.Comm(ctxs[r], ranks, r, group=group, transport=0)
            sets[r].exchange(comms[r], cut[r])
            own = sets[r].coalesce()
            total = sets[r].groups_gather(comms[r])
            out[r] = (own, total, sets[r].groups_all())
        except BaseException as e:  # noqa: BLE001 -- a rank that cannot go on releases the ranks waiting for it
            errs.append((r, e))
            if comms[r] is not None:
                comms[r].abort()

    threads = [threading.Thread(target=rank_thread, args=(r,), daemon=True) for r in range(ranks)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 60   # for all ranks together
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        w.rank_thread_left = True   # nothing is closed: that would be GPU work beside a thread inside a collective
        raise AssertionError("a rank thread is still waiting: nothing more is started on the GPU")
    try:
        assert not errs, errs
        n_with_row = int((rc > 0).sum())
        owners = 0
        for r in range(ranks):
            own, total, (sizes, ent, first) = out[r]
            assert total == (len(want[2]), len(want[1]), n_with_row), "rank %d: totals %s" % (r, total)
            assert own[2] == int((parts[r][0] > 0).sum())   # the fragments with a row among this rank's own
            owners += own[0] > 0
            by = np.argsort(first, kind="stable")
            at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            take = np.concatenate([np.arange(at[g], at[g + 1]) for g in by])
            ptr = np.concatenate([[0], np.cumsum(sizes[by])]).astype(np.uint64)
            check_table("exchange, rank %d of %d" % (r, ranks), want, (ptr, ent[take], first[by]), total, rc, L)
        assert owners == ranks, "a rank owns no pattern: the exchange moved nothing to it"
    finally:
        for c in comms:
            if c is not None:
                c.close()
        for rs in sets:
            rs.close()
        for c in ctxs:
            c.close()
        group.close()
