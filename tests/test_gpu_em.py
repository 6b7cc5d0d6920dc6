"""t1k_em_setup / t1k_em_update / t1k_em_shard (k_em_psum, k_em_cols, the class-major sort) against the restatement of
Genotyper::EMupdate (tests/em_ref.py), bit for bit, at the edges of the kernels' pieces (pytest -m gpu).

The row pass adds a read group's abundances P at a time and carries the sum from piece to piece; the class pass takes S entries per
step in ordered pieces of P, requests the read groups of the step after next and the count / psum of the next step before it adds the
current one.  P and S come from t1k_em_limits; every case asserts from its own inputs that it holds the lengths it is about, and that at
least half of its long rows and long classes get another sum when added backwards (test_em_cpu.py does the same without a GPU, and
holds the restatement to the oracle and to exact sums).  n, x1 and diff are compared as bit patterns; NaN only where the restatement
has NaN (a table without entries: 0 / 0).

Case e's start: from abundances of 10 ** uniform(-9, 0) the FIRST extrapolation cannot leave [0, 1] by much (alpha is about -1 there, so
x3 is about x2: its entries stay below 1 and only a few dip below 0); it is the second round's vector that reaches from -3.0 to 6.3 and
the third's that still exceeds 1, so the assertion is on the four rounds' vectors, not on the first alone.

Value-only mutants of t1k_em.hip these tests were seen to fail on (each built and run once):
  * the carry reset per piece in k_em_psum (`waveOrderedSum(v, cnt, 0, ...)`): cases a, b, f and the case-a step of d; cases c and e pass (their
    rows are shorter than P), and so does test_gpu_parity.py::test_em_update_bit_exact;
  * `rows(base + S)` for `rows(base + 2 * S)` in k_em_cols: cases c and e, in exactly the 13 classes of more than 2 S entries, and d's E = 1;
  * the unrolled loop of waveOrderedSum running j downwards, and one sort bit too few in t1k_em_setup (never fewer than one: no bits at
    all is outside the sort's contract): every test;
  * `<=` in the rowLo / rowHi mask: the two allreduce tests of case f and nothing else.
Row-range errors are provoked without a communicator only: a rank refused before the gather of the ranges would leave the others waiting."""
import threading
import time

import numpy as np
import pytest

import t1k_amd
import em_ref as er

pytestmark = pytest.mark.gpu
T1K_ERR_ARG = -1


class World:
    rank_thread_left = False


@pytest.fixture(scope="module")
def lim(built):
    P, S = t1k_amd.em_limits()
    assert P == 64 and S % P == 0 and S >= 2 * P, "one operand per lane of a wavefront; whole pieces per step"
    return P, S


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    if not World.rank_thread_left:  # (a rank thread that never came back sits inside a collective: nothing more is started on the GPU)
        c.close()


def check(label, got, want, t=None):
    """(x1, n, diff) of t1k_em_update against the restatement's; the first differing class is reported with its size"""
    for what, k in (("n", 1), ("x1", 0), ("diff", 2)):
        if not er.same_bits(got[k], want[k]):
            i, g, w, cnt = er.first_difference(got[k], want[k])
            size = "" if t is None or what == "diff" else ", a class of %d entries" % int(t.class_sizes()[i])
            raise AssertionError("%s: %s differs in %d places, first at %d%s: gpu %r (%s), expected %r (%s)" % (label, what, cnt, i, size, g, float(g).hex(), w, float(w).hex()))


def visible(label, t, x0, P, skip=()):
    rc, rn, cc, cn = er.order_shares(t, x0, P, skip)
    assert 2 * rc >= rn and 2 * cc >= cn, "%s would hide a wrong order: %d of %d long rows, %d of %d long classes change when added backwards" % (label, rc, rn, cc, cn)
    return rn, cn


def run(ctx, label, t, x0=None, want=None, setup=True):
    x0 = t.x0 if x0 is None else x0
    if setup:
        ctx.em_setup(*t.args())
    got = ctx.em_update(x0)
    check(label, got, t.ref() if want is None else want, t)
    return got


@pytest.mark.parametrize("g_mod", [1, 2, 3])
def test_a_row_lengths(ctx, lim, g_mod):
    """case a: eight rows each of 0, 1, 2, P - 1, P, P + 1, 2 P - 1, 2 P, 2 P + 1, 3 P - 1, 3 P, 3 P + 1 and 4 P + 44 entries among 500 short ones; one
    of each length ends the table, the longest last, in a last block of g_mod rows.  One, two, three and five pieces, full and not, the
    carry over each piece edge."""
    P, S = lim
    t = er.case_a(P, g_mod)
    lens = t.row_lengths()
    for n in er.long_row_lengths(P):
        assert int((lens == n).sum()) >= 8, n
    assert t.G % 4 == g_mod and lens[-1] == 4 * P + 44 and lens[-13:].tolist() == er.long_row_lengths(P) and t.E >= 4 * P + 44
    assert visible("case a", t, t.x0, P)[0] >= 80
    run(ctx, "case a, G = %d mod 4" % g_mod, t)
    x1 = t.ref()[0]
    run(ctx, "case a, G = %d mod 4, second update" % g_mod, t, x0=x1, want=t.ref(x1, "x1"), setup=False)


def test_b_cancelling_and_zero_rows(ctx, lim):
    """case b (signed abundances): rows of P and P + 1 zeros (some of them -0.0) and a row of -0.0 alone: psum == 0 -> 1; rows of P + 1 whose
    last entry alone is not zero: the second piece holds one operand; rows [a, -a]; rows of P + 2 whose sum is exactly 0.0 in row order,
    but neither backwards nor when the first piece's sum is dropped; rows of negative abundances alone"""
    P, S = lim
    t, kinds = er.case_b(P)
    row_terms, _ = er.terms(t.row_ptr, t.ec_idx, t.count, t.x0, t.E)
    psum = [er.chain(r) for r in row_terms]
    for g in kinds["cancel"]:
        assert len(row_terms[g]) == P + 2 and psum[g] == 0.0 and er.chain(row_terms[g][::-1]) != 0.0 and er.chain(row_terms[g][P:]) != 0.0
    assert [len(row_terms[g]) for k in ("zeros P", "zeros P + 1") for g in kinds[k]] == [P, P + 1]
    assert all(psum[g] == 0.0 and not any(row_terms[g]) for k in ("zeros P", "zeros P + 1", "minus zeros") for g in kinds[k])
    assert all(np.signbit(v) for g in kinds["minus zeros"] for v in row_terms[g]) and any(np.signbit(v) for v in row_terms[kinds["zeros P"][0]])
    assert all(len(row_terms[g]) == P + 1 and not any(row_terms[g][:P]) and psum[g] == row_terms[g][P] != 0 for g in kinds["last entry alone"])
    assert all(len(row_terms[g]) == 2 and psum[g] == 0.0 and row_terms[g][0] != 0 for g in kinds["a, -a"])
    assert all(psum[g] < 0 for g in kinds["negative"]) and sum(1 for s in psum if s < 0) >= 20
    assert t.G % 4 == 1 and kinds["cancel"][-1] == t.G - 1
    visible("case b", t, t.x0, P)
    run(ctx, "case b", t)


@pytest.mark.parametrize("e_mod", [1, 2, 3])
def test_c_class_sizes(ctx, lim, e_mod):
    """case c: classes of 0, 1, P - 1, P, P + 1, S - P - 1, S - P, S - P + 1, S - 1, S, S + 1, S + P - 1, S + P, S + P + 1, 2 S - 1, 2 S, 2 S + 1, 3 S - 1, 3 S,
    3 S + 1, 3 S + P and 4 S + 1 entries as the first and as the last classes of the table (a last block of e_mod classes), one of
    10 S + 37 between them; rows shorter than P, so the row pass has one piece everywhere.  A class's end lies in the prologue's step, in the
    step the prologue requested, and in the first, second and third step requested by the loop, on and beside every piece and step edge.
    Then once more with x0 = 0 for every other sized class."""
    P, S = lim
    t = er.case_c(P, S, e_mod)
    sizes = er.class_sizes_c(P, S)
    got = t.class_sizes().tolist()
    assert got[:len(sizes)] == sizes and got[-len(sizes):] == sizes and 10 * S + 37 in got and t.E % 4 == e_mod
    assert {0, 1, P, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 1, 4 * S + 1} <= set(sizes)
    assert max(got) < t.G <= max(got) + 64 and int(t.row_lengths().max()) < P
    assert visible("case c", t, t.x0, P)[1] >= 35
    run(ctx, "case c, E = %d mod 4" % e_mod, t)
    x, off = er.zeroed_half(P, S, t)
    assert len(off) == len(sizes) and not x[off].any() and x[er.sized_classes_c(P, S, t)[0::2]].all()
    visible("case c with zeroed classes", t, x, P, skip=off)
    run(ctx, "case c, E = %d mod 4, half the sized classes at 0" % e_mod, t, x0=x, want=t.ref(x, "zeroed"), setup=False)


def test_d_setup_edges(lim):
    """case d, all on one context of its own: E = 65 536, 1, 65 537, 2, 255, 65 535, 256, 257 classes (16, 1, 17, 1, 8, 16, 8 and 9 sort bits) with 3 000
    rows of 1 .. 40 entries, in this order: large, small, large -- the page-locked staging grows twice, and buffers left by a larger table
    lie behind a smaller one's; then one row; rows without entries (0 / 0: NaN, as the reference); a class index equal to E in the last
    entry (T1K_ERR_ARG, `class index out of range`); and case a on the same context after the refusal."""
    P, S = lim
    c = t1k_amd.Context()
    try:
        assert [er.sort_bits(E) for E in er.SETUP_E] == [16, 1, 17, 1, 8, 16, 8, 9]
        for E in er.SETUP_E:
            t = er.case_d(E)
            assert t.E == E and t.G == 3000 and 1 <= t.row_lengths().min() and t.row_lengths().max() <= 40
            assert E > 300 or t.class_sizes().min() > 0
            run(c, "case d, E = %d" % E, t)
        t = er.case_d(300, 1)
        assert t.G == 1
        run(c, "case d, one row", t)
        t = er.case_d(5, 50, True)
        assert len(t.ec_idx) == 0 and t.G == 50
        got = run(c, "case d, rows without entries", t)
        assert np.isnan(got[0]).all() and not got[1].any() and np.isnan(got[2])
        t = er.case_d(257)
        bad = t.ec_idx.copy()
        bad[-1] = t.E
        assert c.em_setup(t.row_ptr, bad, t.count, t.ec_len, raw=True) == T1K_ERR_ARG and "class index out of range" in c.last_error()
        bad[-1], bad[0] = t.ec_idx[-1], 0xFFFFFFFF
        assert c.em_setup(t.row_ptr, bad, t.count, t.ec_len, raw=True) == T1K_ERR_ARG and "class index out of range" in c.last_error()
        run(c, "case a after a refused setup", er.case_a(P, 1))
    finally:
        c.close()


def test_e_squarem_rounds(ctx, lim):
    """case e: four SQUAREM rounds on the table of case c -- x0 -> x1 -> x2, the extrapolation x0 - 2 alpha r + alpha^2 v computed once in Python,
    x3 -> x1 -- with the GPU and the restatement fed the same vector at each of the twelve updates.  Every extrapolated vector has negative
    entries; the second reaches from below -1 to above 2, another one exceeds 1."""
    P, S = lim
    t, steps, x3s = er.case_e(P, S)
    assert len(steps) == 3 * er.SQUAREM_ROUNDS and all(float(x.min()) < 0 for x in x3s) and sum(1 for x in x3s if float(x.max()) > 1) >= 2
    assert float(x3s[1].min()) < -1 and float(x3s[1].max()) > 2
    visible("case e, start", t, steps[0][1], P)
    visible("case e, second extrapolation", t, x3s[1], P)
    ctx.em_setup(*t.args())
    for name, x, want in steps:
        check("case e, " + name, ctx.em_update(x), want, t)


def sharded(ranks, plan):
    """every rank (a thread with a context and a communicator of its own, the in-process transport) sets up each table of `plan`
    [(table, [cuts])] whole, then for every cuts takes its slice (t1k_em_shard) and runs two chained updates; at the end the ranks offer
    ranges with a gap.  Returns per rank ([(table index, cuts, update 1, update 2)], the gap's status, its message)."""
    # the ranges with a gap, on the table set up last: its first cuts with rank 1 starting one row late.  Every rank's own range is sound, so
    # every rank reaches the gather of the ranges and sees the same table: all are refused, none waits
    t, cuts = plan[-1][0], plan[-1][1][0]
    gap = [(cuts[r] + (1 if r == 1 else 0), cuts[r + 1]) for r in range(ranks)]
    assert all(lo <= hi <= t.G for lo, hi in gap) and gap[1][0] != gap[0][1]
    for t, cuts_list in plan:   # (a range its own rank refuses would leave the other ranks waiting in the gather)
        assert all(len(c) == ranks + 1 and c[0] == 0 and c[-1] == t.G and all(a <= b for a, b in zip(c[:-1], c[1:])) for c in cuts_list)
    group = t1k_amd.CommGroup(ranks)
    ctxs = [t1k_amd.Context() for _ in range(ranks)]
    out, errs, comms = [None] * ranks, [], [None] * ranks

    def rank_thread(r):
        try:
            # (collective: the ranks meet in it; a communicator that cannot be made aborts the meeting point itself before Comm raises)
            comms[r] = t1k_amd.Comm(ctxs[r], ranks, r, group=group, transport=0)
            c, res = ctxs[r], []
            for k, (t, cuts_list) in enumerate(plan):
                c.em_setup(*t.args())
                for cuts in cuts_list:
                    c.em_shard(cuts[r], cuts[r + 1], comms[r])
                    u1 = c.em_update(t.x0)
                    res.append((k, cuts, u1, c.em_update(u1[0])))
            rc = c.em_shard(gap[r][0], gap[r][1], comms[r], raw=True)
            out[r] = (res, rc, c.last_error())
        except BaseException as e:  # noqa: BLE001 -- a rank that cannot go on releases the ranks waiting for it
            errs.append((r, e))
            if comms[r] is not None:
                comms[r].abort()

    threads = [threading.Thread(target=rank_thread, args=(r,), daemon=True) for r in range(ranks)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + 60   # for all ranks together
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    if any(th.is_alive() for th in threads):
        World.rank_thread_left = True   # nothing is closed: that would be GPU work beside a thread inside a collective
        raise AssertionError("a rank thread is still waiting: nothing more is started on the GPU")
    try:
        assert not errs, errs
        return out
    finally:
        for c in comms:
            if c is not None:
                c.close()
        for c in ctxs:
            c.close()
        group.close()


@pytest.mark.parametrize("mode", ["gather", "allreduce"])
@pytest.mark.parametrize("ranks", [2, 3])
def test_f_sharded(ctx, lim, monkeypatch, ranks, mode):
    """case f: the table of case a (G = 1 mod 4) on 2 and 3 ranks, cut as the host cuts it (G r / R), directly before and directly after a row of
    2 P + 1 entries, with an empty last slice and (3 ranks) an empty middle one; with 3 ranks also a table of two rows.  Default mode (every rank
    sums its rows' psum, the pieces are gathered in place, every rank adds every class): each rank's n, x1 and diff are the restatement's
    and the one-context result's.  T1K_EM_COLLECTIVE=allreduce (a rank adds its own rows' contributions, the partial sums are added in
    rank order from 0.0): each rank's are em_allreduce_ref(cuts)'s, which differ from the one chain's in some class.  Ranges that leave
    a gap are refused on every rank."""
    P, S = lim
    if mode == "allreduce":
        monkeypatch.setenv("T1K_EM_COLLECTIVE", "allreduce")
    else:
        monkeypatch.delenv("T1K_EM_COLLECTIVE", raising=False)
    ta = er.case_a(P, 1)
    cuts_a = er.cuts_f(ta, P, ranks)
    lens = ta.row_lengths()
    assert cuts_a[0] == [ta.G * r // ranks for r in range(ranks + 1)]
    assert any(lens[c[1]] == 2 * P + 1 for c in cuts_a) and any(lens[c[1] - 1] == 2 * P + 1 for c in cuts_a[1:]), "a cut before and one after a row of 2 P + 1"
    assert any(c[-2] == c[-1] for c in cuts_a) and (ranks == 2 or any(c[1] == c[2] for c in cuts_a)), "an empty last slice, an empty middle one"
    plan = [(ta, cuts_a)]
    if ranks == 3:
        plan.append((er.case_f_small(), [[0, 0, 1, 2]]))
        assert plan[1][0].G == 2 and plan[1][1][0] == [2 * r // 3 for r in range(4)]
    single = []
    for t, _ in plan:   # the one-context result, before any rank thread runs
        u1 = run(ctx, "case f, one context", t)
        single.append((u1, run(ctx, "case f, one context, second update", t, x0=t.ref()[0], want=t.ref(t.ref()[0], "x1"), setup=False)))
    out = sharded(ranks, plan)
    for r in range(ranks):
        res, rc, msg = out[r]
        assert len(res) == sum(len(c) for _, c in plan)
        for k, cuts, u1, u2 in res:
            t = plan[k][0]
            label = "case f, %s, rank %d of %d, cuts %s" % (mode, r, ranks, cuts)
            if mode == "gather":
                want1, want2 = t.ref(), t.ref(t.ref()[0], "x1")
                for got, one in zip((u1, u2), single[k]):
                    assert all(er.same_bits(a, b) for a, b in zip(got, one)), label + ": not the one-context result"
            else:
                want1 = er.em_allreduce_ref(*t.args(), t.x0, cuts)
                want2 = er.em_allreduce_ref(*t.args(), want1[0], cuts)
                if sum(1 for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo) > 1 and t is ta:
                    assert not er.same_bits(want1[1], t.ref()[1]), label + ": the two modes cannot be told apart"
            check(label, u1, want1, t)
            check(label + ", second update", u2, want2, t)
        assert rc == T1K_ERR_ARG and "do not partition" in msg, (r, rc, msg)


def test_f_row_range_errors(ctx, lim):
    """t1k_em_shard refuses row_begin > row_end and row_end > G (no communicator: nothing collective), and the context still updates"""
    P, S = lim
    t = er.case_a(P, 1)
    ctx.em_setup(*t.args())
    assert ctx.em_shard(5, 4, None, raw=True) == T1K_ERR_ARG and "bad row range" in ctx.last_error()
    assert ctx.em_shard(0, t.G + 1, None, raw=True) == T1K_ERR_ARG and "bad row range" in ctx.last_error()
    assert ctx.em_shard(t.G, t.G, None, raw=True) == 0 and ctx.em_shard(0, t.G, None, raw=True) == 0
    run(ctx, "case a after refused row ranges", t, setup=False)
