"""CPU tests (no GPU) of the expectation test_gpu_em.py holds t1k_em_update to: the Python restatement of Genotyper::EMupdate
(tests/em_ref.py) against the oracle's routine (orc_em_update: the code Oracle::quantify runs, compiled C++) bit for bit on every
table of the GPU file, and against exact arithmetic: math.fsum of a class's contributions differs from the chained sum by no more than
recursive summation allows.  The conditions under which a wrong order changes bits are asserted here too, so that the seeds of the
generators are guarded without a GPU."""
import math

import numpy as np
import pytest

import t1k_amd
import util
import em_ref as er


@pytest.fixture(scope="module")
def lim(built):
    P, S = t1k_amd.em_limits()
    assert P == 64 and S % P == 0 and S >= 2 * P, "one operand per lane of a wavefront; whole pieces per step"
    return P, S


def tables(P, S):
    """(name, table, x0, classes left out of the order condition) of every update the GPU file compares"""
    out = [("a, G = %d mod 4" % m, er.case_a(P, m), None, ()) for m in (1, 2, 3)]
    out.append(("b", er.case_b(P)[0], None, ()))
    for m in (1, 2, 3):
        t = er.case_c(P, S, m)
        x, off = er.zeroed_half(P, S, t)
        out += [("c, E = %d mod 4" % m, t, None, ()), ("c, E = %d mod 4, half the sized classes at 0" % m, t, x, tuple(off))]
    out += [("d, E = %d" % E, er.case_d(E), None, ()) for E in er.SETUP_E]
    out += [("d, one row", er.case_d(300, 1), None, ()), ("d, empty rows", er.case_d(5, 50, True), None, ())]
    t, steps, _ = er.case_e(P, S)
    out += [("e, " + name, t, x, ()) for name, x, _ in steps]
    out.append(("f, two rows", er.case_f_small(), None, ()))
    return out


def test_restatement_equals_the_oracle(lim):
    P, S = lim
    for name, t, x, _ in tables(P, S):
        x = t.x0 if x is None else x
        want = util.Oracle.em_update(*t.args(), x)
        got = er.em_update_ref(*t.args(), x)
        for what, g, w in zip(("x1", "n", "diff"), got, want):
            assert er.same_bits(g, w), "%s: %s differs from the oracle's: %s" % (name, what, er.first_difference(g, w))
    # the sharded forms: one rank holding every row is the update itself; so are ranks that hold one row each of a table whose classes
    # have one entry at most (0.0 + v == v, v + 0.0 == v)
    t = er.case_a(P, 1)
    assert er.same_bits(er.em_partial_ref(*t.args(), t.x0, 0, t.G), t.ref()[1])
    for g, w in zip(er.em_allreduce_ref(*t.args(), t.x0, [0, t.G]), t.ref()):
        assert er.same_bits(g, w)
    one = er.build(9, 3, 7, row_len={1: 0}, fixed={0: [1, 2], 2: [3, 4, 5]})
    for g, w in zip(er.em_allreduce_ref(*one.args(), one.x0, [0, 1, 2, 3]), one.ref()):
        assert er.same_bits(g, w)


def test_chained_sums_against_exact_sums(lim):
    """n_ref[e] is the chain 0.0 + c_1 + ... + c_m of the class's contributions, each formed in double.  Recursive summation of m numbers
    makes m - 1 rounded additions; to first order its error is at most (m - 1) u sum|c_i| with u = 2 ** -53 (Higham, Accuracy and Stability
    of Numerical Algorithms, section 4.2), the higher-order term is covered by the factor 1.01 while m u << 0.01.  math.fsum is exact up to
    its one final rounding, and the difference is taken exactly by fsum too."""
    P, S = lim
    u = 2.0 ** -53
    seen = 0
    for name, t, x, _ in tables(P, S):
        x = t.x0 if x is None else x
        n = er.em_update_ref(*t.args(), x)[1]
        _, class_terms = er.terms(t.row_ptr, t.ec_idx, t.count, x, t.E)
        for e, c in enumerate(class_terms):
            m = len(c)
            assert m * u < 1e-4
            assert er.chain(c) == n[e] or (math.isnan(n[e]) and math.isnan(er.chain(c))), "%s: class %d is not the chain of its contributions" % (name, e)
            if m >= 2 and math.isfinite(n[e]):
                err = abs(math.fsum(c + [-float(n[e])]))
                bound = 1.01 * (m - 1) * u * math.fsum(abs(v) for v in c)
                assert err <= bound, "%s: class %d (%d entries): |exact - chained| = %r above %r" % (name, e, m, err, bound)
                seen += m >= P
    assert seen >= 100


def test_a_wrong_order_would_be_seen(lim):
    """every table: of its rows of at least P - 1 entries and of its classes of at least P entries, at least half get another sum when the
    chain is added backwards (classes set to 0 on purpose are left out: their contributions are zeros)"""
    P, S = lim
    rows_seen = classes_seen = 0
    for name, t, x, skip in tables(P, S):
        rc, rn, cc, cn = er.order_shares(t, t.x0 if x is None else x, P, skip)
        assert 2 * rc >= rn and 2 * cc >= cn, "%s: %d of %d long rows and %d of %d long classes change when added backwards" % (name, rc, rn, cc, cn)
        rows_seen += rn
        classes_seen += cn
    assert rows_seen >= 240 and classes_seen >= 200


def test_the_cases_hold_what_they_are_about(lim):
    P, S = lim
    # b: the rows that cancel do so in row order only, and not when the first piece's sum is dropped
    t, kinds = er.case_b(P)
    row_terms, _ = er.terms(t.row_ptr, t.ec_idx, t.count, t.x0, t.E)
    for g in kinds["cancel"]:
        r = row_terms[g]
        assert len(r) == P + 2 and er.chain(r) == 0.0 and er.chain(r[::-1]) != 0.0 and er.chain(r[P:]) != 0.0
    for k in ("zeros P", "zeros P + 1", "minus zeros", "a, -a"):
        assert all(er.chain(row_terms[g]) == 0.0 for g in kinds[k])
    assert all(math.copysign(1.0, v) < 0 for g in kinds["minus zeros"] for v in row_terms[g])
    assert all(len(row_terms[g]) == P + 1 and not any(row_terms[g][:P]) and er.chain(row_terms[g]) == row_terms[g][P] != 0 for g in kinds["last entry alone"])
    assert all(er.chain(row_terms[g]) < 0 for g in kinds["negative"])
    # e: every extrapolated vector has negative entries, two of the four have entries above 1
    _, steps, x3s = er.case_e(P, S)
    assert len(steps) == 3 * er.SQUAREM_ROUNDS and all(float(x.min()) < 0 for x in x3s) and sum(1 for x in x3s if float(x.max()) > 1) >= 2
    assert float(x3s[1].min()) < -1 and float(x3s[1].max()) > 2
    # f: adding the ranks' partial sums is another sum than the one chain, in some class, for every cut of the case
    ta = er.case_a(P, 1)
    for ranks in (2, 3):
        for cuts in er.cuts_f(ta, P, ranks):
            if len([1 for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]) > 1:
                assert not er.same_bits(er.em_allreduce_ref(*ta.args(), ta.x0, cuts)[1], ta.ref()[1]), cuts
