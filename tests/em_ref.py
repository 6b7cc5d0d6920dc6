"""A plain restatement of Genotyper::EMupdate (Genotyper.hpp:372-421) and the tables test_em_cpu.py and test_gpu_em.py run it on.

Every sum here is a chain of Python floats (IEEE doubles) added one after the other in the reference's order: psum over a read group's
entries in row order (psum == 0 -> 1), ecReadCount[ec] += count[g] * (x0[ec] / psum) over the groups in group order, then norm, x1 and
diff over the classes in class order.  numpy is used for element-wise operations only (one correctly rounded operation per element); no
np.sum, no np.add.reduce: they re-associate.

The tables come from prescribed class sizes and prescribed row lengths (build): class e is given to s_e distinct rows, rows of a
prescribed length are filled up with classes that no size is prescribed for, every row's entries are shuffled (the row order is the order
of the psum chain; a class's entries follow the rows' order).  P and S below are the two step sizes t1k_em_limits reports: entries per
ordered piece and entries per step of the class pass."""
import functools
import math

import numpy as np

COUNTS = (1.0, 0.5, 0.1, 37.5, 1200.25, 3.0, 7.0, 1e-3, 1e6)   # read counts with mantissas of one bit and of many


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def _lists(row_ptr, ec_idx, count, x0):
    return [int(v) for v in row_ptr], np.asarray(ec_idx).tolist(), np.asarray(count, np.float64).tolist(), np.asarray(x0, np.float64).tolist()


def e_step(row_ptr, ec_idx, count, x0, n_ec, row_lo=0, row_hi=None):
    """ecReadCount after the rows [row_lo, row_hi) (Genotyper.hpp:378-404), a list of n_ec floats"""
    rp, ei, c, x = _lists(row_ptr, ec_idx, count, x0)
    n = [0.0] * n_ec
    for g in range(row_lo, len(c) if row_hi is None else row_hi):
        r = ei[rp[g]:rp[g + 1]]
        psum = 0.0
        for e in r:
            psum += x[e]
        if psum == 0:
            psum = 1.0
        cg = c[g]
        for e in r:
            n[e] += cg * (x[e] / psum)
    return n


def m_step(n, ec_len, x0):
    """Genotyper.hpp:406-420: (x1, n, diff) from the expected read counts"""
    n = np.asarray(n, np.float64)
    x0 = np.asarray(x0, np.float64)
    with np.errstate(all="ignore"):   # (a table without entries: 0 / 0, as the reference computes it)
        q = n / np.asarray(ec_len).astype(np.float64)
        norm = 0.0
        for v in q.tolist():
            norm += v
        x1 = q / np.float64(norm)
        diff = 0.0
        for v in np.abs(x1 - x0).tolist():
            diff += v
    return x1, n, diff


def em_update_ref(row_ptr, ec_idx, count, ec_len, x0):
    """one Genotyper::EMupdate: (x1, n, diff)"""
    return m_step(e_step(row_ptr, ec_idx, count, x0, len(ec_len)), ec_len, x0)


def em_partial_ref(row_ptr, ec_idx, count, ec_len, x0, row_lo, row_hi):
    """the expected read counts of the rows [row_lo, row_hi) alone: what one rank adds up with T1K_EM_COLLECTIVE=allreduce"""
    return e_step(row_ptr, ec_idx, count, x0, len(ec_len), row_lo, row_hi)


def em_allreduce_ref(row_ptr, ec_idx, count, ec_len, x0, cuts):
    """rank r holds the rows [cuts[r], cuts[r + 1]); the ranks' partial counts are added in rank order starting from 0.0, then the M-step"""
    total = [0.0] * len(ec_len)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = em_partial_ref(row_ptr, ec_idx, count, ec_len, x0, lo, hi)
        for e, v in enumerate(part):
            total[e] += v
    return m_step(total, ec_len, x0)


def squarem_x3(x0, x1, x2):
    """the extrapolated vector of one SQUAREM round (Genotyper.hpp:424-437 and the loop around it; no lower limit on alpha) and alpha"""
    r = x1 - x0
    v = x2 - 2 * x1 + x0
    r2 = v2 = 0.0
    for a in (r * r).tolist():
        r2 += a
    for a in (v * v).tolist():
        v2 += a
    alpha = -1.0 if v2 == 0 else -math.sqrt(r2) / math.sqrt(v2)
    return x0 - 2 * alpha * r + alpha * alpha * v, alpha


def chain(values, start=0.0):
    s = start
    for v in values:
        s += v
    return s


def terms(row_ptr, ec_idx, count, x0, n_ec):
    """(the abundances of every row in row order, the contributions of every class in group order): the operands of the two kinds of chain"""
    rp, ei, c, x = _lists(row_ptr, ec_idx, count, x0)
    row_terms, class_terms = [], [[] for _ in range(n_ec)]
    for g in range(len(c)):
        r = ei[rp[g]:rp[g + 1]]
        row_terms.append([x[e] for e in r])
        psum = chain(row_terms[-1])
        if psum == 0:
            psum = 1.0
        for e in r:
            class_terms[e].append(c[g] * (x[e] / psum))
    return row_terms, class_terms


def order_shares(t, x0, P, skip_classes=()):
    """how many of the rows of at least P - 1 entries, and of the classes of at least P entries, get another sum when their chain is added
    backwards: (rows changed, rows, classes changed, classes)"""
    row_terms, class_terms = terms(t.row_ptr, t.ec_idx, t.count, x0, t.E)
    rows = [r for r in row_terms if len(r) >= P - 1]
    classes = [c for e, c in enumerate(class_terms) if len(c) >= P and e not in skip_classes]
    changed = lambda ls: sum(1 for l in ls if chain(l) != chain(l[::-1]))
    return changed(rows), len(rows), changed(classes), len(classes)


def same_bits(got, want):
    """bit for bit; NaN where the restatement has NaN"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all()) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def first_difference(got, want):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    bad = np.flatnonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))
    return None if len(bad) == 0 else (int(bad[0]), float(got[bad[0]]), float(want[bad[0]]), len(bad))


# ------------------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, rows, n_ec, count, ec_len, x0):
        self.rows = rows
        self.G, self.E = len(rows), n_ec
        self.row_ptr = np.zeros(self.G + 1, np.uint64)
        self.row_ptr[1:] = np.cumsum([len(r) for r in rows])
        self.ec_idx = np.array([e for r in rows for e in r], dtype=np.uint32)
        self.count = np.asarray(count, np.float64)
        self.ec_len = np.asarray(ec_len, np.int32)
        self.x0 = np.asarray(x0, np.float64)
        assert len(self.count) == self.G and len(self.ec_len) == n_ec and len(self.x0) == n_ec
        assert all(len(set(r)) == len(r) for r in rows) and (len(self.ec_idx) == 0 or int(self.ec_idx.max()) < n_ec)
        self._ref = {}

    def args(self):
        return self.row_ptr, self.ec_idx, self.count, self.ec_len

    def row_lengths(self):
        return np.diff(self.row_ptr.astype(np.int64))

    def class_sizes(self):
        return np.bincount(self.ec_idx, minlength=self.E)

    def ref(self, x0=None, key="x0"):
        """em_update_ref of the table (on its own x0, or on another vector under a key of its own), computed once"""
        if key not in self._ref:
            self._ref[key] = em_update_ref(*self.args(), self.x0 if x0 is None else x0)
        return self._ref[key]


def draw_x0(rng, n, signed):
    x = 10.0 ** rng.uniform(-9, 0, n)
    if signed:
        x[rng.random(n) < 0.25] *= -1.0
    return x


def build(seed, G, E, sized=None, row_len=None, fixed=None, signed=False, x_fixed=None):
    """sized: {class: rows it is given to}; row_len: {row: entries} (filled up with the classes that are neither sized nor used by a
    fixed row); fixed: {row: its classes in the order given -- neither filled up nor shuffled}; x_fixed: {class: its x0}"""
    rng = np.random.default_rng(seed)
    sized, row_len, fixed, x_fixed = sized or {}, row_len or {}, fixed or {}, x_fixed or {}
    rows = [[] for _ in range(G)]
    free = np.array([g for g in range(G) if g not in row_len and g not in fixed], dtype=np.int64)
    for e, s in sized.items():
        assert s <= len(free), "class %d: %d rows wanted, %d free" % (e, s, len(free))
        for g in rng.choice(free, size=s, replace=False).tolist():
            rows[g].append(e)
    taken = set(sized) | {e for r in fixed.values() for e in r}
    filler = np.array([e for e in range(E) if e not in taken], dtype=np.int64)
    for g, n in row_len.items():
        need = n - len(rows[g])
        assert 0 <= need <= len(filler), "row %d: %d entries wanted, %d there, %d classes to fill with" % (g, n, len(rows[g]), len(filler))
        if need:
            rows[g] += rng.choice(filler, size=need, replace=False).tolist()
    for g in range(G):
        rows[g] = [int(e) for e in rng.permutation(rows[g])] if rows[g] else []
    for g, r in fixed.items():
        rows[g] = [int(e) for e in r]
    x0 = draw_x0(rng, E, signed)
    for e, v in x_fixed.items():
        x0[e] = v
    return Table(rows, E, rng.choice(COUNTS, size=G), rng.integers(900, 1300, size=E), x0)


def long_row_lengths(P):
    return [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P - 1, 3 * P, 3 * P + 1, 4 * P + 44]


@functools.lru_cache(maxsize=None)
def case_a(P, g_mod, signed=False):
    """eight rows of each length of long_row_lengths among about 500 rows of 1 .. 11 entries; the table's last rows are one of each
    length, the longest last; G = g_mod mod 4"""
    lens = long_row_lengths(P)
    G = 8 * len(lens) + 500
    G += (g_mod - G) % 4
    E = 4 * P + 44 + 113
    rng = np.random.default_rng(1000 + g_mod)
    tail = list(range(G - len(lens), G))
    spots = rng.choice(G - len(lens), size=7 * len(lens), replace=False).tolist()
    row_len = {g: int(rng.integers(1, 12)) for g in range(G)}
    for k, n in enumerate(lens):
        row_len[tail[k]] = n
        for g in spots[7 * k:7 * k + 7]:
            row_len[g] = n
    t = build(2000 + g_mod, G, E, row_len=row_len, signed=signed)
    assert t.G % 4 == g_mod and t.E >= 4 * P + 44 and t.row_lengths().tolist() == [row_len[g] for g in range(G)]
    return t


@functools.lru_cache(maxsize=None)
def case_b(P):
    """rows that cancel, rows of zeros and negative row sums among 200 ordinary signed rows of 1 .. 11 entries and 12 ordinary signed rows of
    P, P + 1 and 2 P + 1 entries.  Returns (table, {kind: rows})"""
    rng = np.random.default_rng(77)
    n_cancel = 4
    zeros = list(range(P + 1))                                  # classes whose x0 is 0.0, every third one -0.0
    minus = list(range(P + 1, P + 5))                           # classes whose x0 is -0.0
    solo = [P + 5, P + 6]                                       # the one entry that is not zero in a row of P + 1
    pair = [P + 7, P + 8, P + 9, P + 10]                        # a, -a, b, -b
    neg = list(range(P + 11, P + 11 + 5))                       # negative abundances: rows of these alone sum below zero
    cancel = [list(range(P + 16 + k * (P + 2), P + 16 + (k + 1) * (P + 2))) for k in range(n_cancel)]
    first_free = P + 16 + n_cancel * (P + 2)
    E = first_free + 2 * P + 1 + 90
    x_fixed = {e: (-0.0 if k % 3 == 2 else 0.0) for k, e in enumerate(zeros)}
    x_fixed.update({e: -0.0 for e in minus})
    x_fixed.update({solo[0]: 0.3718281828, solo[1]: -2.5e-7})
    a, b = 0.1234567891234, 7.7e-5 / 3
    x_fixed.update({pair[0]: a, pair[1]: -a, pair[2]: -b, pair[3]: b})
    x_fixed.update({e: -(10.0 ** rng.uniform(-6, 0)) for e in neg})
    for cl in cancel:   # P + 1 signed abundances and the negative of their ordered sum: the row's chain ends in exactly 0.0
        while True:
            v = draw_x0(rng, P + 1, True).tolist()
            s = chain(v)
            if s != 0 and chain([-s] + v[::-1]) != 0 and chain(v[P:] + [-s]) != 0:   # backwards, and with the carry of the first piece lost
                break
        x_fixed.update(dict(zip(cl, v + [-s])))
    G = 200 + 12 + 17
    G += (1 - G) % 4
    special = rng.choice(G - 1, size=16, replace=False).tolist() + [G - 1]
    kinds = {"zeros P": [special[0]], "zeros P + 1": [special[1]], "minus zeros": [special[2]], "last entry alone": special[3:5], "a, -a": special[5:7],
             "negative": special[7:9], "cancel": special[9:9 + n_cancel - 1] + [G - 1], "zeros then a short row": [special[12]]}
    fixed = {special[0]: zeros[:P], special[1]: zeros, special[2]: minus, special[3]: zeros[:P] + [solo[0]], special[4]: zeros[1:P + 1] + [solo[1]],
             special[5]: pair[:2], special[6]: pair[2:], special[7]: neg, special[8]: neg[3:] + neg[:2], special[12]: zeros[:3]}
    for g, cl in zip(kinds["cancel"], cancel):
        fixed[g] = cl
    others = [g for g in range(G) if g not in fixed]
    long_rows = rng.choice(others, size=12, replace=False).tolist()
    row_len = {g: int(rng.integers(1, 12)) for g in others}
    for k, g in enumerate(long_rows):
        row_len[g] = (P, P + 1, 2 * P + 1)[k % 3]
    t = build(78, G, E, row_len=row_len, fixed=fixed, signed=True, x_fixed=x_fixed)
    assert t.E - len({e for r in fixed.values() for e in r}) >= 2 * P + 1
    return t, kinds


def class_sizes_c(P, S):
    return [0, 1, P - 1, P, P + 1, S - P - 1, S - P, S - P + 1, S - 1, S, S + 1, S + P - 1, S + P, S + P + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S - 1, 3 * S,
            3 * S + 1, 3 * S + P, 4 * S + 1]


@functools.lru_cache(maxsize=None)
def case_c(P, S, e_mod, signed=False):
    """the sizes of class_sizes_c as the first and as the last classes of the table, one class of 10 S + 37 rows and a few of 2 .. 40 between
    them; E = e_mod mod 4; G just above the largest class; no prescribed row: every row holds the classes that drew it"""
    sizes = class_sizes_c(P, S)
    big = 10 * S + 37
    mid = 6 + (e_mod - (2 * len(sizes) + 1 + 6)) % 4
    E = 2 * len(sizes) + 1 + mid
    G = big + 43
    rng = np.random.default_rng(3000 + e_mod)
    sized = {k: s for k, s in enumerate(sizes)}
    sized[len(sizes)] = big
    for k in range(mid):
        sized[len(sizes) + 1 + k] = int(rng.integers(2, 41))
    for k, s in enumerate(sizes):
        sized[E - len(sizes) + k] = s
    t = build(4000 + e_mod, G, E, sized=sized, signed=signed)
    assert t.E % 4 == e_mod and t.class_sizes().tolist() == [sized[e] for e in range(E)] and int(t.row_lengths().max()) < P
    return t


def sized_classes_c(P, S, t):
    k = len(class_sizes_c(P, S))
    return list(range(k)) + list(range(t.E - k, t.E))


def zeroed_half(P, S, t):
    """the table's x0 with 0.0 for every other sized class"""
    x = t.x0.copy()
    off = sized_classes_c(P, S, t)[1::2]
    x[off] = 0.0
    return x, off


SETUP_E = (65536, 1, 65537, 2, 255, 65535, 256, 257)   # the order of the setups on one context: large, small, large, ...


@functools.lru_cache(maxsize=None)
def case_d(E, G=3000, empty=False):
    """G rows of 1 .. 40 distinct classes out of E (of none when `empty`)"""
    rng = np.random.default_rng(5000 + E + 7 * G)
    row_len = {g: 0 if empty else int(rng.integers(1, min(40, E) + 1)) for g in range(G)}
    return build(6000 + E + 7 * G, G, E, row_len=row_len)


def sort_bits(E):
    bits = 1
    while (1 << bits) < E:
        bits += 1
    return bits


SQUAREM_ROUNDS = 4
SQUAREM_SEED = 5   # (of the seeds 0 .. 11 the one whose second extrapolation reaches furthest: alpha -16, x3 from -3.0 to 6.3; test_em_cpu.py asserts it)


@functools.lru_cache(maxsize=None)
def case_e(P, S):
    """the table of case c (E = 1 mod 4) and the vectors of four SQUAREM rounds of the restatement on it: a list of (name, x fed to the
    update, (x1, n, diff) of the restatement), three updates a round, and the four extrapolated vectors"""
    t = case_c(P, S, 1)
    x0 = squarem_start(t)
    steps, x3s = [], []
    for k in range(SQUAREM_ROUNDS):
        r1 = em_update_ref(*t.args(), x0)
        r2 = em_update_ref(*t.args(), r1[0])
        x3, alpha = squarem_x3(x0, r1[0], r2[0])
        r3 = em_update_ref(*t.args(), x3)
        steps += [("round %d, x0 -> x1" % k, x0, r1), ("round %d, x1 -> x2" % k, r1[0], r2), ("round %d, x3 -> x1 (alpha %r)" % (k, alpha), x3, r3)]
        x3s.append(x3)
        x0 = r3[0]
    return t, steps, x3s


def squarem_start(t):
    """the start of case e: abundances of 10 ** uniform(-9, 0), as the tables' own x0 (positive: what the first update of a job gets)"""
    return draw_x0(np.random.default_rng(7000 + SQUAREM_SEED), t.E, False)


@functools.lru_cache(maxsize=None)
def case_f_small():
    """two read groups for three ranks"""
    return build(81, 2, 5, row_len={0: 3, 1: 4})


def cuts_f(t, P, ranks):
    """the row ranges of case f on the table of case a: as the host cuts them (G r / R); a cut directly before and directly after a row of
    2 P + 1 entries; an empty last slice; with three ranks an empty middle slice too"""
    G = t.G
    lens = t.row_lengths()
    g = int(np.flatnonzero(lens == 2 * P + 1)[3])
    assert 0 < g < G - 1
    host = [G * r // ranks for r in range(ranks + 1)]
    if ranks == 2:
        return [host, [0, g, G], [0, g + 1, G], [0, G, G]]
    assert ranks == 3
    return [host, [0, g, g + 1, G], [0, g, g, G], [0, g + 1, G, G]]
