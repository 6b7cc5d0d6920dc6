"""Designed inputs of the bootstrap tests (test_boot_cpu.py, test_gpu_boot.py; the restatement is boot_ref.py): the counts and replicate
numbers of the resampling tests with a vectorised form of the restatement's draws, the table of the one-update test, a small EM with
classes for the SQUAREM driver, and replicate matrices written by hand for the statistics and the text."""
import functools

import numpy as np

import boot_ref as ref
import em_ref

COUNTS = (1.0, 2.0, 3.0, 63.0, 64.0, 65.0, 1000.0, 0.5, 0.1, 2.5, 3.5, 1e-3)   # n_g 1, 2, 3, 63, 64, 65, 1000, 1, 1, 2, 4, 1
REPLICATES = (2, 63, 64, 65, 128, 129)                                           # B + 1: around one and two blocks of 64 lanes
GROUPS = (1, 5, 300)
SEED = 20240611


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement's draws, many at a time (numpy's uint64 arrays wrap modulo 2^64); test_boot_cpu.py holds it to boot_ref.resample
# ------------------------------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = z + np.uint64(ref.GOLD)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(ref.MUL1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(ref.MUL2)
    return z ^ (z >> np.uint64(31))


def resample_fast(count, B, seed, identity=False):
    """as boot_ref.resample: (k int64 [B + 1][G], c' float64 [B + 1][G])"""
    count = np.asarray(count, np.float64)
    G = len(count)
    ns = np.array([ref.n_of(c) for c in count.tolist()], np.int64)
    k = np.zeros((B + 1, G), np.int64)
    k[0] = ns
    T = np.array(ref.T, np.uint64)
    with np.errstate(over="ignore"):
        rk = _mix(np.uint64(seed) ^ (np.arange(1, B + 1, dtype=np.uint64) * np.uint64(ref.REP)))
        for g in range(G):
            if identity:
                k[1:, g] = ns[g]
                continue
            h = _mix(rk ^ np.uint64(g))
            v = _mix(h[:, None] ^ np.arange(int(ns[g]), dtype=np.uint64)[None, :])
            k[1:, g] = np.searchsorted(T, v.ravel(), side="right").reshape(v.shape).sum(axis=1)
    c = count[None, :] * k.astype(np.float64) / ns.astype(np.float64)[None, :]   # (element-wise: one multiplication, then one division)
    return k, c


def counts_for(G):
    """the counts of COUNTS, each at least once from G = 12 on, in an order that moves with the group index"""
    return np.array([COUNTS[(5 * g + g // 12) % len(COUNTS)] for g in range(G)], np.float64)


@functools.lru_cache(maxsize=None)
def resampled(G, n_rep, identity=False):
    """the shared reference of the resampling tests: (counts, k, c'), computed once and not to be written to"""
    count = counts_for(G)
    k, c = resample_fast(count, n_rep - 1, SEED, identity)
    for a in (count, k, c):
        a.setflags(write=False)
    return count, k, c


# ------------------------------------------------------------------------------------------------------------------------------------
# one update
# ------------------------------------------------------------------------------------------------------------------------------------
UPDATE_G = 300
N_ORDINARY = 40          # the classes with a prescribed size and the two of abundance 0
N_FILLER = 66            # classes only the rows of a prescribed length hold: a row's classes are distinct, so a row of 65 needs them
ROWS = {10: 0, 11: 1, 12: 2, 13: 65}
ZERO_ROW, ZERO_CLASSES = 14, (38, 39)


@functools.lru_cache(maxsize=None)
def update_table(U):
    """G = 300; classes 0 .. 5 of 0, 1, U - 1, U, U + 1 and 2 U + 1 entries, 6 .. 37 of 2 .. 40; rows of 0, 1, 2 and 65 entries; a row of
    two classes whose abundance is 0 (psum == 0 -> 1); the counts of COUNTS"""
    rng = np.random.default_rng(16)
    sized = {0: 0, 1: 1, 2: U - 1, 3: U, 4: U + 1, 5: 2 * U + 1}
    for e in range(6, N_ORDINARY - 2):
        sized[e] = int(rng.integers(2, 41))
    t = em_ref.build(161, UPDATE_G, N_ORDINARY + N_FILLER, sized=sized, row_len=dict(ROWS), fixed={ZERO_ROW: list(ZERO_CLASSES)}, x_fixed={e: 0.0 for e in ZERO_CLASSES})
    t = em_ref.Table(t.rows, t.E, counts_for(UPDATE_G), t.ec_len, t.x0)
    assert t.class_sizes()[:6].tolist() == [0, 1, U - 1, U, U + 1, 2 * U + 1] and all(t.row_lengths()[g] == n for g, n in ROWS.items())
    assert t.rows[ZERO_ROW] == list(ZERO_CLASSES) and set(COUNTS) == set(t.count.tolist())
    return t


@functools.lru_cache(maxsize=None)
def update_x0(U, n_rep):
    """every replicate its own abundances (a lane that reads its neighbour's shows); 0 for the classes of the zero row in all of them"""
    t = update_table(U)
    rng = np.random.default_rng(1600 + n_rep)
    x = np.array([em_ref.draw_x0(rng, t.E, False) for _ in range(n_rep)])
    x[:, list(ZERO_CLASSES)] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def update_want(U, n_rep):
    """em_update_ref of every replicate on its c' (replicate 0: the counts): the shared reference of the update tests"""
    t = update_table(U)
    _, c = resample_fast(t.count, n_rep - 1, SEED)
    x = update_x0(U, n_rep)
    return c, [em_ref.em_update_ref(t.row_ptr, t.ec_idx, c[r], t.ec_len, x[r]) for r in range(n_rep)]


def masks(n_rep):
    """{name: active [B + 1]}: all; only lane 0, 63, 64, the last; one whole block of 64 inactive (where there is more than one block)"""
    out = {"all": np.ones(n_rep, bool)}
    for name, r in (("only 0", 0), ("only 63", 63), ("only 64", 64), ("only the last", n_rep - 1)):
        if r < n_rep:
            out[name] = np.arange(n_rep) == r
    if n_rep > 64:
        out["block 0 inactive"] = np.arange(n_rep) >= 64
        out["block 1 inactive"] = np.arange(n_rep) < 64
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# a small EM with classes, for the SQUAREM driver on the CPU
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_em():
    """40 read groups over 12 classes of 17 alleles in 3 genes and 7 series: (table, boot_ref.Classes).  Two series are rare enough for the
    masking of the 10th round to remove them"""
    rng = np.random.default_rng(5)
    ec = [0, 0, 1, 2, 3, 3, 3, 4, 5, -1, 6, 7, 8, 9, 10, 11, 11]
    series = [0, 0, 0, 1, 2, 2, 1, 3, 3, 3, 4, 4, 5, 5, 6, 6, 6]
    gene = [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    eff = [1000, 990, 1010, 1000, 950, 960, 955, 1200, 1190, 1200, 1210, 1200, 800, 805, 810, 800, 790]
    weight = [1, 2, 1, 1, 1, 1, 3, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1]
    rows = []
    for g in range(40):
        k = int(rng.integers(2, 5))
        pool = [0, 1, 3, 4, 6, 8, 9, 10] if g % 7 else list(range(12))      # classes 2, 5, 7 and 11 are seen by few groups
        rows.append([int(e) for e in rng.choice(pool, size=k, replace=False)])
    count = rng.choice([1.0, 2.0, 0.5, 3.0, 0.1], size=40)
    cl = ref.Classes(ec, eff, weight, series, gene)
    t = em_ref.Table(rows, cl.E, count, cl.ec_len, cl.start())
    return t, cl


# ------------------------------------------------------------------------------------------------------------------------------------
# replicate matrices written by hand
# ------------------------------------------------------------------------------------------------------------------------------------
GENES = ["G0", "G1", "G2"]
SERIES = ["G0*01", "G0*02", "G0*03", "G1*01", "G1*02", "G2*01"]
ALLELE_SERIES = [0, 0, 1, 2, 3, 4, 4, 5]
ALLELE_GENE = [0, 0, 0, 0, 1, 1, 1, 2]
NAN = float("nan")
MATRIX = [
    [5, 3, 4, 1, 2, 1, 1, 0],            # 0: the data
    [4, 4, 8, 0, 2, 1, 1, 0],            # 1: G0*01 = G0*02 = 8 and G1*01 = G1*02 = 2 (ties: the reference order decides); G0*03 is 0
    [6, 1, 3, 2, 1, 2, 2, 0],            # 2
    [NAN, 1, 1, 1, 1, 1, 1, 1],          # 3: invalid
    [1, 1, 9, 3, 3, 0, 0, 0],            # 4: G1*02 is 0
    [5, 5, 1, 6, 0.5, 1, 1.5, 0],        # 5
    [2, 2, 2, 2, 1, 1, 1, 0],            # 6: G0*02 = G0*03 = 2 behind G0*01
]
# per gene (allele, rank, quality) as selection leaves them: G0 calls G0*01 (two alleles) and G0*03; G1's first call has quality 0, so its
# series is printed in both fields; G2 has no call
SELECTED = [[(0, 0, 60), (1, 0, 60), (3, 1, 45)], [(5, 0, 0), (6, 1, 0)], []]
CALLED = [([0], [2]), ([4], [4]), ([], [])]


class StatCase:
    def __init__(self, valid):
        self.matrix = np.array(MATRIX, np.float64)
        self.valid = [bool(v) for v in valid]
        self.series, self.gene, self.selected, self.called = ALLELE_SERIES, ALLELE_GENE, SELECTED, CALLED
        self.B = len(MATRIX) - 1

    def rows(self):
        return ref.table(self.matrix, self.valid, self.series, self.gene, self.called)

    def text(self):
        return ref.text(self.rows(), GENES, SERIES)

    def situations(self):
        """which of the situations the tests ask for this case holds, worked out from its numbers"""
        cl = ref.Classes([-1] * len(self.series), [1] * len(self.series), [1] * len(self.series), self.series, self.gene)
        out = set()
        live = [r for r in range(1, self.B + 1) if self.valid[r]]
        out.add("V = %d" % len(live) if len(live) < 2 else "V > 1")
        if any(not self.valid[r] for r in range(1, self.B + 1)) and live:
            out.add("an invalid replicate")
        for r in live:
            major = ref.series_sums(cl, self.matrix[r].tolist())[0]
            for g in range(len(GENES)):
                mine = sorted((major[m] for m in range(len(SERIES)) if m in [self.series[a] for a in range(cl.A) if self.gene[a] == g]), reverse=True)
                if len(mine) > 1 and mine[0] > 0 and (mine[0] == mine[1] or (len(mine) > 2 and mine[1] == mine[2] and mine[1] > 0)):
                    out.add("ties in rank")
                if any(v == 0 for v in mine) and any(v > 0 for v in mine):
                    out.add("a zero abundance")
        if any(set(a) & set(b) for a, b in self.called):
            out.add("a series in both slots")
        named = {m for a, b in self.called for m in a + b}
        if any(r[1] not in named and r[10] > 0 for r in self.rows()):
            out.add("an uncalled series with top2 > 0")
        return out


def stat_cases():
    return {"main": StatCase([1, 1, 1, 0, 1, 1, 1]), "one": StatCase([1, 0, 1, 0, 0, 0, 0]), "none": StatCase([1, 0, 0, 0, 0, 0, 0])}


SITUATIONS = {"ties in rank", "a zero abundance", "V = 1", "V = 0", "an invalid replicate", "a series in both slots", "an uncalled series with top2 > 0"}
