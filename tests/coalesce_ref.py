"""Genotyper::CoalesceReadAssignments (Genotyper.hpp:841-908) restated in plain Python, and the generators of the synthetic fragments that
test_coalesce_cpu.py and test_gpu_coalesce.py fold with it.

coalesce_ref is the expectation of the read-group table (t1k_rowset_coalesce on the GPU, Genotyper::coalesce on the host): fragment by
fragment, in fragment order, one float32 addition at a time.  It shares no code with either."""
import numpy as np

GROUP_DTYPE = np.dtype([("allele", "<i4"), ("start", "<i4"), ("end", "<i4"), ("weight", "<f4"), ("adjust_weight", "<f4")])


def coalesce_ref(row_counts, rows, order=None):
    """row_counts[F], rows: the fragments' rows in the reference's row order (what Rowset.rows() returns).  order: the fragments in the order
    they are folded (default: ascending).  Returns (group_ptr uint64 [G + 1], entries GROUP_DTYPE, first_fragment uint32 [G]) as
    Rowset.groups() does, and run_length int64 [G]: the fragments folded into each group."""
    row_counts = np.asarray(row_counts, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(row_counts)])
    allele, start, end = (np.ascontiguousarray(rows[f]) for f in ("allele_idx", "start", "end"))
    weight, qual, adjust = (np.ascontiguousarray(rows[f]) for f in ("weight", "qual", "adjust_weight"))
    assert weight.dtype == np.float32 and adjust.dtype == np.float32
    group_of = {}   # sorted allele pattern -> group id (844-860: the pattern is the key)
    groups = []     # [allele, start, end, weight, adjust_weight, first fragment, run length]
    for f in (range(len(row_counts)) if order is None else order):
        lo, hi = off[f], off[f + 1]
        if lo == hi:
            continue  # 846-849: a fragment without a row opens nothing
        by = np.argsort(allele[lo:hi], kind="stable") + lo   # 850-853: the row ordered by allele
        pat = tuple(allele[by].tolist())
        g = group_of.get(pat)
        if g is None:  # first sight: the row becomes the group
            group_of[pat] = len(groups)
            groups.append([allele[by], start[by], end[by], weight[by], adjust[by], f, 1])
            continue
        g = groups[g]
        s, e, ok = start[by], end[by], qual[by] == 1
        lower_start = ok & (s < g[1])       # 891-892
        lower_end = ok & (e < g[2])         # 893-894 (sic): the END is compared, the START is stored
        g[1][lower_start] = s[lower_start]
        g[2][lower_end] = s[lower_end]
        g[3] += weight[by]                  # float32 + float32, one fragment at a time
        g[4] += adjust[by]
        g[6] += 1
    sizes = [len(g[0]) for g in groups]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(ptr[-1]), dtype=GROUP_DTYPE)
    for g, at in zip(groups, ptr[:-1].astype(np.int64)):
        for k, field in enumerate(("allele", "start", "end", "weight", "adjust_weight")):
            ent[field][at:at + len(g[0])] = g[k]
    return ptr, ent, np.array([g[5] for g in groups], dtype=np.uint32), np.array([g[6] for g in groups], dtype=np.int64)


def same_table(a, b):
    """None if two (group_ptr, entries, first_fragment, ...) tables are equal -- weights as 32-bit patterns -- else (what, group, slot) of the
    first difference"""
    if len(a[0]) != len(b[0]):
        return ("nGroups", min(len(a[0]), len(b[0])) - 1, 0)
    for what, x, y in (("group_ptr", a[0], b[0]), ("first_fragment", a[2], b[2])):
        if not np.array_equal(x, y):
            return (what, int(np.nonzero(np.asarray(x) != np.asarray(y))[0][0]), 0)
    names = a[1].dtype.names
    for field, fb in zip(names, b[1].dtype.names):
        x, y = a[1][field], b[1][fb]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            g = int(np.searchsorted(a[0], k, side="right")) - 1
            return (field, g, k - int(a[0][g]))
    return None


# ------------------------------------------------------------------------------------------------------------------
# generators: single-end fragments whose rows are known by construction (every overlap of a list ties the best, so the row is the list)
# ------------------------------------------------------------------------------------------------------------------
READ_LEN = 150
DEN = 319          # read span + allele span + clips of every overlap: 319 .. 324


class Fragments:
    """Single-end fragments for a rowset, in fragment order.  A fragment of group `g` lists the group's alleles in an order of its own; all its
    overlaps have one matchCnt, one allele span and one clip (they tie: the row keeps them all, with one weight), and a start of their own.
      * matchCnt 250 .. 319 from a seeded generator over a denominator of 319 .. 324: similarities spread evenly over the steps of the weight
        function (0.01, 0.1, 0.5, 1 at -s 0.8); every seventh fragment of a group matches fully (no 0.25 adjustment);
      * every third fragment of a group has an N: a tenth of the weight;
      * the allele span is 20 .. 40 or 100 .. 170 and the start anywhere it fits: ends fall below a group's `end` several times along a run,
        with start != end (the order-dependent rule of Genotyper.hpp:893-894), and which fragment's start stays depends on the order;
      * every group draws from a generator of its own (seed, group, salt): the salts are chosen once, on the CPU, so that every group meets
        order_conditions();
      * about every fifth fragment has no row: an empty list, or an overlap across a separator (the row is dropped)."""

    def __init__(self, seed, allele_len=400, separator=(5, 200)):
        self.seed, self.rng = seed, np.random.default_rng(seed)
        self.salts, self.low_last = [], []
        self.allele_len, self.separator = allele_len, separator
        self.patterns, self.runs = [], []      # per group
        self.drawn = []
        self.order = None                      # group of every fragment, -1 / -2 for the two kinds without a row

    def group(self, pattern, run, salt=0, low_last=False):
        """low_last: the run's last fragment ends below every other fragment's start, so the `end` rule fires on the very last row folded (the
        last batch's, however few rows it has): the group's `end` is that fragment's start, and with any other last row it is not"""
        self.salts.append(salt)
        self.low_last.append(low_last)
        pattern = np.asarray(pattern, dtype=np.int32)
        assert len(set(pattern.tolist())) == len(pattern)
        self.patterns.append(pattern)
        self.runs.append(int(run))
        return len(self.patterns) - 1

    def _draw(self, g):
        rng, n, pat = np.random.default_rng([self.seed, g, self.salts[g]]), self.runs[g], self.patterns[g]
        span = np.where(rng.random(n) < 0.5, rng.integers(20, 41, n), rng.integers(100, 171, n))
        low = 60 if self.low_last[g] else 0
        if low:
            span[-1] = 20
        clip = (170 - span) // 2 + rng.integers(0, 3, n)
        den = READ_LEN + span + 2 * clip
        assert den.min() >= DEN and den.max() <= DEN + 5
        match = np.minimum(rng.integers(250, 320, n), den)
        match[6::7] = den[6::7]
        base = low + (rng.random(n) * (self.allele_len - span - 24 - low)).astype(np.int64)
        if low:
            base[-1] = 0   # with the start's jitter of up to 23 the last fragment ends at 42 or below: under every other start
        lists = [rng.permutation(pat) for _ in range(n)]
        return dict(span=span, clip=clip, match=match, base=base, has_n=(np.arange(n) % 3 == 2), lists=lists)

    def interleave(self, empty_every=5, shuffle=True):
        """fixes the fragment order: the fragments of all groups shuffled together, a fragment without a row after about every
        (empty_every - 1)-th"""
        tags = [g for g, n in enumerate(self.runs) for _ in range(n)]
        n_empty = len(tags) // (empty_every - 1) if empty_every else 0
        tags += [-1 - (k & 1) for k in range(n_empty)]
        tags = np.array(tags, dtype=np.int64)
        if shuffle:
            self.rng.shuffle(tags)
        self.order = tags
        self.drawn = [self._draw(g) for g in range(len(self.runs))]
        return self

    def lists(self):
        """(counts uint32 [F], the lists one after the other as a dict of int arrays (the overlap record's fields), has_n uint8 [F])"""
        F = len(self.order)
        seen = [0] * len(self.runs)
        alle, cnt = [], np.zeros(F, dtype=np.int64)
        per = {k: np.zeros(F, dtype=np.int64) for k in ("span", "clip", "match", "base", "has_n")}
        sep_allele, sep_at = self.separator
        for f, g in enumerate(self.order.tolist()):
            if g == -1:
                continue                        # no overlap at all
            if g == -2:                         # one overlap across the separator: assigned, but the row is dropped
                alle.append(np.array([sep_allele], dtype=np.int32))
                cnt[f] = 1
                per["span"][f], per["clip"][f], per["match"][f], per["base"][f] = 100, 35, 280, sep_at - 50
                continue
            d, k = self.drawn[g], seen[g]
            seen[g] += 1
            alle.append(d["lists"][k])
            cnt[f] = len(d["lists"][k])
            for key in per:
                per[key][f] = d[key][k]
        assert seen == self.runs
        seq_idx = np.concatenate(alle).astype(np.int64) if alle else np.zeros(0, dtype=np.int64)
        frag = np.repeat(np.arange(F), cnt)
        rep = {k: np.repeat(v, cnt) for k, v in per.items()}
        jitter = np.where(seq_idx == sep_allele, 0, (seq_idx * 7 + frag * 13) % 24)   # a start of its own for every (fragment, allele)
        start = rep["base"] + jitter
        rec = dict(seq_idx=seq_idx, read_start=np.zeros_like(seq_idx), read_end=np.full_like(seq_idx, READ_LEN - 1), seq_start=start,
                   seq_end=start + rep["span"] - 1, strand=np.ones_like(seq_idx), match_cnt=rep["match"], left_clip=rep["clip"],
                   right_clip=np.zeros_like(seq_idx), relaxed_match_cnt=rep["match"])
        return cnt.astype(np.uint32), rec, per["has_n"].astype(np.uint8)

    def fragments_of(self, g):
        return np.nonzero(self.order == g)[0]


def overlap_lists(rec, alen):
    """the lists of Fragments.lists() as one t1k_amd.OVERLAP_DTYPE array, checked and given its similarities by test_gpu_pair.as_list (every
    list lies on the plus strand, so the whole array passes as one list)"""
    import t1k_amd
    import test_gpu_pair
    l = np.zeros(len(rec["seq_idx"]), dtype=t1k_amd.OVERLAP_DTYPE)
    for k, v in rec.items():
        l[k] = v
    return test_gpu_pair.as_list(l, alen)


def rows_by_oracle(orc, counts, ovl, has_n):
    """(row_counts, rows) of single-end fragments from the oracle's pairing: what the GPU's rowset must hold for the same lists"""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = [orc.pair_rows(ovl[off[f]:off[f + 1]], None, int(has_n[f]))[0] for f in range(len(counts))]
    return np.array([len(r) for r in out], dtype=np.uint32), (np.concatenate(out) if out else np.zeros(0, dtype=ovl.dtype))


def last_row_fires(row_counts, rows, fragments):
    """a low_last group: in every slot the last fragment's end lies below the start of every other fragment of the run"""
    c, r = subset(row_counts, rows, fragments)
    n = int(c[0])
    by = lambda x: x[np.argsort(x["allele_idx"], kind="stable")]
    rest = np.stack([by(r[k * n:(k + 1) * n])["start"] for k in range(len(c) - 1)])
    return bool(np.all(by(r[-n:])["end"] < rest.min(axis=0)))


def subset(row_counts, rows, fragments):
    """(row_counts, rows) of the given fragments, in the given order"""
    row_counts = np.asarray(row_counts, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(row_counts)])
    take = np.concatenate([np.arange(off[f], off[f + 1]) for f in fragments]) if len(fragments) else np.zeros(0, dtype=np.int64)
    return row_counts[fragments], rows[take]


def order_conditions(row_counts, rows, fragments):
    """What makes a wrong fold order or a lost row visible in ONE group's result, from the restatement alone.  fragments: the group's, ascending.
    Returns (reversed order changes the weight bits of some slot, reversed order changes the `end` of some slot, dropping the last fragment
    changes the weight bits of every slot)."""
    c, r = subset(row_counts, rows, fragments)
    fwd = coalesce_ref(c, r)[1]
    rev = coalesce_ref(c, r, order=range(len(c) - 1, -1, -1))[1]
    cut = coalesce_ref(c[:-1], r[:len(r) - int(c[-1])])[1]
    bits = lambda e, f: e[f].view(np.uint32)
    assert len(fwd) == len(rev) == len(cut) == int(c[0])
    return (bool(np.any(bits(fwd, "weight") != bits(rev, "weight")) and np.any(bits(fwd, "adjust_weight") != bits(rev, "adjust_weight"))),
            bool(np.any(fwd["end"] != rev["end"])),
            bool(np.all(bits(fwd, "weight") != bits(cut, "weight")) and np.all(bits(fwd, "adjust_weight") != bits(cut, "adjust_weight"))))


# ------------------------------------------------------------------------------------------------------------------
# the cases (B = rows per batch, L = first run length of the long fold, T = slots per tile); the alleles are 10 .. 7999 of a reference whose
# alleles of that range are 400 bases long and carry no separator (test_gpu_pair.make_reference)
# ------------------------------------------------------------------------------------------------------------------
POOL = (10, 8000)


def _patterns(fr, sizes):
    pool = fr.rng.permutation(np.arange(*POOL))
    assert sum(sizes) <= len(pool)
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [pool[a:b] for a, b in zip(at[:-1], at[1:])]


def case_a_runs(B, L):
    """run lengths of k_co_reduce: no fold; the scalar loop alone (up to 2 B); the first pipelined length 2 B + 1; one, two, ... trips of the
    pipelined loop; scalar tails of 0, 1 and B - 1 rows behind it -- those below L"""
    return [n for n in (1, 2, 3, B, B + 1, 2 * B, 2 * B + 1, 2 * B + 2, 3 * B, 3 * B + 1, 3 * B + 2, 4 * B + 1, 5 * B, 6 * B + 1, 7 * B + 5) if n < L]


# salt of every group whose first draw (salt 0) does not meet order_conditions(), by (case, group): the result of search_salts() below
# (`python tests/coalesce_ref.py` prints it) for B = 16, L = 4096 (case a also at L = 34, and with the exchange test's extra run) and
# T = 64.  Other constants, or another list of runs in a case, need the search again: the tests assert the conditions on every run.
SALTS = {("a", 2): 4, ("a", 4): 1, ("a", 5): 2, ("a", 6): 1, ("a", 8): 3, ("a", 9): 3, ("a", 11): 1, ("a", 12): 1, ("a", 15): 3,
         ("b", 0): 2, ("b", 2): 5, ("b", 6): 1, ("c", 1): 1,
         ("d", 0): 2, ("d", 3): 1, ("d", 4): 1, ("d", 5): 1, ("d", 6): 3, ("d", 9): 6, ("d", 10): 1, ("d", 11): 3, ("d", 12): 3, ("d", 14): 4,
         ("d", 18): 1, ("d", 24): 1, ("d", 28): 8, ("d", 29): 4}


def _salt(case, g, salts):
    return (SALTS if salts is None else salts).get((case, g), 0)


def case_a(B, L, seed=101, extra=(), salts=None):
    """extra: further run lengths, appended as groups of their own (the exchange test adds a long run)"""
    fr = Fragments(seed)
    runs = case_a_runs(B, L) + list(extra)
    for g, (p, n) in enumerate(zip(_patterns(fr, [3] * len(runs)), runs)):
        fr.group(p, n, _salt("a", g, salts))
    return fr.interleave()


def case_b(B, T, seed=202, salts=None):
    """groups of 2 B + 3 fragments with 1, T - 1, T, T + 1, T + 1, 2 T and 2 T + 1 alleles.  The pattern of T alleles is the first T (by
    allele) of a pattern of T + 1: a strict prefix; the other pattern of T + 1 differs from that one in its last allele only."""
    fr = Fragments(seed)
    p1, pm, px, p2, p3 = _patterns(fr, [1, T - 1, T + 2, 2 * T, 2 * T + 1])
    px = np.sort(px)
    x, x2, prefix = px[:T + 1], np.concatenate([px[:T], px[T + 1:]]), px[:T]
    for g, p in enumerate((p1, pm, prefix, x, x2, p2, p3)):
        fr.group(p, 2 * B + 3, _salt("b", g, salts))
    return fr.interleave()


def case_c_runs(B, L):
    """L - 1 (the last run of k_co_reduce), L (the first of k_co_reduce_long) and runs whose L - 1 + k rows to fold end in batches of
    B - 1, B, B, 8, 1 and 9 rows"""
    return [L - 1, L, L + 1, L + B + 1, L + 2 * B + 9, L + B + 2, L + 2 * B + 10]


def case_c(B, L, T, seed=303, runs=None, salts=None):
    fr = Fragments(seed)
    runs = case_c_runs(B, L) if runs is None else runs
    sizes = [T + 1 if n == L else 3 for n in runs]
    for g, (p, n) in enumerate(zip(_patterns(fr, sizes), runs)):
        fr.group(p, n, _salt("c", g, salts), low_last=n in (L + B + 2, L + 2 * B + 10))   # the runs whose last batch has 1 and 9 rows
    return fr.interleave()


def case_d_runs(B):
    return [2 * B + 2, 2 * B + 3, 3 * B + 1, 4 * B + 1, 4 * B + 2, 8 * B + 1, 8 * B + 2, 9 * B + 1, 12 * B + 7]


def case_d_tail_runs(B):
    """runs whose last batch in k_co_reduce_long has 1, 2, 1 and 6 rows: the `end` rule fires on the last of them (Fragments.group, low_last)"""
    return [2 * B + 2, 2 * B + 3, 4 * B + 2, 12 * B + 7]


def case_d(B, T, seed=404, salts=None):
    fr = Fragments(seed)
    runs = [n for n in case_d_runs(B) for _ in range(3)]
    tails = case_d_tail_runs(B)
    pats = _patterns(fr, [1, T, T + 1] * len(case_d_runs(B)) + [3] * len(tails))
    for g, (p, n) in enumerate(zip(pats, runs + tails)):
        fr.group(p, n, _salt("d", g, salts), low_last=g >= len(runs))
    return fr.interleave()


def long_batches(run, B):
    """batches of k_co_reduce_long for a run: (their number, the rows of the last one)"""
    total = run - 1
    n = (total + B - 1) // B
    return n, total - (n - 1) * B


def short_trace(run, B):
    """k_co_reduce's way through a run, restated from its loop: (pipelined, trips of the pipelined loop, how it ends, rows left to the scalar loop)"""
    j, j1 = 1, run
    if j + 2 * B > j1:
        return False, 0, None, j1 - j
    j += B
    trips, how = 0, "condition"
    while j + B <= j1:
        more = j + 2 * B <= j1
        trips += 1
        j += B
        if not more:
            how = "break"
            break
    return True, trips, how, j1 - j


def salt_builders(B, L, T):
    """every use the tests make of the cases, as (case, salts -> Fragments): the salts must hold for all of them at once"""
    return [("a", lambda s: case_a(B, L, salts=s)), ("a", lambda s: case_a(B, 2 * B + 2, salts=s)), ("a", lambda s: case_a(B, L, extra=(12 * B + 7,), salts=s)),
            ("b", lambda s: case_b(B, T, salts=s)), ("c", lambda s: case_c(B, L, T, salts=s)), ("c", lambda s: case_c(B, L, T, runs=[L + 1], salts=s)),
            ("d", lambda s: case_d(B, T, salts=s))]


def failing_groups(fr, rc, rows):
    return [g for g, n in enumerate(fr.runs) if n >= 3 and order_conditions(rc, rows, fr.fragments_of(g)) != (True, True, True)]


def search_salts(builders, rows_of, start=None, cap=64):
    """The smallest salts, tried upwards from `start` (default: all 0), with which every group of every builder meets order_conditions().
    rows_of(fragments) -> (row_counts, rows).  Deterministic; gives up when a salt passes `cap`.  A group's salt is shared by the builders
    of its case, so the sweep over the builders repeats until one sweep changes nothing."""
    salts = dict(start or {})
    while True:
        changed = False
        for case, make in builders:
            while True:
                fr = make(salts)
                bad = failing_groups(fr, *rows_of(fr))
                if not bad:
                    break
                changed = True
                for g in bad:
                    salts[(case, g)] = salts.get((case, g), 0) + 1
                    assert salts[(case, g)] <= cap, "no salt up to %d makes group %d of case %s show a wrong fold order" % (cap, g, case)
        if not changed:
            return {k: v for k, v in sorted(salts.items()) if v}


if __name__ == "__main__":  # the search behind SALTS (CPU only): python tests/coalesce_ref.py
    import os
    import sys
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import t1k_amd
    import test_gpu_pair
    import util
    fasta = os.path.join(tempfile.mkdtemp(), "ref.fa")
    alen = test_gpu_pair.make_reference(fasta)
    orc = util.Oracle(fasta, similarity=0.8, relax=False, max_assign=0)

    def rows_of(fr):
        counts, rec, has_n = fr.lists()
        return rows_by_oracle(orc, counts, overlap_lists(rec, alen), has_n)
    B, L, T = t1k_amd.coalesce_limits()
    found = search_salts(salt_builders(B, max(L, 4096), T), rows_of)
    print("SALTS =", found)
    print("as committed" if found == SALTS else "differs from the committed table")
