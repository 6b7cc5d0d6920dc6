"""k_pair's join through the LDS table indexed by allele offset (the "direct" route), against the oracle (pytest -m gpu).

Same method as test_gpu_pair.py, whose helpers are used here: lists made by the host on a hand-made reference (a copy of its own, a few more
alleles than the direct table has words), uploaded, paired on the GPU, every fragment compared with util.Oracle.pair_rows on the very lists
the kernel read.  Every group derives from its inputs alone -- allele range, list lengths, repeated alleles, the limits the library reports --
which route each fragment must take, and asserts it.

The route serves the fragments whose two lists together exceed the hash table's capacity (shorter ones keep the hash table whatever their
range); the library reads T1K_PAIR_DIRECT once per process, 0 turns the route off.  test_direct_off_in_a_child_process runs the groups again in a process where it is 0: the same oracle rows, the same coalesced read groups
(which the pattern hashes decide) then come from the two old routes."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import t1k_amd
import util
import test_gpu_pair as tp
from test_gpu_pair import ov, mates, as_list, run, compare, N_ALLELES, SHORT, SEPS

pytestmark = pytest.mark.gpu

DIRECT = 0 if os.environ.get("T1K_PAIR_DIRECT") == "0" else 1  # as t1k_pair.hip reads it
PLAIN = [a for a in range(N_ALLELES) if a not in SHORT and a not in SEPS]  # alleles of full length without a separator


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = tp.World(str(tmp_path_factory.mktemp("pair_direct")))
    w.cap = t1k_amd.pair_direct_cap()
    assert w.cap == 2 * w.slots and w.cap <= 32766 and w.cap + 3 + 10 < N_ALLELES, "the reference no longer has more alleles than the direct table has words"
    yield w
    w.close()


def span(l1, l2):
    a = l1["seq_idx"].tolist() + ([] if l2 is None else l2["seq_idx"].tolist())
    return (max(a) - min(a) + 1) if a else 0


def route(w, l1, l2):
    """the join table a fragment must end on, the launch that pairs it, and whether it is replayed -- from its lists and the limits alone
    (t1k_pair.hip: the range sweep, the route choice, the duplicate test, the hand-over to the second launch)"""
    n1, n2 = len(l1), 0 if l2 is None else len(l2)
    dup = len(set(l1["seq_idx"].tolist())) < n1 or (l2 is not None and len(set(l2["seq_idx"].tolist())) < n2)
    rg = span(l1, l2)
    fits = n1 + n2 > 0 and rg <= w.cap and n1 <= rg and n2 <= rg
    tried = fits and DIRECT == 1 and n1 + n2 > w.lj_cap
    r = {"second-launch" if n1 + n2 > w.frag_cap else "first-launch"}
    if dup:
        r |= {"hbm", "replay"}
        if tried:
            r.add("direct-left")  # the repeated allele was found while the direct table was filled
    else:
        r.add("direct" if tried else "hash" if n1 + n2 <= w.lj_cap else "hbm")
    return r


def routes(w, frags):
    out = set()
    for l1, l2 in frags:
        out |= route(w, l1, l2)
    return out


def long_direct():
    """what a fragment beyond the hash table's capacity with a fitting range is joined through in this process"""
    return "direct" if DIRECT else "hbm"


def short_direct():
    """... and one within it, whatever its range"""
    return "hash"


def window(rng, lo, width, n1, n2, min_in=3, max_in=3, best_every=97, strand1=None):
    """lists of n1 / n2 distinct plain alleles inside [lo, lo + width), about half of the shorter list's alleles in both; the smallest allele lo is in
    list min_in and the largest lo + width - 1 in list max_in (1, 2, or 3 = both: then it is a tie at the best fragment); matchCnt as
    test_gpu_pair.random_fragment draws them (best_every = 0: no inner allele reaches the best)"""
    top = lo + width - 1
    assert lo in PLAIN and top in PLAIN
    inner = [a for a in PLAIN if lo < a < top]
    rng.shuffle(inner)
    ends = [lo] if width == 1 else [lo, top]
    where = {lo: min_in, top: max_in} if width > 1 else {lo: min_in | max_in}
    e1 = [a for a in ends if where[a] & 1]
    e2 = [a for a in ends if where[a] & 2]
    k1, k2 = n1 - len(e1), n2 - len(e2)
    assert k1 >= 0 and k2 >= 0
    common = min(k1, k2) // 2 if min(k1, k2) > 1 else min(k1, k2)
    common = max(common, k1 + k2 - len(inner))
    assert 0 <= common <= min(k1, k2)
    a1 = inner[:k1]
    a2 = inner[:common] + inner[k1:k1 + k2 - common]
    assert len(a2) == k2
    strand1 = rng.choice((1, -1)) if strand1 is None else strand1
    m = {}
    for k, a in enumerate(inner[:common]):
        m[a] = (300, 300) if best_every and k % best_every == 0 else (rng.choice((280, 288, 294, 296)), rng.choice((280, 290, 296)))
    for a in ends:
        if where[a] == 3:
            m[a] = (300, 300)
    lo_s, hi_s = (50, 200) if strand1 == 1 else (200, 50)
    l1 = [ov(a, lo_s + rng.randrange(3), strand1, m[a][0] if a in m else rng.choice((280, 296, 300))) for a in a1 + e1]
    l2 = [ov(a, (hi_s if (rng.random() < 0.9 or a in ends) else lo_s) + rng.randrange(3), -strand1, m[a][1] if a in m else rng.choice((280, 296, 300))) for a in a2 + e2]
    rng.shuffle(l1)
    rng.shuffle(l2)
    return l1, l2


def test_range_at_the_capacity(world):
    """case 1: allele ranges of DIRECT_CAP - 1, DIRECT_CAP and DIRECT_CAP + 1, each with short lists and with lists beyond the hash table; a range of
    1; lists of one record"""
    w, rng = world, random.Random(101)
    c, lj = w.cap, w.lj_cap
    frags, want = [], []
    for width in (c - 1, c, c + 1):
        fit = width <= c
        frags.append(window(rng, 10, width, 30, 40))                     # short
        want.append(short_direct() if fit else "hash")
        frags.append(window(rng, 10, width, lj // 2 + 1, lj - lj // 2))  # LJ_CAP + 1
        want.append(long_direct() if fit else "hbm")
        frags.append(window(rng, 10, width, 1, 1, min_in=1, max_in=2))   # one record each, nothing joins
        want.append(short_direct() if fit else "hash")
        frags.append(window(rng, 10, width, 2, 2))                       # both ends in both lists
        want.append(short_direct() if fit else "hash")
    frags.append(mates([4000], 300, 300))                                # range 1
    want.append(short_direct())
    frags.append(([ov(4000, 50, 1, 300)], [ov(4001, 200, -1, 300)]))     # range 2, no join
    want.append(short_direct())
    frags.append(mates([10, 10 + c - 1], 300, 300))                      # two records at the two ends of the table
    want.append(short_direct())
    done, rows, flags = run(w, "range at the capacity", frags)
    assert [span(a, b) for a, b in done[:12:4]] == [c - 1, c, c + 1]
    for k, ((l1, l2), r) in enumerate(zip(done, want)):
        assert r in route(w, l1, l2), (k, r, route(w, l1, l2))
    assert len(rows[-1]) == 2 and len(rows[-3]) == 1 and flags[-1] and flags[-3]
    assert routes(w, done) >= {"hash", "hbm"} and (not DIRECT or "direct" in routes(w, done))
    run(w, "range at the capacity, single-end", frags, single=True)


def test_bounds_from_both_lists(world):
    """case 2: the smallest allele only in list 1 and the largest only in list 2, the other way round, and both in both lists -- where the two ends of
    the table carry the best fragment (a tie, both kept) -- for short lists and for lists beyond the hash table, at several bases and widths"""
    w, rng = world, random.Random(102)
    lj = w.lj_cap
    frags, ends = [], []
    for lo, width in ((10, w.cap), (10, 700), (2100, 3001), (8101, 150)):
        for min_in in (1, 2, 3):
            for max_in in (1, 2, 3):
                n = (30, 40) if width < lj else (lj // 2 + 3, lj // 2 + 4)
                n = (min(n[0], width // 2), min(n[1], width // 2))
                frags.append(window(rng, lo, width, n[0], n[1], min_in, max_in, best_every=0))
                ends.append((lo, lo + width - 1, min_in, max_in))
    done, rows, flags = run(w, "bounds from both lists", frags)
    for (l1, l2), r, (lo, top, min_in, max_in) in zip(done, rows, ends):
        assert min(l1["seq_idx"].min(), l2["seq_idx"].min()) == lo and max(l1["seq_idx"].max(), l2["seq_idx"].max()) == top
        assert (lo in l1["seq_idx"]) == bool(min_in & 1) and (lo in l2["seq_idx"]) == bool(min_in & 2)
        assert (top in l1["seq_idx"]) == bool(max_in & 1) and (top in l2["seq_idx"]) == bool(max_in & 2)
        kept = set(r["allele_idx"].tolist())
        # an end that is in both lists is the only 300 + 300 fragment (no inner allele reaches it): it is kept, and nothing else unless the other end ties
        if min_in == 3 or max_in == 3:
            assert kept == set([lo] * (min_in == 3) + [top] * (max_in == 3)), (lo, top, min_in, max_in, sorted(kept))
    got = routes(w, done)
    assert short_direct() in got and long_direct() in got and "replay" not in got
    run(w, "bounds from both lists, relaxed", frags, relax=1)


def test_long_lists_that_left_hbm(world):
    """case 3: both lists together of LJ_CAP + 1, fragCap and fragCap + 1 (the second launch) records inside a range that fits.  Several joined
    fragments share the best (matchCnt, similarity) at list-1 indices i, i + 1 and i + one round of the streamed passes (the same lane's next
    trip); with --relaxIntronAlign the first in order decides through its relaxedMatchCnt which near-best fragments stay (as
    test_gpu_pair.test_ties_first_in_order does on short lists)"""
    w, rng = world, random.Random(103)
    frags, firsts = [], []
    for tot in (w.lj_cap + 1, w.frag_cap, w.frag_cap + 1):
        n2 = tot // 2
        n1 = tot - n2
        assert n1 <= w.cap and n1 > w.round + 201
        for i in (0, 63, 200):
            at = [i, i + 1, i + w.round]
            for lead in range(len(at)):
                ties = at[lead:]
                pool = PLAIN[20:20 + n1 + 40]
                rng.shuffle(pool)
                al = pool[:n1]
                m1, m2, r1, r2 = [290] * n1, [290] * n1, [300] * n1, [300] * n1
                near = [q for q in range(n2) if q not in ties]
                rng.shuffle(near)
                for k, t in enumerate(ties):
                    m1[t], m2[t] = 300, 298
                    r1[t], r2[t] = 310 + k, 305
                    for q in near[3 * k:3 * k + 3]:
                        m1[q], m2[q] = 298, 298
                        r1[q], r2[q] = 310 + k, 305
                l1, l2 = mates(al, m1, m2, r1=r1, r2=r2, strand1=rng.choice((1, -1)))
                l2 = l2[:n2]       # (the ties and their near-best fragments lie below n2: they keep their mates)
                rng.shuffle(l2)
                frags.append((l1, l2))
                firsts.append(ties[0])
    done, rows, flags = run(w, "long lists in a narrow range", frags, relax=1)
    sizes = sorted(set(len(a) + len(b) for a, b in done))
    assert sizes == [w.lj_cap + 1, w.frag_cap, w.frag_cap + 1] and all(span(a, b) <= w.cap for a, b in done)
    assert routes(w, done) == {"first-launch", "second-launch", long_direct()} and all(flags)
    for (l1, _), r, first in zip(done, rows, firsts):
        kept = set(r["allele_idx"].tolist())
        assert l1["seq_idx"][first] in kept and len(r) >= 4
        assert [a for a in l1["seq_idx"].tolist() if a in kept] == r["allele_idx"].tolist()


def test_repeated_allele_on_the_direct_route(world):
    """case 4: an allele twice in list 1, in list 2, in both, among short lists and among lists beyond the hash table, all inside a range that fits:
    found while the direct table is filled, the fragment is replayed on the HBM tables.  The call's pair_overlaps counts every record once."""
    w, rng = world, random.Random(104)
    frags = []
    for big in (0, 40, w.lj_cap + 10):
        for rep1, rep2 in ((2, 1), (1, 2), (2, 2), (3, 1), (1, 3)):
            l1, l2 = window(rng, 3000, 4000, big // 2, big - big // 2) if big else ([], [])
            strand1 = l1[0][5] if l1 else rng.choice((1, -1))
            used = set(r[0] for r in l1 + l2)
            x = next(a for a in range(3500, 6900) if a not in used)
            lo, hi = (40, 190) if strand1 == 1 else (190, 40)
            l1 += [ov(x, lo + 4 * k, strand1, 300 - 4 * (rep1 - 1 - k)) for k in range(rep1)]
            l2 += [ov(x, hi + 4 * k, -strand1, 300 - 2 * (rep2 - 1 - k)) for k in range(rep2)]
            # the repeated allele also as the smallest and as the largest of the fragment (offset 0 / range - 1 of the table)
            if (rep1, rep2) == (2, 2) and big:
                y = 2990 if big == 40 else 7010
                l1 += [ov(y, lo + 4 * k, strand1, 280 + k) for k in range(2)]
            rng.shuffle(l1)
            rng.shuffle(l2)
            frags.append((l1, l2))
    done, rows, flags = run(w, "repeated allele, narrow range", frags)
    got = routes(w, done)
    assert {"hbm", "replay"} <= got and "direct" not in got and "hash" not in got and all(flags)
    assert ("direct-left" in got) == bool(DIRECT)
    assert any(len(a) + len(b) > w.lj_cap for a, b in done) and any(len(a) + len(b) < 8 for a, b in done)
    ctx, _ = w.ctx(0.8, 0, 2000)
    assert ctx.stats()["pair_overlaps"] == sum(len(a) + len(b) for a, b in done), "a replayed fragment's records are counted once"
    run(w, "repeated allele, narrow range, single-end", frags, single=True)


def test_membership_bit(world):
    """case 5: the truncated-reference rule's tie -- an unjoined overlap with the kept mate's matchCnt and a higher similarity -- is excused only
    if its allele has a fragment (test_gpu_pair.test_truncated_reference_rule's three "equal matchCnt" cases), here among lists beyond the hash
    table in a range that fits, with the tie's allele inside the range, at offset 0 and at offset range - 1 of the table"""
    w = world
    filler = [a for a in range(1000, 1000 + w.lj_cap // 2 + 5)]
    frags, labels, where = [], [], []
    for x in (62, 20, 1000 + w.lj_cap // 2 + 900):  # inside / the smallest / the largest allele of the fragment
        for strand1 in (1, -1):
            for side in (1, 2):
                s = strand1 if side == 1 else -strand1
                m_rep = 250 if side == 1 else 240
                f1, f2 = mates(filler, 200, 200, strand1=strand1)

                def case(label, extra, joined=None):
                    l1, l2 = mates([50, 51], [250, 246], [240, 236], strand1=strand1)
                    if joined:
                        l1.append(joined[0])
                        l2.append(joined[1])
                    else:
                        (l1 if side == 1 else l2).append(extra)
                    frags.append((l1 + f1, l2 + f2))
                    labels.append(label)
                    where.append(x)

                case("higher similarity, allele not joined", ov(x, 60 if s == 1 else 190, s, m_rep, rlen=110, span=110))
                case("equal similarity, allele not joined", ov(x, 60 if s == 1 else 190, s, m_rep, rlen=150))
                if side == 1:
                    j = (ov(x, 50 if strand1 == 1 else 200, strand1, m_rep, rlen=110, span=110), ov(x, 200 if strand1 == 1 else 50, -strand1, 150))
                else:
                    j = (ov(x, 50 if strand1 == 1 else 200, strand1, 150), ov(x, 200 if strand1 == 1 else 50, -strand1, m_rep, rlen=110, span=110))
                case("higher similarity, allele joined", None, joined=j)
    done, rows, flags = run(w, "membership bit", frags)
    assert routes(w, done) == {"first-launch", long_direct()}
    for (l1, l2), x in zip(done, where):
        lo = min(l1["seq_idx"].min(), l2["seq_idx"].min())
        assert x - lo in ((0, span(l1, l2) - 1) if x != 62 else (12,))
    by = {}
    for label, fl in zip(labels, flags):
        by.setdefault(label, []).append(fl)
    assert by["higher similarity, allele not joined"] == [0] * 12 and by["higher similarity, allele joined"] == [1] * 12 and by["equal similarity, allele not joined"] == [1] * 12


def stale_fragments(w, rng):
    """four fragments in a row, again and again, each narrow one beyond the hash table's capacity (the direct route):
      n1   alleles [10, 10 + DIRECT_CAP): every word of the table in reach, the top one set from both lists; its first list-2 records lie on
           alleles Y that list 1 lacks: (j + 1) << 16 in their words
      n2b  right behind it, base 500: in list 1 only, with the best matchCnt of the fragment, the alleles whose words (allele - 500) are the
           words n1's Y set -- a word left from n1 would hand each a mate
      wide a few records far apart (the hash table): (j + 1) << 16 in the value words of its list-2 alleles
      n2   right behind it, base 10: in list 1 only the alleles whose direct words those value words are"""
    base, base2, k = 10, 500, 1400
    xs = [a for a in PLAIN if 100 < a < 8290 and base + w.slots + w.lj_hash(a) < 7990][::37][:24]
    hot = sorted(set(base + w.slots + w.lj_hash(x) for x in xs))
    ys = list(range(6000, 6020))
    hot2 = [y - base + base2 for y in ys]
    assert all(a in PLAIN for a in hot + ys + hot2) and len(hot) >= 16 and 2 * k > w.lj_cap
    wide = ([ov(9, 50, 1, 290), ov(8290, 50, 1, 290)], [ov(x, 200, -1, 300) for x in xs])
    cold = [a for a in PLAIN if base2 < a < 7990 and a not in hot and a not in ys and a not in hot2]
    out = []
    for _ in range(24):
        rng.shuffle(cold)
        l1, l2 = mates([base] + cold[:k] + [base + w.cap - 1], 296, 296)
        out.append((l1, [ov(y, 200, -1, 300) for y in ys] + l2))
        l1, l2 = mates([base2] + cold[100:100 + k], 290, 290)
        l1 += [ov(a, 50, 1, 300) for a in hot2]
        rng.shuffle(l1)
        out.append((l1, l2))
        out.append(wide)
        l1, l2 = mates([base] + cold[200:200 + k], 290, 290)
        l1 += [ov(a, 50, 1, 300) for a in hot]
        rng.shuffle(l1)
        out.append((l1, l2))
    return out


def test_no_stale_words(world):
    """case 6: in one workgroup (the hand-out gives a workgroup consecutive fragments; the call has more fragments than the child process's
    T1K_PAIR_WGS=64 workgroups) a direct fragment follows a direct fragment of another base and range, and a wide fragment on the hash table
    runs between two direct ones; each later fragment asks for exactly the words the earlier one set.  Here, and in the child, the rows are
    the oracle's: the alleles without a mate get none"""
    w, rng = world, random.Random(106)
    frags = stale_fragments(w, rng)
    done, rows, flags = run(w, "no stale words", frags)
    narrow = {"first-launch", long_direct()}
    assert [route(w, *f) for f in done[:4]] == [narrow, narrow, {"first-launch", "hash"}, narrow]
    assert span(*done[0]) == w.cap and span(*done[1]) < span(*done[0]) and done[1][0]["seq_idx"].min() != done[0][0]["seq_idx"].min()
    # (the alleles in one list only have no mate: a row holds the joined alleles, all tied at the best; the wide fragment joins nothing)
    assert all(len(r) == 0 for r in rows[2::4]) and all(len(rows[q]) == len(done[q % 4][1]) - (20 if q % 4 == 0 else 0) for q in range(len(rows)) if q % 4 != 2)
    if os.environ.get("T1K_PAIR_WGS") is None and os.environ.get("T1K_PAIR_DIRECT") is None:
        env = dict(os.environ, T1K_PAIR_WGS="64")
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_no_stale_words"],
                           env=env, cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-6000:]


def test_old_routes_keep_their_traffic(world):
    """case 7: fragments whose alleles span more than the direct table -- short ones on the hash table, with test_gpu_pair.test_join_table's
    cluster of alleles whose probe chains wrap past the last slot, and at the table's capacity; long ones on the HBM tables -- now that
    narrow ranges no longer reach those routes"""
    w, rng = world, random.Random(107)
    window_ = 40
    cluster = [a for a in PLAIN if w.lj_hash(a) >= w.slots - window_]
    first = [a for a in PLAIN if w.lj_hash(a) < 16]
    assert len(cluster) >= 64 and len(cluster) > window_ + 8
    taken, wrapped = set(), 0
    for a in cluster + first:
        h = w.lj_hash(a)
        while h in taken:
            h = (h + 1) % w.slots
        taken.add(h)
        wrapped += h < w.lj_hash(a)
    assert wrapped >= 8 and 0 in taken and w.slots - 1 in taken, "no probe chain wraps past the last slot"
    far = [8, 8 + w.cap + 20]   # two alleles further apart than the direct table is long
    assert all(a in PLAIN for a in far)
    frags = []
    for trial in range(4):
        al = [a for a in cluster + first if a not in far] + far
        rng.shuffle(al)
        l1, l2 = mates(al, [rng.choice((296, 300)) for _ in al], 300, strand1=rng.choice((1, -1)))
        rng.shuffle(l2)
        frags.append((l1, l2[:len(l2) - trial * 7] if trial else l2))
    n_hash = len(frags)
    for tot in (w.lj_cap, w.lj_cap + 1, w.frag_cap + 1):
        l1, l2 = tp.random_fragment(rng, tot // 2, tot - tot // 2)
        used1, used2 = set(r[0] for r in l1), set(r[0] for r in l2)
        # (a far pair of alleles in place of two records, should the draw have missed them)
        if far[0] not in used1 | used2:
            l1[0] = ov(far[0], 50 if l1[0][5] == 1 else 200, l1[0][5], 280)
        if far[1] not in used1 | used2:
            l1[1] = ov(far[1], 50 if l1[1][5] == 1 else 200, l1[1][5], 280)
        frags.append((l1, l2))
    done, rows, flags = run(w, "wide ranges", frags)
    assert all(span(a, b) > w.cap for a, b in done)
    assert all(route(w, a, b) == {"first-launch", "hash"} for a, b in done[:n_hash + 1])
    assert route(w, *done[n_hash + 1]) == {"first-launch", "hbm"} and route(w, *done[n_hash + 2]) == {"second-launch", "hbm"}
    assert all(flags[:n_hash])
    run(w, "wide ranges, single-end", frags, single=True)


def test_other_forms(world):
    """case 8: the direct route under the kernel's other forms: single ends and dangling mates (every overlap its own fragment), relax = 1, and
    the rowset form (rows ordered by allele, pattern hashes, a whitelist) with its coalesced groups"""
    w, rng = world, random.Random(108)
    lj = w.lj_cap
    frags = [window(rng, 2100, 3500, lj // 2 + 1, lj // 2 + 9, best_every=7) for _ in range(3)]
    frags += [window(rng, 300, 900, 60, 70, best_every=5) for _ in range(6)]
    done, _, flags = run(w, "direct, relaxed", frags, relax=1)
    assert routes(w, done) == {"first-launch", long_direct(), short_direct()} and all(flags)
    done, _, flags = run(w, "direct, single-end", frags, single=True)
    assert routes(w, done) <= {"first-launch", long_direct(), short_direct()} and all(flags)
    dang = [(a, []) for a, _ in frags[:5]] + [([], b) for _, b in frags[:5]]
    done, _, _ = run(w, "direct, dangling", dang)
    assert routes(w, done) <= {"first-launch", long_direct(), short_direct()}
    # rowset form
    t = w.sort_tile
    ctx, orc = w.ctx(0.8, 0, 0)
    rs_frags = [mates(PLAIN[500:500 + k], 300, 300, strand1=s) for k, s in ((t + 1, 1), (lj // 2 + 2, -1))]
    rs_frags += frags[3:] + frags[3:6] + [rs_frags[0]]
    rs_frags = [(as_list(a, w.alen), as_list(b, w.alen)) for a, b in rs_frags]
    assert {long_direct(), short_direct()} <= routes(w, rs_frags)
    lists = [l for fr in rs_frags for l in fr]
    ctx.reads_upload(["ACGTACGTACGTACGTACGTACGTACGTACGTACGT"] * len(lists))
    ctx.overlaps_upload([len(l) for l in lists], np.concatenate(lists))
    n = len(rs_frags)
    has_n = [k % 3 == 0 for k in range(n)]
    e1, e2 = np.arange(n) * 2, np.arange(n) * 2 + 1
    wl = np.array([rng.random() < 0.5 for _ in range(N_ALLELES)], dtype=np.uint8)
    for label, whitelist in (("direct, rowset", None), ("direct, rowset with a whitelist", wl)):
        rs = t1k_amd.Rowset(ctx, n + 3, whitelist=whitelist)
        rs.pair_into(ctx, e1, e2, has_n, frag_base=3)
        counts, rows = rs.rows(3, n)
        exp_rows, exp_flags = compare(label, rs_frags, has_n, orc, counts, rs.assigned(3, n), rows, whitelist=whitelist)
        assert rs.coalesce() == tp.coalesce_expectation(exp_rows, exp_flags), label
        ptr, ent, first = rs.groups()
        # one group for the large pattern that occurs twice (its hashes agree), first seen at its first fragment
        if whitelist is None:
            assert max(np.diff(ptr.astype(np.int64))) == t + 1 and len(exp_rows[0]) == t + 1
        rs.close()


def test_direct_off_in_a_child_process(built):
    """case 8, the switch: T1K_PAIR_DIRECT=0 in a fresh process (the library reads it once); every group above runs there on the hash table and
    the HBM tables alone, asserts those routes, and meets the same oracle rows and the same coalesced groups"""
    if os.environ.get("T1K_PAIR_DIRECT") is not None:
        return
    env = dict(os.environ, T1K_PAIR_DIRECT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not child_process"],
                       env=env, cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-6000:]
