"""CPU tests (no GPU) of the restatement of t1k_dedupe.hip (dedupe_ref.py) and of the case builder the GPU tests use (dedupe_cases.py):
the restatement against brute force, and the builder against what it claims to deliver."""
import random
import re

import pytest

import dedupe_cases as dc
import dedupe_ref as dr


def brute_collapse(reads, weights=None):
    """O(n^2): read i belongs to the first read j <= i with the same canonical string; the distinct sequences are numbered by how many first
    occurrences lie before j"""
    canon = [re.sub("[^ACGT]", "N", r) for r in reads]
    first = [min(j for j in range(i + 1) if canon[j] == canon[i]) for i in range(len(reads))]
    reps = [i for i in range(len(reads)) if first[i] == i]
    distinct_of = [sum(1 for k in range(first[i]) if first[k] == k) for i in range(len(reads))]
    weight = [sum((1 if weights is None else weights[i]) for i in range(len(reads)) if first[i] == r) for r in reps]
    return distinct_of, reps, weight


def pack(read, S):
    """forward-strand words of a read as k_pack_reads lays them out: 2 bits a base, N as N_CODE_BASE's bits plus a bit in the mask"""
    bases, mask = [0] * S, [0] * S
    for i, c in enumerate(dr.canonical(read)):
        code = "ACGT".index(dc.N_CODE_BASE if c == "N" else c)
        bases[i // 32] |= code << (2 * (i % 32))
        if c == "N":
            mask[i // 32] |= 1 << (2 * (i % 32))
    return bases, mask


FAKE_ALLELES = [dc.random_seq(random.Random(70 + i), 1500 + 100 * i) for i in range(4)]


def small_batches():
    out = [("family %d" % L, dc.family_batch(L)) for L in dc.LENGTHS]
    out += [("longest %d" % L, dc.s_batch(L)) for L, _ in dc.S_OF_LONGEST]
    out += [("n %d" % n, dc.size_batch(n)) for n in dc.SIZES if n <= 257]
    out += [("identical", dc.all_identical()), ("distinct", dc.all_distinct())]
    return out


@pytest.mark.parametrize("name,reads", small_batches(), ids=[n for n, _ in small_batches()])
def test_collapse_equals_brute_force(name, reads):
    rng = random.Random(len(reads))
    for weights in (None, [rng.randrange(6) for _ in reads]):
        got = dr.collapse(reads, weights)
        assert got == brute_collapse(reads, weights)
        distinct_of, reps, weight = got
        assert sum(weight) == (len(reads) if weights is None else sum(weights))
        assert all(distinct_of[r] == d for d, r in enumerate(reps)) and len(reps) == len(set(dr.canonical(r) for r in reads))


def test_collapse_neighbours():
    """the restatement of the all-hashes-collide build: neighbours merge, nothing else; on sorted reads it is collapse() itself"""
    assert dr.collapse_neighbours(["A", "A", "C", "A", "a", "N", ""], [1, 2, 3, 4, 5, 6, 7]) == ([0, 0, 1, 2, 3, 3, 4], [0, 2, 3, 4, 6], [3, 3, 4, 11, 7])
    assert dr.collapse_neighbours([]) == ([], [], [])
    for L in dc.LENGTHS:
        reads = sorted(dc.family_batch(L), key=dr.canonical)
        assert dr.collapse_neighbours(reads) == dr.collapse(reads)
        near = dc.twin_neighbours(L)
        f = dc.family(L)
        d = dr.collapse_neighbours(near)[0]
        assert len(near) == 3 * (len(f.twins) + len(f.longer) + len(f.aliases)) or L == 0
        k = 3 * (len(f.twins) + len(f.longer))
        assert all(d[i] < d[i + 1] < d[i + 2] for i in range(0, k, 3))   # twins side by side: a, b, a stay three runs
        assert all(d[i] == d[i + 1] == d[i + 2] for i in range(k, len(near), 3))   # an alias and its member: one run


def test_collapse_on_the_empty_batch_and_on_aliases():
    assert dr.collapse([]) == ([], [], [])
    assert dr.collapse(["ACNT", "ACnT", "ACRT", "ACTT", "acgt", "NNNN", ""], [1, 2, 3, 4, 5, 6, 7]) == ([0, 0, 0, 1, 2, 2, 3], [0, 3, 4, 6], [6, 4, 11, 7])


@pytest.mark.parametrize("L", dc.LENGTHS)
def test_family_members_and_twins(L):
    f = dc.family(L)
    assert len(f.base) == L and f.members[0] == f.base
    assert all(set(m) <= set("ACGTN") and len(m) <= dc.MAX_READ for m in f.members)
    assert len(set(f.members)) == len(f.members), "members are not pairwise distinct"
    want_pos = sorted(set(p for p in (0, 31, 32, L - 1) if 0 <= p < L))
    assert f.positions == want_pos
    for p in want_pos:
        here = [(i, j) for i, j, q in f.twins if q == p]
        assert len(here) == 10                                       # the five characters at p, pair by pair
        assert sorted(set(f.members[k][p] for ij in here for k in ij)) == list("ACGNT")
    for i, j, p in f.twins:
        a, b = f.members[i], f.members[j]
        assert len(a) == len(b) == L and [q for q in range(L) if a[q] != b[q]] == [p]
    assert [p for _, _, p in f.n_pairs] == want_pos
    S = dc.stride(f.members)
    for i, j, p in f.n_pairs:
        a, b = f.members[i], f.members[j]
        assert a[p] == dc.N_CODE_BASE and b[p] == "N" and a[:p] + a[p + 1:] == b[:p] + b[p + 1:]
        (ba, ma), (bb, mb) = pack(a, S), pack(b, S)
        assert ba == bb and ma != mb                                 # the N mask alone tells them apart
    assert [f.members[i] for i in f.longer] == [f.base + "A" * k for k in (1, 32) if L + k <= dc.MAX_READ]
    for i in f.longer:
        assert pack(f.members[i], S) == pack(f.base, S)              # the length alone tells them apart
    assert len(f.aliases) == 2 * len(want_pos)
    for s, i in f.aliases:
        assert s not in f.members and dr.canonical(s) == f.members[i] and "N" in f.members[i]
        assert re.search("[a-z]|R", s)
    # ... and the family's upload holds every member and alias, some of them twice
    batch = dc.family_batch(L)
    assert set(batch) == set(f.members) | set(a for a, _ in f.aliases) and len(batch) > len(set(batch))


def test_families_cover_the_n_code_base_at_every_kind_of_position():
    """the base sequences are random: over all families the base itself carries N_CODE_BASE at some tested position and another base at some other,
    so the pair (base sequence, N variant) and the pair (variant, N variant) both occur"""
    firsts = [i for L in dc.LENGTHS for i, _, _ in dc.family(L).n_pairs]
    assert 0 in firsts and any(i != 0 for i in firsts)


@pytest.mark.parametrize("longest,S", dc.S_OF_LONGEST)
def test_s_batches_have_the_stated_stride(longest, S):
    reads = dc.s_batch(longest)
    assert max(len(r) for r in reads) == longest and dc.stride(reads) == S
    assert min(len(r) for r in reads) == 0 and sum(1 for r in reads if len(r) <= 33) >= 20    # short reads beside the longest
    assert len(set(reads)) < len(reads)
    assert any(len(r) == longest for r in reads)


def test_size_batches():
    for n in dc.SIZES:
        reads = dc.size_batch(n)
        assert len(reads) == n and all(len(r) == 40 for r in reads)
        assert n < 255 or len(set(reads)) < n
    assert len(dc.all_identical()) == 257 and len(set(dc.all_identical())) == 1
    assert len(dc.all_distinct()) == 257 and len(set(dc.all_distinct())) == 257
    reads, counts = dc.multiplicities()
    assert min(counts.values()) == 1 and max(counts.values()) == 300
    assert all(reads.count(s) == c for s, c in counts.items()) and len(reads) == sum(counts.values())
    assert dc.size_batch(257) == dc.size_batch(257) and dc.multiplicities()[0] == reads    # deterministic


def test_aligning_reads_and_expansion():
    reads, weights = dc.aligning_reads(FAKE_ALLELES, 5, 60, 200, (40, 100, 150), fixed=(1000, 0, 32))
    assert len(reads) == len(weights) == 200 and len(set(reads)) <= 60 and set(weights) == set(range(6))
    assert sorted(set(len(r) for r in reads)) == [0, 32, 40, 100, 150, 1000]
    both = "".join(FAKE_ALLELES) + "|" + "".join(dc.revcomp(a) for a in FAKE_ALLELES)
    assert sum(1 for r in set(reads) if r in both) >= len(set(reads)) // 2       # the draws without a substitution are bases of an allele
    ex = dc.expand(reads, weights)
    assert len(ex) == sum(weights) and all(ex.count(r) == sum(w for q, w in zip(reads, weights) if q == r) for r in set(reads))


def test_link_equals_the_set_based_form():
    rng = random.Random(9)
    pool = [dc.random_seq(rng, rng.choice((0, 1, 5, 40))) for _ in range(60)] + ["ACNT", "ACnT", "ACRT"]
    windows = []
    for _ in range(6):
        windows.append(list(dict.fromkeys(dr.canonical(r) for r in rng.sample(pool, 25))))
    windows.insert(3, [])
    got = dr.link(windows)
    for w, seqs in enumerate(windows):
        earlier = set(s for v in windows[:w] for s in v)
        assert got[w][0] == set(d for d, s in enumerate(seqs) if s in earlier)
        for d, (v, e) in got[w][1].items():
            assert v < w and windows[v][e] == seqs[d] and not any(seqs[d] in windows[u] for u in range(v))
        assert set(got[w][1]) == got[w][0]
    assert got[0] == (set(), {}) and got[3] == (set(), {})
    # aliases of one read-end in different windows link
    assert dr.link([["ACNT"], ["ACnT", "ACTT"], ["ACRT"]])[1:] == [({0}, {0: (0, 0)}), ({0}, {0: (0, 0)})]


def test_xwin_windows_hold_what_they_claim():
    windows, marked = dc.xwin_windows(FAKE_ALLELES)
    assert tuple(max(len(r) for r in reads) for reads, _ in windows) == dc.XWIN_LONGEST
    assert [dc.stride(reads) for reads, _ in windows] == [6, 33, 3, 6]
    assert all(len(r) == len(w) and set(w) <= set(range(6)) and 0 in w for r, w in windows)
    assert [reads.count(marked) for reads, _ in windows] == [3, 0, 5, 0] and len(marked) == 40
    assert all(w == 1 for reads, ws in windows for r, w in zip(reads, ws) if r == marked)
    distinct = [[reads[i] for i in dr.collapse(reads)[1]] for reads, _ in windows]
    assert all(len(d) < len(reads) for d, (reads, _) in zip(distinct, windows))          # repeats inside every window
    links = dr.link(distinct)
    assert links[0] == (set(), {})
    for w in (1, 2, 3):
        assert set(v for v, _ in links[w][1].values()) == set(range(w))                  # a later window repeats some of every earlier one
        assert len(links[w][0]) < len(distinct[w])
    by_len = lambda w, v: set(len(distinct[w][d]) for d, (u, _) in links[w][1].items() if u == v)
    assert {0, 32, 64} <= by_len(1, 0) and 160 in by_len(3, 1) and {0, 32} <= by_len(2, 0)
    # near twins of earlier sequences that must not link: one position apart, or the same bases and another length
    for w in (1, 2):
        earlier = set(dr.canonical(s) for v in distinct[:w] for s in v)
        fresh = [dr.canonical(distinct[w][d]) for d in range(len(distinct[w])) if d not in links[w][0]]
        one_off = sum(1 for s in fresh for e in earlier if len(e) == len(s) and sum(a != b for a, b in zip(e, s)) == 1)
        longer = sum(1 for s in fresh if s.endswith("A") and s[:-1] in earlier)
        assert one_off >= 10 and longer >= 3, (w, one_off, longer)
    # the aliases of window 2 link to the N variants window 1 saw
    assert any(re.search("[a-z]|R", distinct[2][d]) and v == 1 for d, (v, _) in links[2][1].items())


def test_undersized_table_windows():
    first, second = dc.undersized_windows(FAKE_ALLELES)
    assert len(first) == len(set(first)) == 1500 and len(second) == len(set(second)) == 1000
    assert len(set(first) & set(second)) == 500 and all(len(r) == 40 for r in first + second)
    assert len(dr.link([first, second])[1][0]) == 500


def test_job_fragments_layout():
    frags = dc.job_fragments([a * 2 for a in FAKE_ALLELES])
    assert len(frags) == 184
    assert all(len(a) == len(b) == 150 for a, b in frags[:8])
    mid, last = frags[8:80], frags[80:]
    assert all(any(len(a) == 1000 for a, _ in mid[i:i + 8]) for i in range(len(mid) - 7))     # every window cut there holds a 1000-base read
    assert sum(1 for f in mid if f in frags[:8]) == 8 and sum(1 for a, _ in mid if len(a) == 40) == 8
    assert all(len(a) == len(b) == 40 for a, b in last)
    mates = set(m for f in mid for m in f if len(m) == 40)
    assert sum(1 for a, b in last if a in mates and b in mates) == 52
