"""The pairing stage (k_pair: SeqSet::ReadAssignmentToFragmentAssignment + Genotyper::SetReadAssignments) against the oracle's restatement
of the same two routines, fragment by fragment (pytest -m gpu).

Part a pairs the overlap lists the GPU's own assignment produced (downloaded, so that pairing is judged apart from assignment); part b
pairs lists made by the host (t1k_overlaps_upload) on a hand-made reference, placed on the sizes at which the kernel changes its
route.  Those sizes come from t1k_pair_limits; every group asserts from its inputs that its route is reached.  The expectation is
always util.Oracle.pair_rows on the very lists the kernel read."""
import os
import random

import numpy as np
import pytest

import t1k_amd
import util

pytestmark = pytest.mark.gpu

FIELDS = ("seq_idx", "read_start", "read_end", "seq_start", "seq_end", "strand", "match_cnt", "left_clip", "right_clip", "relaxed_match_cnt")
# The library reads T1K_PAIR_LIST once per process: with it, mates that both have a list are joined through the materialised fragment list (k_pair's
# list form) instead of the streamed passes.  test_list_form_in_a_child_process runs the synthetic groups again in a process that has it set.
LIST_FORM = os.environ.get("T1K_PAIR_LIST") is not None
JOINED = "list" if LIST_FORM else "stream"
HIT_LEN = 31      # t1k_params_default / the oracle's Params: the dangling rule's 3 * hitLenRequired
SPAN_RANGE = 100  # the dangling rule's spanRange (SeqSet.hpp:2567)


# ------------------------------------------------------------------------------------------------------------------
# comparison: one helper for every test
# ------------------------------------------------------------------------------------------------------------------
def show_list(l, head=12):
    if l is None:
        return "    (none: single-end)"
    s = ["    %d overlaps" % len(l)]
    for r in l[:head]:
        s.append("    " + " ".join("%s=%d" % (f, r[f]) for f in FIELDS) + " similarity=%r" % float(r["similarity"]))
    if len(l) > head:
        s.append("    ... and %d more" % (len(l) - head))
    return "\n".join(s)


def compare(label, frags, has_n, orc, counts, assigned, rows, whitelist=None, raw=False):
    """frags: [(l1, l2 or None)] as paired by the GPU; counts / assigned / rows: what it returned (rows in the reference's row order).
    Per fragment: row count, fragAssigned, allele_idx / start / end, weight and adjust_weight as 32-bit patterns, qual == 1 -- against
    Oracle.pair_rows on the same lists.  The first differing fragment is reported with its two lists.  raw: the rows are the undropped
    fragment list (allele, start, end only).  Returns the oracle's rows and flags (for the coalescing expectations)."""
    assert len(counts) == len(frags) and len(assigned) == len(frags) and int(counts.sum()) == len(rows), label
    pos = 0
    exp_rows, exp_flags = [], []
    for f, (l1, l2) in enumerate(frags):
        res = orc.pair_rows(l1, l2, has_n[f], whitelist=whitelist, raw=raw)
        want, flag = res[0], res[1]
        got = rows[pos:pos + counts[f]]
        pos += counts[f]
        bad = None
        if raw:
            w3 = res[2]
            if len(w3) != len(got):
                bad = "raw list length: oracle %d, gpu %d" % (len(w3), len(got))
            elif not (np.array_equal(w3[:, 0], got["allele_idx"]) and np.array_equal(w3[:, 1], got["start"]) and np.array_equal(w3[:, 2], got["end"])):
                bad = "raw list entries: oracle %s, gpu %s" % (w3[:8].tolist(), got[:8].tolist())
        elif len(want) != len(got):
            bad = "row count: oracle %d, gpu %d" % (len(want), len(got))
        if bad is None and int(assigned[f]) != flag:
            bad = "fragAssigned: oracle %d, gpu %d" % (flag, assigned[f])
        if bad is None and not raw:  # (the raw form's weights are not part of the reference's list)
            for field in ("allele_idx", "start", "end"):
                if not np.array_equal(want[field], got[field]):
                    k = int(np.nonzero(want[field] != got[field])[0][0])
                    bad = "%s of entry %d: oracle %d, gpu %d (oracle alleles %s, gpu alleles %s)" % (field, k, want[field][k], got[field][k], want["allele_idx"][:8].tolist(), got["allele_idx"][:8].tolist())
                    break
        if bad is None and not raw:
            for field in ("weight", "adjust_weight"):
                a, b = want[field].view(np.uint32), got[field].view(np.uint32)
                if not np.array_equal(a, b):
                    k = int(np.nonzero(a != b)[0][0])
                    bad = "%s of entry %d: oracle %r, gpu %r" % (field, k, float(want[field][k]), float(got[field][k]))
                    break
        if bad is None and not np.all(got["qual"] == 1.0):
            bad = "qual != 1: %s" % got["qual"][:8].tolist()
        if bad is not None:
            raise AssertionError("%s: fragment %d (hasN %d): %s\n  list 1:\n%s\n  list 2:\n%s" % (label, f, has_n[f], bad, show_list(l1), show_list(l2)))
        exp_rows.append(res[0])
        exp_flags.append(flag)
    return exp_rows, exp_flags


def fragment_lists(counts, ovl, e1, e2):
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cut = lambda e: ovl[starts[e]:starts[e] + counts[e]]
    return [(cut(a), None if e2 is None else cut(b)) for a, b in zip(e1, e1 if e2 is None else e2)]


# ------------------------------------------------------------------------------------------------------------------
# a. real lists: assignment on the GPU, its lists downloaded, pairing on the GPU against the oracle on those lists
# ------------------------------------------------------------------------------------------------------------------
def real_case(name, tmp):
    import goldens
    if name == "adversarial":
        import test_gpu_fuzz as fz
        ref = os.path.join(tmp, "ref.fa")
        util.synth_ref("ref-rna", ref, seed=5, genes=6, scale=0.3)
        pairs = fz.adversarial_pairs(fz.alleles(ref), random.Random(17), 400)
        return ref, [p[0] for p in pairs], [p[1] for p in pairs], 0.8, False
    c = goldens.Case(name, tmp)
    r1 = [s for _, _, s in t1k_amd.read_fastx(c.r1)][:300]
    r2 = [s for _, _, s in t1k_amd.read_fastx(c.r2)][:300]
    return c.ref, r1, r2, float(c.flags[c.flags.index("-s") + 1]), "--relaxIntronAlign" in c.flags


@pytest.mark.parametrize("name,sim,relax", [("hla_synth_2x150", 0.97, False), ("cyp_dna_relax_2x150", 0.9, True), ("adversarial", 0.8, False)])
def test_real_lists_vs_oracle(built, tmp_path, name, sim, relax):
    """the lists t1k_assign_batch left on the device, paired as mates, as single ends, and after identical read-ends were collapsed"""
    ref, r1, r2, s, rl = real_case(name, str(tmp_path))
    assert (s, rl) == (sim, relax)
    n = len(r1)
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(ref)
    orc = util.Oracle(ref, similarity=sim, relax=relax)
    assert orc.n_alleles == len(seqs)
    reads = [x for pr in zip(r1, r2) for x in pr]
    n_pair = [1 if ("N" in a or "N" in b) else 0 for a, b in zip(r1, r2)]   # Genotyper.cpp:537-539
    n_single = [1 if "N" in x else 0 for x in reads]
    ctx = t1k_amd.Context(ref_seq_similarity=sim, relax_intron_align=1 if relax else 0)
    ctx.ref_upload(seqs, masks)
    for dedupe in (False, True):
        ctx.reads_upload(reads)
        idx = ctx.reads_dedupe().astype(np.int64) if dedupe else np.arange(2 * n)
        if dedupe:
            assert ctx.n_read_ends <= 2 * n
        ctx.assign()
        counts, ovl = ctx.overlaps()
        assert len(counts) == ctx.n_read_ends and len(ovl) > n
        e1, e2 = idx[0::2], idx[1::2]
        ctx.pair(e1, e2, n_pair)
        got = ctx.rows()
        frags = fragment_lists(counts, ovl, e1, e2)
        compare("%s paired%s" % (name, " deduped" if dedupe else ""), frags, n_pair, orc, *got)
        assert got[1].sum() > n // 10, "hardly any fragment was assigned: the case checks nothing"
        ctx.pair(idx, None, n_single)
        got = ctx.rows()
        compare("%s single-end%s" % (name, " deduped" if dedupe else ""), fragment_lists(counts, ovl, idx, None), n_single, orc, *got)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# b. synthetic lists on a hand-made reference
# ------------------------------------------------------------------------------------------------------------------
N_ALLELES = 8300          # more than the first launch's fragment capacity: one list can hold that many distinct alleles
LEN, SHORT_LEN = 400, 250
SHORT = range(8000, 8100)  # the shorter group
SEPS = {5: 200, 6: 330, 7: 60, 8050: 125}  # allele -> position of its N (a separator, SeqSet.hpp:924-928)


def make_reference(path):
    """about 8 300 alleles of one gene: one random 400-mer in which allele k differs by the base-4 digits of k written at seven fixed positions
    (so no two are identical and none is merged on loading); a few carry one N; alleles 8000-8099 are 250 bases long"""
    rng = random.Random(20240607)
    base = [rng.choice("ACGT") for _ in range(LEN)]
    lens = []
    with open(path, "w") as f:
        for k in range(N_ALLELES):
            s = list(base)
            for d in range(7):
                s[13 + 31 * d] = "ACGT"[(k >> (2 * d)) & 3]
            if k in SEPS:
                s[SEPS[k]] = "N"
            if k in SHORT:
                s = s[:SHORT_LEN]
            lens.append(len(s))
            f.write(">G*%05d\n%s\n" % (k, "".join(s)))
    return np.array(lens)


class World:
    """the synthetic reference, the kernel's limits, and one GPU context + oracle per parameter set (contexts are kept for the whole module:
    every later call runs on per-workgroup tables that earlier calls stamped)"""

    def __init__(self, tmp):
        self.fasta = os.path.join(tmp, "pair_ref.fa")
        self.alen = make_reference(self.fasta)
        self.names, self.seqs, self.masks, _ = t1k_amd.load_reference_fasta(self.fasta)
        assert len(self.seqs) == N_ALLELES and all(len(s) == l for s, l in zip(self.seqs, self.alen))
        self.lj_cap, self.frag_cap, self.sort_tile, self.round = t1k_amd.pair_limits()
        slots = [p for p in (1 << b for b in range(8, 20)) if p * 17 // 25 == self.lj_cap]
        assert len(slots) == 1, "the LDS join table's capacity is no longer 68 % of a power of two"
        self.slots = slots[0]
        # workgroup sizes the kernel may be built with: multiples of a wavefront that divide one round of the streamed passes
        self.wgs = [d for d in range(64, self.round + 1, 64) if self.round % d == 0]
        assert self.wgs and self.lj_cap < self.frag_cap and 2 * self.frag_cap <= 2 * (N_ALLELES - 100) and 2 * self.sort_tile + 50 < self.lj_cap * 4
        self.ctxs, self.orcs = {}, {}

    def ctx(self, sim=0.8, relax=0, max_assign=2000):
        key = (sim, relax, max_assign)
        if key not in self.ctxs:
            c = t1k_amd.Context(ref_seq_similarity=sim, relax_intron_align=relax, max_assign_cnt=max_assign if max_assign else -1)  # (0 asks t1k_ctx_create for the default; -1 is the reference's "-n 0": no limit)
            c.ref_upload(self.seqs, self.masks)
            self.ctxs[key] = c
            self.orcs[key] = util.Oracle(self.fasta, similarity=sim, relax=bool(relax), max_assign=max_assign)
            assert self.orcs[key].n_alleles == N_ALLELES
        return self.ctxs[key], self.orcs[key]

    def lj_hash(self, allele):
        return ((allele * 2654435761) & 0xFFFFFFFF) >> (32 - self.slots.bit_length() + 1)

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(str(tmp_path_factory.mktemp("pair")))
    yield w
    w.close()


def ov(allele, start, strand, match, rlen=150, span=None, relaxed=None, rs=0, lc=0, rc=0):
    span = rlen if span is None else span
    return (allele, rs, rs + rlen - 1, start, start + span - 1, strand, match, lc, rc, match if relaxed is None else relaxed, 0.0)


def as_list(recs, alen):
    """One read-end's overlap list from ov() tuples.  What SeqSet::AssignRead guarantees and k_pair relies on, asserted here:
      * every overlap of a read-end's list lies on one strand (the kernel reads the strand of the first record only);
      * 0 <= seqStart <= seqEnd < allele length;
      * every field inside the packed ranges of t1k_ovl_pack (allele < 2^24, seqStart < 2^20, seqEnd - seqStart < 4096, read coordinates
        and clips < 1024, matchCnt and relaxedMatchCnt < 4096);
      * similarity = matchCnt / (read span + allele span + 2 * clips), evaluated in float64 -- the kernel keeps no similarity, ovlSim
        recomputes exactly this quotient."""
    l = np.array(recs, dtype=t1k_amd.OVERLAP_DTYPE) if len(recs) else np.zeros(0, dtype=t1k_amd.OVERLAP_DTYPE)
    if len(l):
        assert len(set(l["strand"].tolist())) == 1 and l["strand"][0] in (1, -1)
        assert np.all(l["seq_start"] >= 0) and np.all(l["seq_start"] <= l["seq_end"]) and np.all(l["seq_end"] < alen[l["seq_idx"]])
        assert np.all(l["seq_idx"] >= 0) and np.all(l["seq_idx"] < min(len(alen), 1 << 24)) and np.all(l["seq_start"] < (1 << 20)) and np.all(l["seq_end"] - l["seq_start"] < 4096)
        for f in ("read_start", "read_end", "left_clip", "right_clip"):
            assert np.all(l[f] >= 0) and np.all(l[f] < 1024), f
        assert np.all(l["read_start"] <= l["read_end"])
        for f in ("match_cnt", "relaxed_match_cnt"):
            assert np.all(l[f] >= 0) and np.all(l[f] < 4096), f
        den = (l["read_end"] - l["read_start"] + 1 + l["seq_end"] - l["seq_start"] + 1 + 2 * l["left_clip"] + 2 * l["right_clip"]).astype(np.float64)
        l["similarity"] = l["match_cnt"].astype(np.float64) / den
    return l


def route(w, l1, l2):
    """the routes of k_pair a fragment takes, derived from its lists and the kernel's limits alone (t1k_pair.hip: the join-table choice, the
    duplicate test, `stream`, the hand-over to the second launch)"""
    n1, n2 = len(l1), 0 if l2 is None else len(l2)
    dup = len(set(l1["seq_idx"].tolist())) < n1 or (l2 is not None and len(set(l2["seq_idx"].tolist())) < n2)
    r = set()
    r.add("second-launch" if n1 + n2 > w.frag_cap else "first-launch")
    r.add("lds" if n1 + n2 <= w.lj_cap and not dup else "hbm")
    if dup:
        r.add("replay")
    elif l2 is not None and n1 and n2:
        r.add(JOINED)   # both mates have a list: the streamed form, or the list form the library takes when T1K_PAIR_LIST is set
    else:
        r.add("unpaired")  # single ends and dangling mates: every overlap its own fragment
    return r


def routes(w, frags):
    out = set()
    for l1, l2 in frags:
        out |= route(w, l1, l2)
    return out


def run(w, label, frags, has_n=None, sim=0.8, relax=0, max_assign=2000, single=False):
    """frags: [(l1, l2)] of ov()-tuple lists (l2 ignored for a single-end call).  Uploads the lists, pairs on the GPU, compares with the oracle."""
    ctx, orc = w.ctx(sim, relax, max_assign)
    frags = [(as_list(a, w.alen), None if single else as_list(b, w.alen)) for a, b in frags]
    has_n = [0] * len(frags) if has_n is None else has_n
    lists = [l for fr in frags for l in (fr if not single else fr[:1])]
    ctx.reads_upload(["ACGTACGTACGTACGTACGTACGTACGTACGTACGT"] * len(lists))  # (the reads' text is irrelevant to pairing)
    ctx.overlaps_upload([len(l) for l in lists], np.concatenate(lists) if lists else np.zeros(0, dtype=t1k_amd.OVERLAP_DTYPE))
    n = len(frags)
    if single:
        ctx.pair(np.arange(n), None, has_n)
    else:
        ctx.pair(np.arange(n) * 2, np.arange(n) * 2 + 1, has_n)
    counts, assigned, rows = ctx.rows()
    exp_rows, exp_flags = compare(label, frags, has_n, orc, counts, assigned, rows)
    return frags, exp_rows, exp_flags


def mates(alleles, m1, m2, s1=50, s2=200, strand1=1, rlen=150, r1=None, r2=None):
    """a proper pair's two lists on the given alleles: mate 1 on strand1 at s1, mate 2 on the other strand at s2.  m1 / m2 / r1 / r2 (matchCnt and
    relaxedMatchCnt of the two mates): one value or one per allele"""
    at = lambda v, i: v[i] if isinstance(v, (list, tuple, np.ndarray)) else v
    if strand1 == -1:
        s1, s2 = s2, s1
    l1 = [ov(a, s1, strand1, at(m1, i), rlen, relaxed=None if r1 is None else at(r1, i)) for i, a in enumerate(alleles)]
    l2 = [ov(a, s2, -strand1, at(m2, i), rlen, relaxed=None if r2 is None else at(r2, i)) for i, a in enumerate(alleles)]
    return l1, l2


def random_fragment(rng, n1, n2, best_every=97):
    """lists of n1 / n2 distinct alleles (long alleles only), about half of the shorter list's alleles in both; matchCnt mostly 280 .. 296,
    every best_every-th joinable allele 300 on both mates (the ties at the best), some mates in the wrong order (no join)"""
    pool = [a for a in range(N_ALLELES) if a not in SHORT and a not in SEPS]
    rng.shuffle(pool)
    common = min(n1, n2) // 2 if min(n1, n2) > 1 else min(n1, n2)
    common = max(common, n1 + n2 - len(pool))  # (lists longer than half the reference share more)
    a1 = pool[:n1]
    a2 = pool[:common] + pool[n1:n1 + n2 - common]
    assert len(a2) == n2 and len(set(a2)) == n2
    strand1 = rng.choice((1, -1))
    m = {}
    for k, a in enumerate(pool[:common]):
        m[a] = (300, 300) if k % best_every == 0 else (rng.choice((280, 288, 294, 296)), rng.choice((280, 290, 296)))
    lo, hi = (50, 200) if strand1 == 1 else (200, 50)
    l1 = [ov(a, lo + rng.randrange(3), strand1, m[a][0] if a in m else rng.choice((280, 296, 300))) for a in a1]
    l2 = [ov(a, (hi if rng.random() < 0.9 else lo) + rng.randrange(3), -strand1, m[a][1] if a in m else rng.choice((280, 296, 300))) for a in a2]
    rng.shuffle(l1)
    rng.shuffle(l2)
    return l1, l2


def test_list_lengths(world):
    """group 1: list lengths on every size at which a loop of the kernel takes another trip -- the wavefront, the workgroup, one round of the
    streamed passes -- as mates, with one list empty (the dangling candidates) and as single ends"""
    w, rng = world, random.Random(1)
    sizes = sorted(set([0, 1, 2, 63, 64, 65, 1023, 1025] + [d + k for d in w.wgs for k in (-1, 0, 1)]))
    assert w.round + 1 in sizes and max(sizes) * 2 <= w.lj_cap
    pairs = [(a, b) for a in sizes for b in (sizes[(sizes.index(a) * 5 + 3) % len(sizes)], a)]
    pairs += [(0, b) for b in sizes] + [(a, 0) for a in sizes]
    frags = [random_fragment(rng, a, b) for a, b in pairs]
    done, _, flags = run(w, "list lengths", frags)
    assert routes(w, done) == {"first-launch", "lds", JOINED, "unpaired"} and sum(flags) > len(frags) // 3
    done, _, flags = run(w, "list lengths, single-end", frags, single=True)
    assert routes(w, done) == {"first-launch", "lds", "unpaired"} and sum(flags) >= len(frags) - 2 * len(sizes)


def test_ties_first_in_order(world):
    """group 2: several joined fragments share the best (matchCnt, similarity): at list-1 indices i, i + d for every possible workgroup size d and
    i + one round (the same lane's next trips), in other wavefronts, at the last index.  The reference takes the first in order
    (SeqSet.hpp:2474-2487): with --relaxIntronAlign its relaxedMatchCnt decides which near-best fragments stay, so every tied fragment gets a
    relaxedMatchCnt of its own and a near-best fragment that only that one would keep; the row keeps list order."""
    w, rng = world, random.Random(2)
    n = 2 * w.round + 70
    pool = [a for a in range(N_ALLELES) if a not in SHORT and a not in SEPS]
    frags, firsts = [], []
    for i in (0, 1, 37, 63, 64, 200):
        at = sorted(set([i, i + 5, i + 64, i + w.round, n - 1] + [i + d for d in w.wgs]))  # (i + 5: another lane of the same wavefront)
        for lead in range(len(at)):           # the first tie moves along: each of the positions is the first in order once
            ties = at[lead:]
            rng.shuffle(pool)
            al = pool[:n]
            m1, m2, r1, r2 = [290] * n, [290] * n, [300] * n, [300] * n
            near = [q for q in range(n) if q not in ties]
            rng.shuffle(near)
            for k, t in enumerate(ties):
                m1[t], m2[t] = 300, 298
                r1[t], r2[t] = 310 + k, 305          # the k-th tie's relaxed sum: 615 + k
                for q in near[3 * k:3 * k + 3]:       # near-best fragments only the k-th tie's relaxed sum keeps
                    m1[q], m2[q] = 298, 298
                    r1[q], r2[q] = 310 + k, 305
            frags.append(mates(al, m1, m2, r1=r1, r2=r2, strand1=rng.choice((1, -1))))
            firsts.append(ties[0])
    done, rows, flags = run(w, "ties", frags, relax=1)
    assert routes(w, done) == {"first-launch", "lds", JOINED} and all(flags)
    for (l1, _), r, first in zip(done, rows, firsts):
        # the first tie and its three near-best fragments stay, in list order, next to the other ties
        kept = set(r["allele_idx"].tolist())
        assert l1["seq_idx"][first] in kept and len(r) >= 4
        assert [a for a in l1["seq_idx"].tolist() if a in kept] == r["allele_idx"].tolist()
    # the same lists as single ends (the unpaired branch: a two-step reduction over the materialised fragments and its own "first in order" resolution)
    done, rows, flags = run(w, "ties, single-end", frags, relax=1, single=True)
    assert routes(w, done) == {"first-launch", "lds", "unpaired"} and all(flags)


def test_join_table(world):
    """group 3: both lists together at the capacity of the LDS join table and one above it (the per-workgroup tables in device memory), and a
    cluster of alleles whose home slots are the table's last ones: more keys than slots up to the end, so the probe chain wraps past the
    last slot.  (With 8 300 alleles the multiplicative hash puts two or three into any one slot; sixty-four in ONE slot need a quarter of
    a million alleles.  The cluster makes the same chain: every key probes through the slots taken before it.)"""
    w, rng = world, random.Random(3)
    frags = []
    for tot in (w.lj_cap - 1, w.lj_cap, w.lj_cap + 1, w.lj_cap + 2):
        for n1 in (tot // 2, tot // 3, tot - 1):
            frags.append(random_fragment(rng, n1, tot - n1))
    window = 40
    cluster = [a for a in range(N_ALLELES) if w.lj_hash(a) >= w.slots - window and a not in SHORT and a not in SEPS]
    assert len(cluster) >= 64 and len(cluster) > window + 8, "the cluster no longer overflows the table's last slots"
    first = [a for a in range(N_ALLELES) if w.lj_hash(a) < 16 and a not in SHORT and a not in SEPS]  # the slots the wrapped chain runs into
    # the table after the inserts (which slots end up taken does not depend on the order of linear-probing inserts): keys whose home slot is one of
    # the last `window` come to rest in slot 0 or behind it, and keys whose home is among the first slots are pushed on by them
    taken, wrapped, pushed = set(), 0, 0
    for a in cluster + first:
        h = w.lj_hash(a)
        while h in taken:
            h = (h + 1) % w.slots
        taken.add(h)
        wrapped += h < w.lj_hash(a)
        pushed += w.lj_hash(a) < 16 and h != w.lj_hash(a)
    assert wrapped >= 8 and pushed >= 8 and 0 in taken and w.slots - 1 in taken, "no probe chain wraps past the last slot"
    for trial in range(6):
        al = cluster + first
        rng.shuffle(al)
        m1 = [rng.choice((296, 300)) for _ in al]
        l1, l2 = mates(al, m1, 300, strand1=rng.choice((1, -1)))
        rng.shuffle(l2)
        frags.append((l1, l2[:len(l2) - trial * 7]))
    done, _, flags = run(w, "join table", frags)
    assert routes(w, done) == {"first-launch", "lds", "hbm", JOINED} and all(flags)
    assert sorted(len(a) + len(b) for a, b in done[:12:3]) == [w.lj_cap - 1, w.lj_cap, w.lj_cap + 1, w.lj_cap + 2]
    run(w, "join table, single-end", frags, single=True)


def test_repeated_allele(world):
    """group 4: an allele two and three times in list 1, in list 2, in both (the one-lane replay of SeqSet.hpp:2385-2455 keeps the better
    fragment per allele: placed second here), alone and among many alleles, once with lists above the LDS capacity"""
    w, rng = world, random.Random(4)
    frags = []
    for big in (0, 40, w.lj_cap + 10):
        for rep1, rep2 in ((2, 1), (3, 1), (1, 2), (1, 3), (2, 2), (3, 3), (2, 3)):
            for strand1 in (1, -1):
                l1, l2 = random_fragment(rng, big // 2, big - big // 2) if big else ([], [])
                if l1:
                    strand1 = l1[0][5]
                used = set(r[0] for r in l1 + l2)
                x = next(a for a in range(100, N_ALLELES) if a not in used and a not in SEPS and a not in SHORT)
                lo, hi = (40, 190) if strand1 == 1 else (190, 40)
                # later copies are the better ones; the last copy of each list ties the best of the fragment
                l1 += [ov(x, lo + 4 * k, strand1, 300 - 4 * (rep1 - 1 - k)) for k in range(rep1)]
                l2 += [ov(x, hi + 4 * k, -strand1, 300 - 2 * (rep2 - 1 - k)) for k in range(rep2)]
                rng.shuffle(l1)
                rng.shuffle(l2)
                frags.append((l1, l2))
    done, rows, flags = run(w, "repeated allele", frags)
    assert routes(w, done) == {"first-launch", "hbm", "replay"} and all(flags)
    assert any(len(a) + len(b) > w.lj_cap for a, b in done) and any(len(a) + len(b) < 8 for a, b in done)
    done, _, _ = run(w, "repeated allele, relaxed", frags, relax=1)
    done, _, flags = run(w, "repeated allele, single-end", frags, single=True)
    assert "replay" in routes(w, done) and all(flags)
    # dangling: the repeated allele in the only list
    run(w, "repeated allele, dangling", [(a, []) for a, _ in frags[:14]] + [([], b) for _, b in frags[:14]])


def test_second_launch(world):
    """group 5: both lists together at the first launch's capacity and one above, one fragment of about twice that, among small fragments in
    the same call: both launches write rows"""
    w, rng = world, random.Random(5)
    c = w.frag_cap
    big = [(c // 2, c - c // 2), (c // 2, c - c // 2 + 1), (c - 100, 101), (c - 4, c - 7), (c + 1, 0), (0, c + 1), (c, 0)]
    frags = []
    for n1, n2 in big:
        frags += [random_fragment(rng, rng.randrange(1, 90), rng.randrange(1, 90)) for _ in range(5)]
        frags.append(random_fragment(rng, n1, n2))
    frags += [random_fragment(rng, 30, 30) for _ in range(5)]
    done, rows, flags = run(w, "second launch", frags)
    sizes = [len(a) + len(b) for a, b in done]
    assert c in sizes and c + 1 in sizes and max(sizes) >= 2 * c - 16
    assert routes(w, done) == {"first-launch", "second-launch", "lds", "hbm", JOINED, "unpaired"}
    second = [f for f, s in enumerate(sizes) if s > c]
    assert any(len(rows[f]) for f in second) and any(len(rows[f]) for f in range(len(frags)) if f not in second)
    # a repeated allele in a fragment of the second launch
    l1, l2 = random_fragment(rng, c // 2 + 3, c // 2 + 3)
    x = l1[7][0]
    l1.append(ov(x, l1[7][3] + 5, l1[0][5], 300))
    done, _, _ = run(w, "second launch, repeated allele", [random_fragment(rng, 20, 20), (l1, l2), random_fragment(rng, 5, 9)])
    assert {"second-launch", "replay"} <= routes(w, done)


def test_no_join(world):
    """group 6: mates that do not form a fragment (SeqSet.hpp:2369-2380): both on one strand, plus-strand mate 1 not left of mate 2 and the
    mirrored minus case, alleles in one list only -- alone (no fragment at all) and beside one better allele that does join"""
    w = world
    al = list(range(100, 140))
    frags = []
    for good in (False, True):
        for s in (1, -1):
            extra1 = [ov(99, 50 if s == 1 else 200, s, 300)] if good else []
            extra2 = [ov(99, 200 if s == 1 else 50, -s, 300)] if good else []
            frags.append(([ov(a, 50, s, 290) for a in al] + extra1[:0], [ov(a, 200, s, 290) for a in al]))            # one strand
            frags.append(([ov(a, 200, s, 290) for a in al] + extra1, [ov(a, 200, -s, 290) for a in al] + extra2))      # equal starts
            frags.append(([ov(a, 200 if s == 1 else 50, s, 290) for a in al] + extra1, [ov(a, 50 if s == 1 else 200, -s, 290) for a in al] + extra2))  # wrong order
            frags.append(([ov(a, 50 if s == 1 else 200, s, 290) for a in al] + extra1, [ov(a + 1000, 200 if s == 1 else 50, -s, 290) for a in al] + extra2))  # disjoint alleles
            frags.append(([ov(a, 200 - (a & 1) * s, s, 290) for a in al], [ov(a, 200, -s, 290) for a in al]))  # one base either side of the boundary
    done, rows, flags = run(w, "no join", frags)
    assert routes(w, done) == {"first-launch", "lds", JOINED}
    assert flags[:10] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1] and flags[10] == 0 and flags[15] == 0 and all(flags[11:15]) and all(flags[16:20])
    assert all(len(r) == 1 and r["allele_idx"][0] == 99 for r in (rows[11], rows[12], rows[13], rows[16], rows[17], rows[18]))


def test_relaxed_keep(world):
    """group 7 (--relaxIntronAlign, SeqSet.hpp:2488-2545): a fragment stays if it is within 2 of the best matchCnt -- within 4 if its mates
    overlap on the allele and both have matchCnt < relaxedMatchCnt -- and its relaxedMatchCnt equals the best's.  Fragments at best - 2, - 3,
    - 4, - 5 with every combination of the three conditions"""
    w, rng = world, random.Random(7)
    frags = []
    for strand1 in (1, -1):
        for trial in range(4):
            recs = []  # (allele, d, overlap, both_lt, equal)
            a = 300 + 500 * trial
            l1, l2 = [], []
            best_at = None
            for d in (0, 1, 2, 3, 4, 5):
                for overlap in (True, False):
                    for both_lt in (True, False):
                        for equal in (True, False):
                            a += 1
                            m1, m2 = 295 - d, 295
                            r1, r2 = (300, 300) if both_lt else (305, 295)
                            if not equal:
                                r1 -= 2
                            if d == 0 and best_at is None:
                                best_at, r1, r2 = a, 300, 300
                            lo = 80 if overlap else 40            # (far enough from both allele ends for the truncated-reference rule to stay out of it)
                            hi = 180 if overlap else 195          # mate 1 spans lo .. lo + 149
                            s1, s2 = (lo, hi) if strand1 == 1 else (hi, lo)
                            l1.append(ov(a, s1, strand1, m1, relaxed=r1))
                            l2.append(ov(a, s2, -strand1, m2, relaxed=r2))
            if trial:
                both = list(zip(l1, l2))
                rng.shuffle(both)
                l1, l2 = [x for x, _ in both], [y for _, y in both]
                rng.shuffle(l2)
            frags.append((l1, l2))
    done, rows, flags = run(w, "relaxed keep", frags, relax=1)
    assert routes(w, done) == {"first-launch", "lds", JOINED} and all(flags)
    # unshuffled fragment 0: the best's own rows plus, of the others, exactly those within the margin with the equal relaxed sum
    l1 = done[0][0]
    d_of = {int(r["seq_idx"]): 295 - int(r["match_cnt"]) for r in l1}
    kept_d = sorted(d_of[a] for a in rows[0]["allele_idx"].tolist())
    assert 4 in kept_d and 3 in kept_d and 5 not in kept_d and kept_d.count(2) > kept_d.count(4), kept_d
    run(w, "relaxed keep, without the option", frags, relax=0)
    # the same fragments through the one-lane replay (an allele twice in list 1), whose keep filter reads the materialised fragment list
    replay = []
    for l1, l2 in frags:
        s1 = l1[0][5]
        replay.append((l1 + [ov(9, 80 if s1 == 1 else 180, s1, 200), ov(9, 84 if s1 == 1 else 184, s1, 210)], l2 + [ov(9, 180 if s1 == 1 else 80, -s1, 200)]))
    done, rows2, flags = run(w, "relaxed keep, replay", replay, relax=1)
    assert routes(w, done) == {"first-launch", "hbm", "replay"} and all(flags)
    assert [r["allele_idx"].tolist() for r in rows2] == [r["allele_idx"].tolist() for r in rows]


def dangling_cases(w):
    """(label, l1-or-l2 records, strand) of single-overlap dangling fragments on both sides of every boundary of SeqSet.hpp:2553-2578"""
    out = []
    L = LEN
    for strand in (1, -1):
        ok_start = (L - SPAN_RANGE) - 150 + 1 if strand == 1 else SPAN_RANGE - 1 - 20  # passes the span-range test: seqEnd + 100 == len / seqStart - 100 == -21
        # similarity 1 and just below
        out.append(("sim 1", [ov(20, ok_start, strand, 300)]))
        out.append(("sim below 1", [ov(20, ok_start, strand, 299)]))
        # read span + allele span at 3 * hitLenRequired - 1 and at 3 * hitLenRequired
        for tot in (3 * HIT_LEN - 1, 3 * HIT_LEN):
            rl, sp = tot // 2, tot - tot // 2
            st = L - SPAN_RANGE - sp + 1 if strand == 1 else 10
            out.append(("span sum %d" % tot, [ov(21, st, strand, tot, rlen=rl, span=sp)]))
        if strand == 1:
            for end in (L - SPAN_RANGE - 2, L - SPAN_RANGE - 1, L - SPAN_RANGE, L - SPAN_RANGE + 1):  # seqEnd + 100 at len - 2 .. len + 1
                out.append(("plus, seqEnd %d" % end, [ov(22, end - 149, 1, 300)]))
            for end in (SHORT_LEN - SPAN_RANGE - 1, SHORT_LEN - SPAN_RANGE):  # the allele's own length counts
                out.append(("plus, short allele, seqEnd %d" % end, [ov(8010, end - 99, 1, 200, rlen=100)]))
            # separator (allele 6: N at 330) inside the span, directly beside it on either side
            out.append(("separator inside", [ov(6, 250, 1, 200, rlen=100)]))
            out.append(("separator left of the span", [ov(6, SEPS[6] + 1, 1, 2 * (L - SEPS[6] - 1), rlen=L - SEPS[6] - 1)]))
            out.append(("separator right of the span", [ov(6, SEPS[6] - 100, 1, 200, rlen=100)]))
            out.append(("span ends on the separator", [ov(6, SEPS[6] - 99, 1, 200, rlen=100)]))
        else:
            for start in (SPAN_RANGE - 2, SPAN_RANGE - 1, SPAN_RANGE, SPAN_RANGE + 1):  # seqStart - 100 at -2 .. 1
                out.append(("minus, seqStart %d" % start, [ov(22, start, -1, 300)]))
            out.append(("separator inside", [ov(7, 0, -1, 200, rlen=100)]))
            out.append(("separator left of the span", [ov(7, SEPS[7] + 1, -1, 200, rlen=100)]))
            out.append(("span starts on the separator", [ov(7, SEPS[7], -1, 200, rlen=100)]))
            out.append(("separator right of the span", [ov(7, 0, -1, 2 * SEPS[7], rlen=SEPS[7])]))
        # two tied overlaps: both pass / one of them fails (the whole fragment goes)
        far = 100 if strand == 1 else 200
        out.append(("two pass", [ov(30, ok_start, strand, 300), ov(31, ok_start, strand, 300)]))
        out.append(("second fails", [ov(30, ok_start, strand, 300), ov(31, far, strand, 300)]))
        out.append(("first fails", [ov(30, far, strand, 300), ov(31, ok_start, strand, 300)]))
        out.append(("a worse overlap that would fail is not looked at", [ov(30, ok_start, strand, 300), ov(31, far, strand, 298)]))
    return out


def test_dangling_mate_rule(world):
    """group 8: one mate has no overlap (SeqSet.hpp:2330-2347, 2553-2578): the other's kept overlaps stay only if each has similarity 1, no
    separator in its span, read span + allele span >= 3 * hitLenRequired, and lies within 100 bases of the allele end it points to"""
    w = world
    cases = dangling_cases(w)
    frags = [(c, []) for _, c in cases] + [([], c) for _, c in cases]
    done, rows, flags = run(w, "dangling", frags)
    assert routes(w, done) == {"first-launch", "lds", "unpaired"}
    assert 0 < sum(flags) < len(flags)
    by = {}
    for (label, c), fl in zip(cases, flags):
        by[(label, c[0][5])] = fl
    assert by[("sim 1", 1)] == 1 and by[("sim below 1", 1)] == 0 and by[("span sum %d" % (3 * HIT_LEN - 1), 1)] == 0 and by[("span sum %d" % (3 * HIT_LEN), 1)] == 1
    assert [by[("plus, seqEnd %d" % e, 1)] for e in range(LEN - SPAN_RANGE - 2, LEN - SPAN_RANGE + 2)] == [0, 0, 1, 1]
    assert [by[("minus, seqStart %d" % s, -1)] for s in range(SPAN_RANGE - 2, SPAN_RANGE + 2)] == [1, 1, 0, 0]
    assert by[("separator inside", 1)] == 0 and by[("separator left of the span", 1)] == 1 and by[("two pass", -1)] == 1 and by[("first fails", 1)] == 0
    assert flags[:len(cases)] == flags[len(cases):]  # the mate the overlaps come from does not matter
    # as single ends none of this applies: every fragment is assigned
    done, rows, flags = run(w, "dangling cases as single ends", [(c, []) for _, c in cases], single=True)
    assert all(flags)


def test_truncated_reference_rule(world):
    """group 9 (SeqSet.hpp:2580-2653): next to the kept fragment one list holds an overlap that did not join.  If it has a higher matchCnt than the
    kept fragment's mate of that list -- or the same with a higher similarity on an allele without any fragment -- and its projected mate
    would run off the allele or into a separator, or its similarity exceeds the other mate's by more than 0.1, the fragment goes"""
    w = world
    frags, labels = [], []

    def case(label, extra, side, strand1, m1=250, m2=240, joined_extra=None):
        # the kept fragment: allele 50, mate 1 at 50..199 (plus) and mate 2 at 200..349; a worse joined fragment on allele 51
        l1, l2 = mates([50, 51], [m1, m1 - 4], [m2, m2 - 4], strand1=strand1)
        if joined_extra:
            l1.append(joined_extra[0])
            l2.append(joined_extra[1])
        (l1 if side == 1 else l2).append(extra)
        frags.append((l1, l2))
        labels.append(label)

    for strand1 in (1, -1):
        for side in (1, 2):
            s = strand1 if side == 1 else -strand1        # strand of the list the extra overlap is in
            m_rep = 250 if side == 1 else 240
            # the projected mate of a plus-strand overlap ends 150 bases behind its own end (the kept mates' ends are 150 apart); of a minus-strand one starts 150 before
            for k in (-2, -1, 0, 1):
                if s == 1:
                    start = LEN - 150 - 1 + k - 149   # seqEnd + 150 + 1 == len + k
                else:
                    start = 150 + 1 - k - 1 + 0       # seqStart - 150 - 1 == -k - 1 ... on both sides of -1
                case("higher matchCnt, mate projected %d past the allele" % k, ov(60, start, s, m_rep + 2), side, strand1)
            # into a separator / just short of it
            for k in (-1, 0, 1):
                if s == 1:
                    start = SEPS[6] - 151 + k - 149   # seqEnd + 151 == separator + k   (allele 6)
                    al = 6
                else:
                    start = SEPS[7] + 151 - k         # seqStart - 151 == separator - k   (allele 7)
                    al = 7
                case("higher matchCnt, mate projected %d past a separator" % k, ov(al, start, s, m_rep + 2), side, strand1)
            # similarity against the other mate's + 0.1, on both sides (other mate: 240 / 300 = 0.8 or 250 / 300)
            other = 240 if side == 1 else 250
            for m in (other + 29, other + 30, other + 31):
                case("higher matchCnt, similarity %d / 300 against %d / 300 + 0.1" % (m, other), ov(61, 60 if s == 1 else 190, s, m), side, strand1)
            # equal matchCnt, higher similarity (a shorter read span): on an allele without a fragment, and on one with a (worse) joined fragment
            hs = ov(62, 60 if s == 1 else 190, s, m_rep, rlen=110, span=110)
            case("equal matchCnt, higher similarity, allele not joined", hs, side, strand1)
            lo = ov(62, 60 if s == 1 else 190, s, m_rep, rlen=150)
            case("equal matchCnt, equal similarity, allele not joined", lo, side, strand1)
            # ... the same overlap, its allele joined through a mate in the other list (a fragment far below the best)
            if side == 1:
                j1 = ov(62, 50 if strand1 == 1 else 200, strand1, m_rep, rlen=110, span=110)
                j2 = ov(62, 200 if strand1 == 1 else 50, -strand1, 150)
            else:
                j1 = ov(62, 50 if strand1 == 1 else 200, strand1, 150)
                j2 = ov(62, 200 if strand1 == 1 else 50, -strand1, m_rep, rlen=110, span=110)
            l1, l2 = mates([50, 51], [250, 246], [240, 236], strand1=strand1)
            frags.append((l1 + [j1], l2 + [j2]))
            labels.append("equal matchCnt, higher similarity, allele joined")
    done, rows, flags = run(w, "truncated reference", frags)
    assert routes(w, done) == {"first-launch", "lds", JOINED}
    by = {}
    for label, fl in zip(labels, flags):
        by.setdefault(label, []).append(fl)
    assert 0 < sum(flags) < len(flags), by
    assert by["equal matchCnt, higher similarity, allele not joined"] == [0] * 4 and by["equal matchCnt, higher similarity, allele joined"] == [1] * 4
    assert by["equal matchCnt, equal similarity, allele not joined"] == [1] * 4
    assert by["higher matchCnt, mate projected -2 past the allele"] == [1] * 4 and by["higher matchCnt, mate projected 1 past the allele"] == [0] * 4
    assert by["higher matchCnt, mate projected -1 past a separator"] == [1] * 4 and by["higher matchCnt, mate projected 0 past a separator"] == [0] * 4
    for other in (240, 250):
        assert by["higher matchCnt, similarity %d / 300 against %d / 300 + 0.1" % (other + 29, other)] == [1, 1]
        assert by["higher matchCnt, similarity %d / 300 against %d / 300 + 0.1" % (other + 31, other)] == [0, 0]
    # the same among long lists: the device-memory tables and the replay keep the "allele has a fragment" mark elsewhere
    rng = random.Random(9)
    long_frags = []
    for (l1, l2), label in zip(frags, labels):
        if "equal matchCnt" not in label:
            continue
        s1 = l1[0][5]
        filler = [a for a in range(1000, 1000 + w.lj_cap // 2 + 5)]
        f1, f2 = mates(filler, 200, 200, strand1=s1)
        long_frags.append((l1 + f1, l2 + f2))
        long_frags.append((l1 + f1[:20] + [ov(1000, 60 if s1 == 1 else 210, s1, 190)], l2 + f2[:20]))  # a repeated allele: the replay
    done, rows, flags2 = run(w, "truncated reference, long lists", long_frags)
    assert {"hbm", "replay", JOINED} <= routes(w, done) and 0 < sum(flags2) < len(flags2)


def weight_cases(sim, single):
    """one fragment per matchCnt around every step of Genotyper::ReadAssignmentWeight (205-230): similarity 1 - seg, 1 - 2 seg, 1 - 3 seg with
    seg = max((1 - s) / 4, 0.01), and similarity 1 (no 0.25 adjustment)"""
    den = 300 if single else 600
    seg = max((1 - sim) / 4.0, 0.01)
    ms = sorted(set([den, den - 1] + [int(round(den * (1 - k * seg))) + d for k in (1, 2, 3) for d in (-1, 0, 1)]))
    frags = []
    for k, m in enumerate(ms):
        a = 400 + k
        frags.append(([ov(a, 50, 1, m)], []) if single else ([ov(a, 50, 1, m - m // 2)], [ov(a, 200, -1, m // 2)]))
    return frags


@pytest.mark.parametrize("sim", [0.8, 0.9, 0.97])
def test_row_weights(world, sim):
    """group 10, weights: every step of the weight function for -s 0.8, 0.9 and 0.97 (where the segment clamps to 0.01), with and without an N in
    the reads (a tenth), the 0.25 adjustment when no kept similarity reaches 1"""
    w = world
    for single in (False, True):
        frags = weight_cases(sim, single)
        has_n = [k % 2 for k in range(len(frags))]
        _, rows, flags = run(w, "weights -s %s" % sim, frags + frags, has_n=has_n + [1 - h for h in has_n], sim=sim, single=single)
        assert all(flags) and all(len(r) == 1 for r in rows)
        seen = sorted(set(round(float(r["weight"][0]), 4) for r in rows))
        assert seen == [0.001, 0.01, 0.05, 0.1, 0.5, 1.0], seen
        assert sorted(set(round(float(r["adjust_weight"][0] / r["weight"][0]), 3) for r in rows)) == [0.25, 1.0]
    # several kept fragments, one of them at similarity 1: no adjustment for any; none at 1: 0.25 for all (relaxed keeping makes such rows)
    l1, l2 = mates([500, 501, 502], [300, 299, 298], [300, 299, 300], r1=[300, 300, 300], r2=[300, 300, 300])
    m1, m2 = mates([500, 501, 502], [298, 297, 298], [300, 299, 298], r1=[300, 300, 300], r2=[300, 300, 300])
    _, rows, _ = run(w, "weights of relaxed rows", [(l1, l2), (m1, m2)], has_n=[0, 1], sim=sim, relax=1)
    assert len(rows[0]) == 3 and np.array_equal(rows[0]["weight"], rows[0]["adjust_weight"]) and len(rows[1]) == 3 and np.all(rows[1]["adjust_weight"] < rows[1]["weight"])


def test_set_read_assignments_drops(world):
    """group 10, drops (Genotyper.hpp:778-800): more kept fragments than -n, or a separator inside one of them, empty the row -- the fragment still
    counts as assigned"""
    w = world
    n = 6
    frags = []
    for k in (n - 1, n, n + 1, 3 * n):
        frags.append(mates(list(range(600, 600 + k)), 300, 300))
        frags.append(mates(list(range(600, 600 + k)) + list(range(700, 740)), [300] * k + [290] * 40, 300, strand1=-1))
    frags.append(mates([601, 5], 300, 300))       # allele 5: N at 200, inside 50 .. 349
    frags.append(mates([5], 300, 300))
    frags.append(mates([601, 7], 300, 300))       # allele 7: N at 60, mate 1 covers it
    frags.append(mates([601, 5, 602], [300, 290, 300], 300))  # the fragment over the separator is not kept: the row stays
    frags.append(([ov(6, SEPS[6] - 149, 1, 300)] , [ov(6, SEPS[6] + 1, -1, 2 * (LEN - SEPS[6] - 1), rlen=LEN - SEPS[6] - 1)]))  # the separator between the mates
    done, rows, flags = run(w, "-n and separators", frags, max_assign=n)
    assert all(flags)
    assert [len(r) for r in rows[:8]] == [n - 1, n - 1, n, n, 0, 0, 0, 0] and [len(r) for r in rows[8:]] == [0, 0, 0, 2, 0]
    single = [(a, []) for a, _ in frags]
    done, rows, flags = run(w, "-n and separators, single-end", single, max_assign=n, single=True)
    assert all(flags) and [len(r) for r in rows[:8:2]] == [n - 1, n, 0, 0]
    _, rows0, flags = run(w, "-n 0: no limit", frags[:8], max_assign=0)
    assert [len(r) for r in rows0] == [n - 1, n - 1, n, n, n + 1, n + 1, 3 * n, 3 * n]


def coalesce_expectation(rows, flags):
    """(nGroups, nEntries, assignedFragments) of Genotyper::CoalesceReadAssignments from the oracle's rows: one read group per distinct sorted
    allele pattern (841-908), its entries counted once, and the routine's return value: the fragments that have a row (846-849).  That is the
    sum of the fragmentAssigned flags less the fragments whose row SetReadAssignments dropped (-n, a separator, the whitelist); the flags
    themselves are compared fragment by fragment in compare()."""
    pats = set(tuple(sorted(r["allele_idx"].tolist())) for r in rows if len(r))
    with_row = sum(1 for r in rows if len(r))
    return len(pats), sum(len(p) for p in pats), with_row


def rowset_frags(w, rng):
    """fragments for the rowset form: kept rows of SORT_TILE - 1, SORT_TILE, SORT_TILE + 1 and about twice SORT_TILE entries (every allele of the two
    lists ties the best), small rows that repeat (read groups of several fragments), empty rows, a dangling and an unjoinable fragment"""
    t = w.sort_tile
    pool = [a for a in range(N_ALLELES) if a not in SHORT and a not in SEPS]
    frags = []
    for k in (t - 1, t, t + 1, 2 * t + 37, 1, 2):
        rng.shuffle(pool)
        frags.append(mates(pool[:k], 300, 300, strand1=rng.choice((1, -1))))
        frags.append(random_fragment(rng, 40, 50, best_every=5))
    small = [random_fragment(rng, rng.randrange(1, 60), rng.randrange(1, 60), best_every=3) for _ in range(12)]
    frags += small + small[:5] + [(b, a) for a, b in small[:3]]
    frags.append(([ov(20, LEN - SPAN_RANGE - 149, 1, 300)], []))             # a dangling mate that stays
    frags.append(([ov(20, 50, 1, 300)], [ov(20, 200, 1, 300)]))             # nothing joins
    frags.append(mates([601, 5], 300, 300))                                  # separator: empty row, assigned
    rng.shuffle(pool)
    frags.append(mates(pool[:t + 3], 300, 300))                              # the same large pattern twice: one group
    frags.append(frags[-1])
    return frags


def test_rowset_form(world):
    """group 11: the same kernel writing into a rowset (t1k_pair_into): rows ordered by allele with their place in the reference's order kept aside,
    which t1k_rowset_rows_download undoes -- the rows must equal the oracle's; a whitelist, the raw form, two calls into one rowset at different
    fragment bases; and t1k_rowset_coalesce's counts, which a wrong rank or pattern hash changes"""
    w, rng = world, random.Random(11)
    ctx, orc = w.ctx(0.8, 0, 0)  # -n 0: no limit on the kept fragments
    frags = [(as_list(a, w.alen), as_list(b, w.alen)) for a, b in rowset_frags(w, rng)]
    kept_sizes = set()
    lists = [l for fr in frags for l in fr]
    ctx.reads_upload(["ACGTACGTACGTACGTACGTACGTACGTACGTACGT"] * len(lists))
    ctx.overlaps_upload([len(l) for l in lists], np.concatenate(lists))
    n = len(frags)
    has_n = [k % 3 == 0 for k in range(n)]
    e1, e2 = np.arange(n) * 2, np.arange(n) * 2 + 1
    half = n // 2
    wl = np.array([rng.random() < 0.5 for _ in range(N_ALLELES)], dtype=np.uint8)
    for label, whitelist, raw in (("rowset", None, False), ("rowset, whitelist", wl, False), ("rowset, raw", None, True), ("rowset, raw with a whitelist", wl, True)):
        pad = 7  # fragments of the rowset before and behind the ones paired here: they stay empty
        rs = t1k_amd.Rowset(ctx, n + 2 * pad, whitelist=whitelist, raw=raw)
        # two calls, the later fragments first, both at a fragment base that is not 0
        rs.pair_into(ctx, e1[half:], e2[half:], has_n[half:], frag_base=pad + half)
        rs.pair_into(ctx, e1[:half], e2[:half], has_n[:half], frag_base=pad)
        counts, rows = rs.rows(pad, n)
        assigned = rs.assigned(pad, n)
        exp_rows, exp_flags = compare(label, frags, has_n, orc, counts, assigned, rows, whitelist=None if raw else whitelist, raw=raw)
        c_all, _ = rs.rows()
        assert not c_all[:pad].any() and not c_all[pad + n:].any() and not rs.assigned()[:pad].any()
        if not raw:
            kept_sizes |= set(len(r) for r in exp_rows)
            assert rs.coalesce() == coalesce_expectation(exp_rows, exp_flags), label
        rs.close()
    t = w.sort_tile
    assert {t - 1, t, t + 1, 2 * t + 37} <= kept_sizes, "the rank sort's tile boundary is no longer reached"
    # the context's own rows of the same fragments (the list order of the batch form)
    ctx.pair(e1, e2, has_n)
    compare("rowset fragments, batch form", frags, has_n, orc, *ctx.rows())


def test_reuse_of_stamped_tables(world):
    """group 12: three calls on one context.  The per-workgroup allele tables in device memory are stamped with a fragment epoch and never
    cleared between calls: the first call stamps a set of alleles from both lists in every workgroup that takes a fragment; the later calls
    hold those alleles in one list only (no mate: no fragment), at positions that would join if a stale stamp were believed"""
    w, rng = world, random.Random(12)
    k = w.lj_cap // 2 + 20           # both lists together beyond the LDS table
    stamped = list(range(2000, 2000 + k))
    other = list(range(5000, 5000 + k))
    first = [mates(stamped, [300 if (a + f) % 50 == 0 else 290 for a in stamped], 300, strand1=1 if f % 2 else -1) for f in range(64)]
    done, _, flags = run(w, "reuse: first call", first)
    assert routes(w, done) == {"first-launch", "hbm", JOINED} and all(flags)
    for call in (2, 3):
        frags = []
        for f in range(64):
            s1 = 1 if (f + call) % 2 else -1
            l1, l2 = mates(stamped[:k - 30] + other[:30], 290, 290, strand1=s1)
            m1, m2 = mates(other, [300 if (a + f) % 40 == 0 else 290 for a in other], 300, strand1=s1)
            frags.append((l1[:k - 30] + m1[:30], m2) if (f + call) % 3 else (m1, l2[:k - 30] + m2[:30]))
        frags.append(([l for l in first[0][0]] + [ov(stamped[3], 60, first[0][0][0][5], 300)], first[0][1]))  # and a replay on the same tables
        done, rows, flags = run(w, "reuse: call %d" % call, frags)
        assert {"hbm", JOINED, "replay"} <= routes(w, done) and all(flags)
        assert all(set(r["allele_idx"].tolist()) <= set(other) for r in rows[:-1]), "an allele without a mate in this call has a row entry"


def test_list_form_in_a_child_process(built):
    """the list form of the join: the library decides once per process (T1K_PAIR_LIST) whether mates that both have a list are streamed or
    materialised, so the synthetic groups above run once more in a fresh process that has the variable set; there route() names the form
    "list" and every group asserts it as it asserts "stream" here"""
    import subprocess
    import sys
    if LIST_FORM:
        return  # this process already runs the groups in the list form
    env = dict(os.environ, T1K_PAIR_LIST="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not real_lists and not child_process"],
                       env=env, cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-6000:]


def test_overlaps_upload_refuses_what_does_not_fit(world):
    """t1k_overlaps_upload returns an error for a record outside the packed fields or outside its allele (the kernel would look up separators behind
    the allele's end); the lists uploaded before stay in place"""
    ctx, _ = world.ctx()
    ctx.reads_upload(["ACGTACGTACGTACGTACGTACGTACGTACGTACGT"] * 2)
    good = as_list([ov(20, 50, 1, 300)], world.alen)
    ctx.overlaps_upload([1, 0], good)
    for field, value in (("match_cnt", 4096), ("relaxed_match_cnt", 4096), ("read_end", 1024), ("seq_idx", N_ALLELES), ("seq_end", LEN), ("seq_end", 49), ("seq_start", -1),
                         ("strand", 0), ("left_clip", 1024)):
        bad = good.copy()
        bad[field] = value
        if field == "seq_end" and value == 49:
            bad["seq_start"] = 50  # seqEnd < seqStart
        with pytest.raises(t1k_amd.T1kError):
            ctx.overlaps_upload([1, 0], bad)
    short = as_list([ov(8010, 100, 1, 300)], world.alen)  # 100 .. 249 on an allele of 250 bases
    ctx.overlaps_upload([1, 0], short)
    short["seq_end"] = SHORT_LEN
    with pytest.raises(t1k_amd.T1kError):
        ctx.overlaps_upload([1, 0], short)
