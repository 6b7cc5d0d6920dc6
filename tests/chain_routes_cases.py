"""Designed inputs for the routes of the chain stage: small references and single reads built so that the target
(read-end, '+' strand, allele) group leaves t1k_run_chain through one named route, with the hit count of that group computed here
in plain Python.  The constructions (read length, copy count, partial last copy, positions of the edits) and the seeds in SEEDS came
from a search on the CPU; what is committed is its result.

The hit count is exact under two preconditions that tests/test_chain_routes_cpu.py checks for every case: every posting list is
shorter than 100 entries and the read repeats no k-mer within 6 positions (then seeding uses every read offset and a group's hits
are the pairs (read offset, allele offset) with equal k-mers).

What a case claims, and predict() derives from the hit pairs by the predicates of the chain stage:
  n          pairs of equal k-mers between the read and the target allele
  multi      a multi-diagonal group: a hit within RADIUS diagonals of the reference diagonal (the fullest), or more than two beyond
  near_done  k_near_hits writes the hit list: no hit beyond RADIUS, 0 < near hits < 31, the read's window inside the packed text
  simple     ... and the near hits lie on one diagonal, entirely before or behind the reference diagonal's on the read and on the allele
  route      general_lane: n <= 32, or simple and n <= 96; wave_small: n <= 512; wave_large: n <= 4096; big_by_size beyond.
             big_by_scratch is stated by the case (`scratch`): it puts a substitution three bases in front of a deletion of six, so the
             chain meets a gap with bases on both sides whose lengths differ by more than 4, which neither the lane nor the wavefront aligns.
A read of the long class (161 .. 320 bases, NW = 10) is often the short one behind a prefix of the allele with every tenth base
substituted: the prefix keeps the read a read of that allele and adds no hit.
"""
import random

K = 11
RADIUS = 10
GENERAL_SMALL, WAVE_SMALL, WAVE_CAP, BIG_CAP = 32, 512, 4096, 16384
HIT_LEN_REQUIRED = 31
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def postings(seq):
    """k-mer -> allele offsets, by the index's insert rule (a k-mer equal to the one just before it is not inserted again)"""
    out = {}
    prev = "A" * K
    for b in range(len(seq) - K + 1):
        km = seq[b:b + K]
        if km != prev or b == 1:
            out.setdefault(km, []).append(b)
        prev = km
    return out


def hit_pairs(read, allele):
    post = postings(allele)
    return [(a, b) for a in range(len(read) - K + 1) for b in post.get(read[a:a + K], ())]


def preconditions(alleles, reads):
    """(longest posting list over the whole reference, smallest distance at which a read repeats a k-mer on either strand)"""
    lists = {}
    for s in alleles:
        for km, bs in postings(s).items():
            lists[km] = lists.get(km, 0) + len(bs)
    near = 1 << 30
    for r in reads:
        for s in (r, revcomp(r)):
            last = {}
            for a in range(len(s) - K + 1):
                km = s[a:a + K]
                if km in last:
                    near = min(near, a - last[km])
                last[km] = a
    return max(lists.values()), near


def layout(alleles):
    """allele offsets in the packed text and the text's length: every allele starts on a 32-base boundary with a spare position behind it"""
    off, tot = [], 0
    for s in alleles:
        off.append(tot)
        tot += (len(s) + 32) // 32 * 32
    return off, tot + 64


def outcome(hits, d0, alleles, target, nw):
    """the predicates of the module docstring on a group whose reference diagonal is d0"""
    n = len(hits)
    diags = {}
    for a, b in hits:
        diags.setdefault(a - b, []).append((a, b))
    near_d = [d for d in diags if d != d0 and abs(d - d0) <= RADIUS]
    near = sum(len(diags[d]) for d in near_d)
    far = n - len(diags[d0]) - near
    multi = near > 0 or far > 2
    off, total = layout(alleles)
    w0 = off[target] - d0 - RADIUS
    inside = w0 >= 0 and (w0 >> 5) + nw + 3 < (total >> 5) + 7
    near_done = multi and far == 0 and 0 < near < 31 and inside
    simple = False
    if near_done and len(near_d) == 1 and n >= 3 and n * K >= HIT_LEN_REQUIRED:
        h0, h1 = diags[d0], diags[near_d[0]]
        simple = (max(a for a, _ in h0) < min(a for a, _ in h1) and max(b for _, b in h0) < min(b for _, b in h1)) or \
                 (max(a for a, _ in h1) < min(a for a, _ in h0) and max(b for _, b in h1) < min(b for _, b in h0))
    route = None
    if multi:
        if n > WAVE_CAP:
            route = "big_by_size"
        elif n <= GENERAL_SMALL or (simple and n <= 3 * GENERAL_SMALL):
            route = "general_lane"
        else:
            route = "wave_small" if n <= WAVE_SMALL else "wave_large"
    return dict(n=n, multi=multi, near_done=near_done, simple=simple, route=route, near=near, far=far)


def predict(read, alleles, target, nw):
    """the outcome with the fullest diagonal as the reference diagonal (what a case claims), and under `admissible` the (route, near_done,
    simple) of every other choice: seeding takes the diagonal of the first hit that arrives, and any choice is valid"""
    hits = hit_pairs(read, alleles[target])
    count = {}
    for a, b in hits:
        count[a - b] = count.get(a - b, 0) + 1
    if not count:
        return dict(n=0, multi=False, near_done=False, simple=False, route=None, near=0, far=0, admissible=set())
    full = sorted(count, key=lambda d: (-count[d], d))
    out = outcome(hits, full[0], alleles, target, nw)
    alls = [outcome(hits, d, alleles, target, nw) for d in full]
    out["admissible"] = set((o["route"], o["near_done"], o["simple"]) for o in alls)
    out["always_multi"] = all(o["multi"] for o in alls)
    return out


def sub(seg, positions):
    s = list(seg)
    for p in positions:
        s[p] = OTHER[s[p]]
    return "".join(s)


def noisy(seg):
    """every tenth base substituted, the last one included: no k-mer of seg, and none that reaches into it, survives"""
    assert len(seg) % 10 == 0
    return sub(seg, range(9, len(seg), 10))


def deletion(al, at, head, d, tail):
    """head bases of al from `at`, d bases left out, tail bases"""
    return al[at:at + head] + al[at + head + d:at + head + d + tail]


def insertion(al, at, head, d, tail):
    """head bases, d bases that are not the allele's next ones, tail bases"""
    return al[at:at + head] + "".join(OTHER[c] for c in al[at + head:at + head + d]) + al[at + head:at + head + tail]


class Case:
    def __init__(self, name, nw, alleles, target, read, route=None, n=None, near_done=False, simple=False, scratch=False, expect_none=False,
                 single=None, threshold=None, copies=None):
        self.name, self.nw, self.alleles, self.target, self.read = name, nw, alleles, target, read
        self.route, self.n, self.near_done, self.simple, self.scratch = route, n, near_done, simple, scratch
        self.expect_none, self.single, self.threshold, self.copies = expect_none, single, threshold, copies
        # Seeding makes the diagonal of the first hit that arrives the reference diagonal.  Every case keeps at most 30 hits on each diagonal, so
        # that its claim holds for every choice -- except these, which need more than 96 hits in a two-diagonal chain: with the shorter
        # diagonal as the reference the near count saturates and the group is left to k_gather_general
        self.asymmetric = name.startswith(("simple_n96", "simple_n97", "scratch_wave"))
        self.heavy = name == "tandem_le16384_nw10"  # seconds on the GPU: assigned once, not in every variant
        assert (len(read) <= 160) == (nw == 5) and len(read) <= 320, (name, len(read))

    def __repr__(self):
        return "Case(%s)" % self.name


def _ref(rng, lens=(900, 1200, 900)):
    return [rand_seq(rng, n) for n in lens]


PRE = {5: 0, 10: 110}  # bases of noisy prefix that make a short construction a read of the long class


def c_single(nw, rng, kind):
    """one diagonal: at most three mismatches (closed form); one gap with four (the gap walk registers an alignment, the candidate waits
    for it: finish); five such gaps, more than a record has memo references (the group runs again behind the dense DP: retry)"""
    al = _ref(rng)
    L = 150 if nw == 5 else 250
    seg = al[1][300:300 + L]
    if kind == "fast":
        return Case("closed_form_nw%d" % nw, nw, al, 1, sub(seg, (40, 90)), n=L - K + 1 - 2 * K, single="fast")
    if kind == "finish":
        return Case("gap_walk_finish_nw%d" % nw, nw, al, 1, sub(seg, (60, 62, 64, 66)), n=L - K + 1 - (K + 6), single="finish")
    pos = [18 + g * ((L - 30) // 5) + j for g in range(5) for j in (0, 2, 4, 6)]
    return Case("gap_walk_retry_nw%d" % nw, nw, al, 1, sub(seg, pos), n=L - K + 1 - 5 * (K + 6), single="retry")


def c_indel(nw, rng, kind, d):
    """one insertion or deletion of d bases, 25 hits in front of it and 20 behind: whichever diagonal seeding makes the reference, fewer
    than 31 hits lie off it.  d <= RADIUS: two near diagonals in order, a chain; d = 11: the other diagonal is a far stray and the hit
    list comes from the postings"""
    al = _ref(rng)
    front = 25 if d <= RADIUS else 40  # (beyond the radius nothing depends on the reference diagonal; the longer front earns the read an overlap)
    head = front + K - 1
    read = noisy(al[1][400 - PRE[nw]:400]) + (deletion if kind == "D" else insertion)(al[1], 400, head, d, 20 + K - 1)
    n = front + 20
    within = d <= RADIUS
    route = "general_lane" if within else "wave_small"
    return Case("indel_%s%d_nw%d" % (kind, d, nw), nw, al, 1, read, route, n=n, near_done=within, simple=within)


def c_simple(nw, rng, n):
    """a two-diagonal chain (1-base deletion, 20 hits behind it) of n hits: 96 stay with the lane, 97 go to a wavefront"""
    al = _ref(rng)
    head = n - 20 + K - 1
    read = noisy(al[1][400 - PRE[nw]:400]) + deletion(al[1], 400, head, 1, 20 + K - 1)
    return Case("simple_n%d_nw%d" % (n, nw), nw, al, 1, read, "general_lane" if n <= 96 else "wave_small", n=n, near_done=True, simple=True)


def c_simple3(nw, rng):
    """three hits: two k-mers on one diagonal, one behind a 1-base deletion, inside noise.  Too short for an overlap."""
    al = _ref(rng)
    L = 100 if nw == 5 else 200
    read = rand_seq(rng, 30) + deletion(al[1], 500, K + 1, 1, K) + rand_seq(rng, L - 30 - 2 * K - 1)
    return Case("simple_n3_nw%d" % nw, nw, al, 1, read, "general_lane", n=3, near_done=True, simple=True, expect_none=True)


def c_three(nw, rng, n):
    """two deletions: three diagonals within the radius, no two-diagonal chain; 32 hits stay with the lane, 33 go to a wavefront"""
    al = _ref(rng)
    at = 400
    a1 = al[1]
    read = noisy(a1[at - PRE[nw]:at]) + a1[at:at + 25] + a1[at + 26:at + 26 + 19] + a1[at + 47:at + 47 + (n - 24) + K - 1]
    return Case("three_diag_n%d_nw%d" % (n, nw), nw, al, 1, read, "general_lane" if n <= 32 else "wave_small", n=n, near_done=True, simple=False)


def c_near(nw, rng, near):
    """30 hits off the reference diagonal are the most k_near_hits takes; 31 is the saturated count, left to k_gather_general.  Both
    diagonals hold the same number of hits, so it does not matter which of them seeding makes the reference diagonal"""
    al = _ref(rng)
    read = noisy(al[1][400 - PRE[nw]:400]) + deletion(al[1], 400, near + K - 1, 1, near + K - 1)
    ok = near < 31
    return Case("near_count_%d_nw%d" % (near, nw), nw, al, 1, read, "general_lane" if ok else "wave_small", n=2 * near, near_done=ok, simple=ok)


def c_text_start(nw, rng):
    """an indel read on the first allele's first bases: the window of k_near_hits would begin in front of the text"""
    al = _ref(rng)
    head = 60 if nw == 5 else 170
    read = deletion(al[0], 3, head, 1, 20 + K - 1)
    return Case("text_start_nw%d" % nw, nw, al, 0, read, "wave_small", n=head - K + 1 + 20, near_done=False, simple=False)


def c_text_end(nw, rng):
    """... and on the last allele's last bases, hanging over its end.  For reads of at most 160 bases the window's last word always lies
    inside the slack behind the text (that test cannot fire: the group stays with k_near_hits); a read of the long class that begins in
    the text's last four words reaches it."""
    al = _ref(rng)
    m, head = 80, 40  # 30 hits on either side of the deletion
    L = 100 if nw == 5 else 200
    read = deletion(al[2], len(al[2]) - m - 1, head, 1, m - head) + rand_seq(rng, L - m)
    n = head - K + 1 + m - head - K + 1
    gather = nw == 10
    return Case("text_end_nw%d" % nw, nw, al, 2, read, "wave_small" if gather else "general_lane", n=n, near_done=not gather, simple=not gather)


def c_scratch(nw, rng, wave):
    """a deletion of 6 with a substitution three bases in front of it: the chain's gap has 3 bases on the read and 9 on the allele"""
    al = _ref(rng)
    head = 110 if wave else 28 + 3 + K - 1  # (wave: more than 96 hits need more than 30 on one diagonal, see Case.asymmetric)
    seg = deletion(al[1], 400, head, 6, 20 + K - 1)
    read = noisy(al[1][400 - PRE[nw]:400]) + sub(seg, (head - 3,))
    n = head - K + 1 - 3 + 20
    return Case("scratch_%s_nw%d" % ("wave" if wave else "lane", nw), nw, al, 1, read, "big_by_scratch", n=n, near_done=True, simple=True, scratch=True)


def c_gap_job(nw, rng):
    """the same with a deletion of 2: the gap (3 bases on the read, 5 on the allele) fits the register band, so the lane registers the
    alignment in the read-end's memo (the general job list) and k_general_finish adds its match count"""
    al = _ref(rng)
    head = 25 + 3 + K - 1
    read = noisy(al[1][400 - PRE[nw]:400]) + sub(deletion(al[1], 400, head, 2, 20 + K - 1), (head - 3,))
    return Case("gap_job_nw%d" % nw, nw, al, 1, read, "general_lane", n=head - K + 1 - 3 + 20, near_done=True, simple=True)


def c_short_repeat(nw, rng):
    """a repeat of period 5 under the read: its k-mers repeat within 6 positions (the sequential replay of seeding); n is not predicted"""
    unit = "ACGTC"
    L = 140 if nw == 5 else 240
    a1 = rand_seq(rng, 400)
    al = [rand_seq(rng, 400), a1[:200] + unit * 12 + a1[200:], rand_seq(rng, 400)]
    h = (L - 60) // 2
    return Case("short_repeat_nw%d" % nw, nw, al, 1, a1[200 - h:200] + unit * 12 + a1[200:200 + L - 60 - h])


def c_tandem(nw, rng, thr, side, period, copies, partial, read_len, prefix):
    """copies of a random unit (period above the radius) plus `partial` bases of one more; the read is read_len bases of the repeat"""
    unit = rand_seq(rng, period)
    rep = unit * copies + unit[:partial]
    flank = rand_seq(rng, 200)
    al = [rand_seq(rng, 400), flank + rep + rand_seq(rng, 60), rand_seq(rng, 400)]
    read = noisy(flank[200 - prefix:]) + rep[:read_len]
    n = len(hit_pairs(read, al[1]))
    route = "capacity" if n > BIG_CAP else "big_by_size" if n > WAVE_CAP else "wave_large" if n > WAVE_SMALL else "wave_small" if n > GENERAL_SMALL else "general_lane"
    return Case("tandem_%s%d_nw%d" % (side, thr, nw), nw, al, 1, read, route, n=n, threshold=(thr, side), copies=copies + (1 if partial else 0),
                expect_none=False)


def c_many_diagonals(nw, rng):
    """28 copies of a 12-mer under a read of 158 bases: 4096 hits on 41 diagonals, each a run of its own with hits enough for a candidate.
    k_chain_wave and k_chain_big keep at most 32 candidates per group and refuse the range beyond that ("group too large"), where the
    oracle returns overlaps: the limitation this case records"""
    c = c_tandem(nw, rng, 4096, "le", 12, 28, 6, 158, 0)
    c.name, c.route, c.threshold = "many_diagonals_nw%d" % nw, "candidate_cap", None
    return c


# (threshold, class) -> (period, copies, partial, read length, noisy prefix) at or below the threshold and above it.  The search found T and T + 1
# for every pair that exists.  Every diagonal of a tandem repeat with a period above the radius is a run of its own and, with 21 hits or
# more, a candidate; a group may yield 32 (c_many_diagonals), so the counts around 4096 use a period as long as the read (one diagonal per
# copy).  That leaves 32 * 310 hits at most, so exactly 16384 is built with a period of 10: all diagonals chain into ONE run, one
# candidate, and k_chain_big's single lane sorts and filters 16384 hits in one piece (about 12 s: the one slow case, run once).  A read
# of at most 160 bases (150 offsets, posting lists below 100) cannot reach 16384 at all
TANDEM = {
    (32, 5): ((40, 1, 13, 39, 0), (40, 1, 13, 40, 0)),
    (32, 10): ((40, 1, 13, 39, 130), (40, 1, 13, 40, 130)),
    (512, 5): ((12, 7, 9, 84, 0), (12, 7, 8, 85, 0)),
    (512, 10): ((12, 7, 9, 84, 100), (12, 7, 8, 85, 100)),
    (4096, 5): ((160, 27, 56, 160, 0), (160, 27, 57, 160, 0)),
    (4096, 10): ((300, 14, 46, 300, 0), (300, 14, 47, 300, 0)),
    (16384, 10): ((10, 57, 3, 301, 0), (12, 55, 1, 312, 0)),
}


def _registry():
    reg = []
    for nw in (5, 10):
        for kind in ("fast", "finish", "retry"):
            reg.append(("single_%s_nw%d" % (kind, nw), c_single, (nw,), dict(kind=kind)))
        for kind in ("D", "I"):
            for d in (1, 4, 5, 10, 11):
                reg.append(("indel_%s%d_nw%d" % (kind, d, nw), c_indel, (nw,), dict(kind=kind, d=d)))
        for n in (96, 97):
            reg.append(("simple_n%d_nw%d" % (n, nw), c_simple, (nw,), dict(n=n)))
        reg.append(("simple_n3_nw%d" % nw, c_simple3, (nw,), {}))
        for n in (32, 33):
            reg.append(("three_diag_n%d_nw%d" % (n, nw), c_three, (nw,), dict(n=n)))
        for near in (30, 31):
            reg.append(("near_count_%d_nw%d" % (near, nw), c_near, (nw,), dict(near=near)))
        reg.append(("text_start_nw%d" % nw, c_text_start, (nw,), {}))
        reg.append(("text_end_nw%d" % nw, c_text_end, (nw,), {}))
        for wave in (False, True):
            reg.append(("scratch_%s_nw%d" % ("wave" if wave else "lane", nw), c_scratch, (nw,), dict(wave=wave)))
        reg.append(("gap_job_nw%d" % nw, c_gap_job, (nw,), {}))
        reg.append(("short_repeat_nw%d" % nw, c_short_repeat, (nw,), {}))
    reg.append(("many_diagonals_nw5", c_many_diagonals, (5,), {}))
    for (thr, nw), pair in sorted(TANDEM.items()):
        for side, prm in zip(("le", "gt"), pair):
            if prm is None:
                continue
            period, copies, partial, read_len, prefix = prm
            reg.append(("tandem_%s%d_nw%d" % (side, thr, nw), c_tandem, (nw,), dict(thr=thr, side=side, period=period, copies=copies, partial=partial, read_len=read_len, prefix=prefix)))
    return reg


# seed of each case's random sequences: the first from 1000 on at which the case's claims hold exactly (no chance k-mer, no base next to an
# edit that equals the one it replaces), for every choice of the reference diagonal unless the case is asymmetric, and the oracle gives the
# read an overlap
SEEDS = {
    "single_fast_nw5": 1000, "single_finish_nw5": 1000, "single_retry_nw5": 1000, "indel_D1_nw5": 1003, "indel_D4_nw5": 1002, "indel_D5_nw5": 1000,
    "indel_D10_nw5": 1001, "indel_D11_nw5": 1000, "indel_I1_nw5": 1000, "indel_I4_nw5": 1000, "indel_I5_nw5": 1001, "indel_I10_nw5": 1000,
    "indel_I11_nw5": 1027, "simple_n96_nw5": 1000, "simple_n97_nw5": 1001, "simple_n3_nw5": 1000, "three_diag_n32_nw5": 1002,
    "three_diag_n33_nw5": 1002, "near_count_30_nw5": 1000, "near_count_31_nw5": 1001, "text_start_nw5": 1000, "text_end_nw5": 1005,
    "scratch_lane_nw5": 1000, "scratch_wave_nw5": 1001, "short_repeat_nw5": 1000,
    "single_fast_nw10": 1000, "single_finish_nw10": 1000, "single_retry_nw10": 1000, "indel_D1_nw10": 1003, "indel_D4_nw10": 1002, "indel_D5_nw10": 1000,
    "indel_D10_nw10": 1001, "indel_D11_nw10": 1000, "indel_I1_nw10": 1000, "indel_I4_nw10": 1000, "indel_I5_nw10": 1001, "indel_I10_nw10": 1000,
    "indel_I11_nw10": 1001, "simple_n96_nw10": 1000, "simple_n97_nw10": 1001, "simple_n3_nw10": 1000, "three_diag_n32_nw10": 1002,
    "three_diag_n33_nw10": 1002, "near_count_30_nw10": 1000, "near_count_31_nw10": 1001, "text_start_nw10": 1000, "text_end_nw10": 1005,
    "scratch_lane_nw10": 1000, "scratch_wave_nw10": 1001, "short_repeat_nw10": 1000,
    "tandem_le32_nw5": 1001, "tandem_gt32_nw5": 1001, "tandem_le32_nw10": 1001, "tandem_gt32_nw10": 1001, "tandem_le512_nw5": 1000,
    "tandem_gt512_nw5": 1000, "tandem_le512_nw10": 1001, "tandem_gt512_nw10": 1001, "tandem_le4096_nw5": 1000, "tandem_gt4096_nw5": 1000,
    "tandem_le4096_nw10": 1003, "tandem_gt4096_nw10": 1000, "tandem_le16384_nw10": 1000, "tandem_gt16384_nw10": 1000, "many_diagonals_nw5": 1000, "gap_job_nw5": 1000, "gap_job_nw10": 1000,
}


def build(key, seed):
    for k, fn, args, kw in _registry():
        if k == key:
            return fn(*args, random.Random(seed), **kw)
    raise KeyError(key)


def all_cases():
    return [fn(*args, random.Random(SEEDS[k]), **kw) for k, fn, args, kw in _registry()]


def write_fasta(case, path):
    """the case's reference as a file: one gene per allele, so that no two records are merged"""
    with open(path, "w") as f:
        for i, s in enumerate(case.alleles):
            f.write(">G%d*01:0%d\n%s\n" % (i, i + 1, s))
    return path
