"""A designed reference and designed reads for the look-up rule of seeding (tests/seed_ref.py states the rule; tests/test_seed_cpu.py
proves that every case below meets the edge it is named for; tests/test_gpu_seed.py runs them through the kernels).  Pure Python and
seeded: World(k, n_code) is the same on every machine.

The reference is built from PREFIX FAMILIES.  family(R), for a root R of 400 bases, is
    99 full copies of R, made distinct by private random tails, and the prefixes R[:n] for every n in 60 .. 399,
so the list of the k-mer at root offset p has 99 + #{n >= p + k} postings: 439 at the start, one less at every offset from 60 - k on,
... 101, 100, 99 at the offsets 398 - k, 399 - k, 400 - k.  The lengths differ at every offset, so the sum `postings` of a read
identifies WHICH positions of a big run were used: a phase error of one position changes it.

    R1        random, free of repeats; family(R1) and family(revcomp(R1)): a read of R1 is big on both strands
    R2        family(R2) alone: a read of R2 is big as given and finds nothing as its reverse complement.  R2[:REP_END] carries a
              homopolymer of the base an N is coded as and tandem repeats of the periods 2, 3, 5, k/2 + 1 and k/2 + 2 (for k = 11:
              2, 3, 5, 6, 7), each k + 12 bases long, all inside the big region.  (R1 has to stay free of them: a 320-base read of a
              root with repeats would take the kernels' replay, and the scan edges of their parallel form need such reads.)
    variant   99 copies of R2[VAR_A:VAR_B] with one substitution at VAR_SITE and private flanks: the k k-mers over the site have lists
              of exactly 99 postings -- not empty and not big -- and the others of the window 99 more than the family gives them
    B0        one allele with the same kinds of repeats from other units (and a homopolymer of another base): repeats outside a big run
    background  50 random alleles"""
import collections
import random

import seed_ref

ROOT_LEN = 400
COPIES = 99
PREFIX_MIN = 60
MAX_ALLELE = 430
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}

Case = collections.namedtuple("Case", "name kind read meta")


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


class Fresh:
    """random text none of whose k-mers occurs anywhere else in what was generated so far, on either strand: every list length of the
    reference is then what the construction says, at any k.  `core` holds the k-mers of the designed text (roots, repeats, the
    variant), `seen` those and every k-mer handed out."""

    def __init__(self, rng, k):
        self.rng, self.k, self.seen, self.core = rng, k, set(), set()

    def note(self, text):
        """the k-mers of designed text (repeats: they may recur inside it) join the core"""
        for t in (text, seed_ref.revcomp(text)):
            for i in range(len(t) - self.k + 1):
                self.seen.add(t[i:i + self.k])
                self.core.add(t[i:i + self.k])

    def known(self, text):
        return any(text[i:i + self.k] in self.seen for i in range(len(text) - self.k + 1))

    def text(self, n, left="", private=False):
        """n bases that may follow `left`, grown base by base.  private: one of many tails behind the same text -- the k-mers that
        straddle the junction only have to stay out of the core (there are 4 first bases and 99 tails), the ones behind it are new"""
        k = self.k
        for _ in range(1000):  # (at a small k a text can run into a corner where none of the four bases is new: it is begun again)
            out, mine = left, []
            for i in range(n):
                for c in self.rng.sample("ACGT", 4):
                    w = (out + c)[-k:]
                    shared = private and i < k - 1
                    if len(w) < k or (w not in (self.core if shared else self.seen) and seed_ref.revcomp(w) != w):
                        break
                else:
                    break
                out += c
                if len(w) == k:
                    for x in (w, seed_ref.revcomp(w)):
                        if x not in self.seen:
                            self.seen.add(x)
                            mine.append(x)
            else:
                return out[len(left):]
            self.seen.difference_update(mine)
        raise AssertionError("no text of %d bases is left at k = %d" % (n, k))

    def before(self, n, right):
        """n bases that may precede `right`, one of many such flanks (drawn whole until they fit): as text(private=True), mirrored"""
        k = self.k
        while True:
            t = rand_seq(self.rng, n)
            j = t + right[:k - 1]
            ks = [j[i:i + k] for i in range(len(j) - k + 1)]
            inner = ks[:max(0, n - k + 1)]  # wholly inside the flank
            if len(set(ks)) == len(ks) and not any(x in self.core or seed_ref.revcomp(x) in ks for x in ks) and not any(x in self.seen for x in inner):
                for x in ks:
                    self.seen.add(x)
                    self.seen.add(seed_ref.revcomp(x))
                return t


def primitive_unit(rng, d, avoid=()):
    while True:
        u = rand_seq(rng, d)
        rots = [v[j:] + v[:j] for v in (u, seed_ref.revcomp(u)) for j in range(d)]
        if any(r in avoid for r in rots) or any(u == rots[j] for j in range(1, d)):  # the same repeat as another unit's, or a shorter period
            continue
        return u


def repeat_block(fresh, rng, k, periods, homopolymer, avoid=()):
    """text with one tandem repeat of k + 12 bases per period (period 1: of the base `homopolymer`) between random spacers whose ends
    break the period, every k-mer of it new to the reference; -> (text, [(start, end, period)], units)"""
    text = fresh.text(k + 6)
    spans, units = [], []
    for d in periods:
        n = k + 12
        for _ in range(10000):
            u = homopolymer if d == 1 else primitive_unit(rng, d, avoid=tuple(avoid) + tuple(units))
            head = text[:-1] + OTHER[text[-1]] if text[-1] == u[-1] else text  # the base before the repeat must not continue it to the left
            cont = (u * (n // d + 3))[n]                                        # ... nor the one behind it to the right
            new = (u * (n // d + 2))[:n] + OTHER[cont]
            if not fresh.known((head + new)[len(head) - k + 1:]):
                break
            assert d > 1, "the homopolymer's k-mers are taken"
        else:
            raise AssertionError("no new repeat of period %d" % d)
        units.append(u)
        spans.append((len(head), len(head) + n, d))
        text = head + new
        fresh.note(text)
        text += fresh.text(7, left=text)
    fresh.note(text)
    return text, spans, units


class World:
    def __init__(self, k=11, n_code=3, seed=20261):
        rng = random.Random(seed * 100 + k * 4 + n_code)
        fresh = Fresh(rng, k)
        self.k, self.n_code = k, n_code
        self.W = k // 2
        self.W1 = self.W + 1
        self.T = ROOT_LEN - 1 - k  # last root offset whose list is big (100 postings)
        self.periods = sorted({1, 2, 3, 5, self.W1, self.W1 + 1})
        nb = "ACGT"[n_code]
        self.R1 = fresh.text(ROOT_LEN)
        fresh.note(self.R1)
        block, self.spans2, units2 = repeat_block(fresh, rng, k, self.periods, nb)
        self.REP_END = len(block)
        self.R2 = block + fresh.text(ROOT_LEN - len(block), left=block)
        assert len(self.R2) == ROOT_LEN
        fresh.note(self.R2)
        self.VAR_A, self.VAR_B = self.REP_END + 4, self.REP_END + 4 + 100
        self.VAR_SITE = self.VAR_A + 50
        assert self.VAR_B <= ROOT_LEN - 40
        other = "C"  # neither the base of an N nor its complement, at either n_code
        block0, self.spans0, _ = repeat_block(fresh, rng, k, self.periods, other, avoid=units2)
        self.B0 = block0 + fresh.text(60, left=block0)
        fresh.note(self.B0)
        core = self.R2[self.VAR_A:self.VAR_B]
        at = self.VAR_SITE - self.VAR_A
        while True:  # the substituted base: one whose k-mers are new
            self.var_core = core[:at] + rng.choice([c for c in "ACGT" if c != core[at]]) + core[at + 1:]
            if not fresh.known(self.var_core[at - k + 1:at + k]):
                break
        fresh.note(self.var_core)
        names, seqs = [], []

        def add(name, s):
            assert len(s) <= MAX_ALLELE
            names.append(name)
            seqs.append(s)

        self.copy = {}
        for tag, root in (("R1", self.R1), ("R1rc", seed_ref.revcomp(self.R1)), ("R2", self.R2)):
            for i in range(COPIES):
                s = root + fresh.text(MAX_ALLELE - ROOT_LEN, left=root, private=True)
                if i == 0:
                    self.copy[tag] = s
                add("%s*c%03d" % (tag, i), s)
            for n in range(PREFIX_MIN, ROOT_LEN):
                add("%s*p%03d" % (tag, n), root[:n])
        for i in range(COPIES):
            left = fresh.before(20, self.var_core)
            add("V2*v%03d" % i, left + self.var_core + fresh.text(20, left=self.var_core, private=True))
        add("B0*01", self.B0)
        for i in range(50):
            add("BG%d*01" % i, fresh.text(rng.randint(300, MAX_ALLELE)))
        assert len(set(seqs)) == len(seqs)  # no two records are merged by the genotyper's loader
        self.names, self.alleles = names, seqs
        self.fresh = fresh
        self.cases = self._cases(random.Random(seed + 7 * k + n_code))

    def write_fasta(self, path):
        with open(path, "w") as f:
            for n, s in zip(self.names, self.alleles):
                f.write(">%s\n%s\n" % (n, s))
        return path

    # ---- the designed reads ----
    def _cases(self, rng):
        k, W, W1, T = self.k, self.W, self.W1, self.T
        R1, R2 = self.R1, self.R2
        c1, c2 = self.copy["R1"], self.copy["R2"]
        out = []

        def case(name, kind, read, **meta):
            out.append(Case(name, kind, read, meta))

        def sub(s, *xs):
            """substitutions at xs whose k-mers occur nowhere in the reference, on either strand; None where no base does that"""
            for x in xs:
                for c in "ACGT":
                    t = s[:x] + c + s[x + 1:]
                    if c != s[x] and not self.fresh.known(t[max(0, x - k + 1):x + k]):
                        break
                else:
                    return None
                s = t
            return s

        def first(make, candidates):
            """make(v) of the first candidate for which every substitution exists (at a small k the k-mers are crowded)"""
            for v in candidates:
                r = make(v)
                if r is not None and all(x is not None for x in (r if isinstance(r, list) else [r])):
                    return v, r
            raise AssertionError("no candidate admits the substitutions")

        # Threshold: the 101 / 100 / 99 step (root offsets T - 1, T, T + 1) at an interior read offset, the skip counter at the 100 taking
        # every value 0 .. k/2; then the step on the first and on the last k-mer
        for s in range(W1):
            a = T - 1 - s - 3 * W1
            case("threshold_interior_s%d" % s, "threshold_interior", c1[a:ROOT_LEN + 12], at=T - a, skip=s)
        s5 = [sp for sp in self.spans2 if sp[2] == 5][0]
        for s in range(W1):  # ... and the same in a read that is replayed: a period-5 repeat of R2 in front (the junction's k-mers have no list)
            a = T - s - 2 * W1
            head = [h for h in (R2[s5[0] - 9:s5[1] + 9 + j] for j in range(4)) if h[-1] != c1[a - 1]][0]  # (the junction must not continue R1 to the left)
            case("threshold_replay_s%d" % s, "threshold_replay", head + c1[a:ROOT_LEN + 12], at=len(head) + T - a)
        for j, nm in ((-1, "101"), (0, "100"), (1, "99")):
            case("threshold_first_%s" % nm, "threshold_first", c1[T + j:T + j + k + 14], size=100 - j)
            case("threshold_last_%s" % nm, "threshold_last", c1[T + j - 40:T + j + k], size=100 - j)
        # Ends: wholly inside the big region, nk = 1 .. 14 and lengths 150 .. 161: the last k-mer (never skipped) at every phase, and on R1 the
        # strand boundary interrupts the big run at every phase as well
        for nk in range(1, 15):
            case("ends_nk%d" % nk, "ends", R1[100:100 + nk + k - 1], nk=nk)
        for ln in range(150, 162):
            case("ends_len%d" % ln, "ends", R1[90:90 + ln], nk=ln - k + 1)
        for nk in (2, 3, W1, W1 + 1, W1 + 2, 2 * W1 + 1):  # ... and big as given only
            case("ends_r2_nk%d" % nk, "ends", R2[self.REP_END + 10:self.REP_END + 10 + nk + k - 1], nk=nk)
        # Broken runs, each at every phase of the counter (the read's start moves by 0 .. k/2)
        def broken(ph):
            return R1[100 + ph:230 + ph]

        for ds in [()] + [(d,) for d in (1, 3, k - 1, k, k + 1, k + W1, k + W1 + 1)]:
            # the same root position X in every phase: the first from 145 on where the substitutions exist
            X, reads = first(lambda X: [sub(broken(ph), X - 100 - ph, *[X - 100 - ph + d for d in ds]) for ph in range(W1)], range(145, 176))
            for ph in range(W1):
                if ds:
                    case("broken_sub2_d%d_ph%d" % (ds[0], ph), "broken_sub2", reads[ph], x=X - 100 - ph, d=ds[0], phase=ph)
                else:
                    case("broken_sub_ph%d" % ph, "broken_sub", reads[ph], x=X - 100 - ph, phase=ph)
        for ph in range(W1):
            base, x = broken(ph), 45 - ph
            case("broken_n_ph%d" % ph, "broken_n", base[:x] + "N" + base[x + 1:], x=x, phase=ph)
            case("broken_99_ph%d" % ph, "broken_99", self.var_core[ph:], x=self.VAR_SITE - self.VAR_A - ph, phase=ph)
        # Repeats: equal k-mers at distance 1, 2, 3, 5, k/2 + 1 (all replayed) and k/2 + 2 (the edge of the precondition: not replayed), inside a
        # big run (R2: as given; its reverse complement: the run is on the other strand) and outside one (B0)
        for where, src, spans in (("big", R2, self.spans2), ("small", self.B0, self.spans0)):
            for (s, e, d) in spans:
                for shift in (0, 1, 4):
                    a, b = s - k - 1 - shift, e + k + 2
                    r = src[a:b]
                    case("repeat_%s_d%d_sh%d" % (where, d, shift), "repeat", r, d=d, where=where, replay=d <= W1)
                    if shift == 0:
                        case("repeat_%s_d%d_rc" % (where, d), "repeat", seed_ref.revcomp(r), d=d, where=where, replay=d <= W1)
        # N beside a homopolymer of the base its code stands for (R2) and of another base (B0): directly behind the run, directly before it
        for where, src, spans in (("same", R2, self.spans2), ("other", self.B0, self.spans0)):
            (s, e, d) = [sp for sp in spans if sp[2] == 1][0]
            r = src[s - k - 3:e + k + 3]
            lo, hi = k + 3, k + 3 + (e - s)  # the run inside r
            case("n_homopolymer_%s_behind" % where, "n_homopolymer", r[:hi] + "N" + r[hi + 1:], where=where)
            case("n_homopolymer_%s_before" % where, "n_homopolymer", r[:lo - 1] + "N" + r[lo:], where=where)
            case("n_homopolymer_%s_inside" % where, "n_homopolymer", r[:lo + 5] + "N" + r[lo + 6:], where=where)
        # Replay segments: the replay takes 64 positions a pass over the lanes; nk around one and two segments.  Alone (big as given) and with a
        # piece of revcomp(R1) behind it (big on both strands: the counter and prevKmerCode cross the strand boundary in a replay)
        s5 = [sp for sp in self.spans2 if sp[2] == 5][0]
        for nk in (63, 64, 65, 128, 129):
            ln = nk + k - 1
            case("replay_nk%d" % nk, "replay_segment", R2[s5[0] - 20:s5[0] - 20 + ln], nk=nk)
            head = R2[s5[0] - 9:s5[1] + 9]
            case("replay_both_nk%d" % nk, "replay_segment", head + seed_ref.revcomp(R1[150:150 + ln - len(head)]), nk=nk)
        # Scan edges of the parallel form: 320 bases of R1 (the kernels give a lane three consecutive positions of the two strands' nk + nk:
        # wavefronts meet at the combined positions 192 j).  Plain, and with one substitution whose empty stretch ends at / begins behind a
        # wavefront's last position, on either strand
        nkL = 320 - k + 1
        for a in (1, 37, 79):  # (from 1: the reverse complement's last k-mer is then still inside the big region)
            case("scan_plain_a%d" % a, "scan", R1[a:a + 320], nk=nkL)
        for cpos in (190, 191, 192, 193):  # the last empty position as given
            a, r = first(lambda a: sub(R1[a:a + 320], cpos), range(40, 80))
            case("scan_plus_c%d" % cpos, "scan", r, nk=nkL, last_empty=cpos)
        for cpos in (383, 384, 385, 575, 576, 577):  # ... of the reverse complement (combined position nk + p)
            x = 319 - (cpos - nkL)
            if 0 <= x < 320:
                a, r = first(lambda a: sub(R1[a:a + 320], x), range(40, 80))
                case("scan_minus_c%d" % cpos, "scan", r, nk=nkL, last_empty=cpos)
        # Long read-ends (beyond the masks' 320 bases: the sequential kernel), from a full copy of a root with its private tail
        for nm, r in (("r1_321", c1[0:321]), ("r1_430", c1[0:430]), ("r1_tail", c1[60:430]), ("r2_400", c2[0:400]), ("r2rc_350", seed_ref.revcomp(c2[30:380])),
                      ("r1_sub", first(lambda a: sub(c1[a:a + 350], 170), range(10, 40))[1]), ("r1_450", c1[0:430] + self.fresh.text(20, left=c1))):
            case("long_" + nm, "long", r)
        # too short to seed, and exactly one k-mer outside the big region
        case("tiny_lt_k", "tiny", R1[100:100 + k - 1])
        case("tiny_one_base", "tiny", "A")
        case("tiny_eq_k_bg", "tiny", self.alleles[-1][5:5 + k])
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        return out

    def by_kind(self, kind):
        return [c for c in self.cases if c.kind == kind]

    def shapes(self):
        """the three read sets of the kernel shapes: (name, cases) with the read-ends too short to seed between the others"""
        tiny = self.by_kind("tiny")

        def mix(cs):
            res = []
            for i, c in enumerate(cs):
                res.append(c)
                if i % 40 == 7:
                    res.append(tiny[(i // 40) % len(tiny)])
            return res

        short = [c for c in self.cases if c.kind != "tiny" and len(c.read) <= 160]
        mid = [c for c in self.cases if c.kind != "tiny" and len(c.read) <= 320]
        every = [c for c in self.cases if c.kind != "tiny"]
        return [("nw5", mix(short)), ("nw10", mix(mid)), ("xlong", mix(every))]

    def random_reads(self, n, seed):
        """seeded reads with substitutions, Ns and inserted repeats, both orientations, lengths k .. 250"""
        rng = random.Random(seed)
        srcs = [self.copy["R1"], self.copy["R2"], self.B0, self.alleles[-3], self.var_core]
        out = []
        for _ in range(n):
            src = rng.choice(srcs)
            ln = min(len(src), rng.randint(self.k, 250))
            a = rng.randint(0, len(src) - ln)
            r = list(src[a:a + ln])
            for _ in range(rng.choice((0, 0, 1, 2, 4))):
                x = rng.randrange(ln)
                r[x] = OTHER[r[x]] if r[x] in OTHER else "A"
            for _ in range(rng.choice((0, 0, 0, 1, 2))):
                r[rng.randrange(ln)] = "N"
            r = "".join(r)
            if rng.random() < 0.4:  # a tandem repeat of period 1 .. 7 written over a piece of the read
                d = rng.randint(1, 7)
                m = rng.randint(self.k, self.k + 14)
                x = rng.randrange(max(1, ln - m))
                u = rand_seq(rng, d)
                r = (r[:x] + (u * (m // d + 1))[:m] + r[x + m:])[:ln]
            if rng.random() < 0.5:
                r = seed_ref.revcomp(r)
            out.append(r)
        return out


class Expect:
    """a world with its reference written out, the oracle's index behind the list lengths (orc_kmer_postings), and the restatement's
    answer to every read asked for (kept: the tests share them)"""

    def __init__(self, world, d):
        import os
        import util
        self.w = world
        self.fasta = world.write_fasta(os.path.join(d, "seed_k%d_n%d.fa" % (world.k, world.n_code)))
        if world.n_code == 3:  # the genotyper's loader and its N
            assert world.k == 11
            self.orc = util.Oracle(self.fasta)
        else:                  # the extractors': every record kept, N coded as A, any k
            self.orc = util.ExtractOracle(self.fasta, k=world.k, hit_len_required=world.k)
        self._len, self._res = {}, {}

    def list_len(self, kmer):
        if kmer not in self._len:
            self._len[kmer] = self.orc.kmer_len(kmer)
        return self._len[kmer]

    def of(self, read):
        if read not in self._res:
            self._res[read] = seed_ref.seed(read, self.w.k, self.w.n_code, self.list_len)
        return self._res[read]

    def flat(self, read):
        """[(strand, offset, list length)] in the order the kernels keep them"""
        u = self.of(read)["used"]
        return [(0, o, l) for o, l in u[0]] + [(1, o, l) for o, l in u[1]]
