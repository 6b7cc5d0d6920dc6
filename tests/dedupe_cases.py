"""Inputs for the tests of t1k_dedupe.hip (test_dedupe_cpu.py checks the builder itself, test_gpu_dedupe.py runs the kernels on them).
Everything is drawn from random.Random with a fixed seed: the same batches in every process.

A packed read-end is S = max(2, ceil(longest / 32) + 1) 64-bit words per strand (32 bases a word, one spare word), the N mask likewise; S is
set by the longest read of the upload.  The cases sit where that layout can go wrong: lengths at the word edges, reads that differ in
one base at a word edge or in the N mask alone, reads that differ in their length alone, batches at the edges of S and of the 256-thread
blocks."""
import random

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 159, 160, 161, 319, 320, 321, 999, 1000)
MAX_READ = 1000                                   # t1k_params::max_read_len
N_CODE_BASE = "ACGT"[3]                           # t1k_params::n_base_code = 3: an N is stored with the base bits of T
S_OF_LONGEST = ((31, 2), (32, 2), (33, 3), (320, 11), (321, 12), (1000, 33))
SIZES = (1, 2, 255, 256, 257, 65537)
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def stride(reads):
    """S of an upload of `reads`"""
    longest = max([len(r) for r in reads] + [0])
    return max(2, (longest + 31) // 32 + 1)


def random_seq(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


class Family:
    """A base sequence of L bases and its near twins.

    members   pairwise distinct strings over ACGTN, members[0] the base sequence;
    twins     (i, j, p): members i and j have the same length and differ at position p alone -- p is the first base, the last base,
              index 31 or index 32 (the two sides of the first word edge), each carrying A, C, G, T and N in turn;
    n_pairs   (i, j, p): the twins that carry N_CODE_BASE and N at p: their packed bases are equal, the N mask alone tells them apart;
    longer    indices of the base sequence extended by one A and by 32 A (code 0: the words of the bases are those of the base sequence
              with zeros behind, the length alone differs) -- left out where they would pass MAX_READ;
    aliases   (string, i): the N variant members[i] with a lower-case base or R in place of the N: the same read-end as members[i]"""

    def __init__(self, L):
        rng = random.Random(1000 + L)
        base = random_seq(rng, L)
        self.L, self.base = L, base
        self.members, self.twins, self.n_pairs, self.longer, self.aliases = [base], [], [], [], []
        self.positions = sorted(set(p for p in (0, 31, 32, L - 1) if 0 <= p < L))
        for p in self.positions:
            at = {}
            for c in "ACGTN":
                if c == base[p]:
                    at[c] = 0
                else:
                    at[c] = len(self.members)
                    self.members.append(base[:p] + c + base[p + 1:])
            idx = sorted(at.values())
            self.twins += [(i, j, p) for a, i in enumerate(idx) for j in idx[a + 1:]]
            self.n_pairs.append((at[N_CODE_BASE], at["N"], p))
            for c in (base[p].lower(), "R"):
                self.aliases.append((base[:p] + c + base[p + 1:], at["N"]))
        for k in (1, 32):
            if L + k <= MAX_READ:
                self.longer.append(len(self.members))
                self.members.append(base + "A" * k)


_families = {}


def family(L):
    if L not in _families:
        _families[L] = Family(L)
    return _families[L]


def _mixed(rng, reads):
    """every read once, half of them a second time, shuffled"""
    out = list(reads) + rng.sample(list(reads), len(reads) // 2)
    rng.shuffle(out)
    return out


def family_batch(L):
    """the family of length L as one upload: members and aliases, half of them twice"""
    f = family(L)
    return _mixed(random.Random(1500 + L), f.members + [a for a, _ in f.aliases])


def twin_neighbours(L):
    """the family of length L with every pair of twins side by side (a, b, a), the extended sequences beside the base sequence and every
    alias beside the member it stands for: what must stay apart and what must merge when the word-by-word compare alone decides"""
    f = family(L)
    reads = []
    for i, j, _ in f.twins:
        reads += [f.members[i], f.members[j], f.members[i]]
    for i in f.longer:
        reads += [f.base, f.members[i], f.base]
    for a, i in f.aliases:
        reads += [a, f.members[i], a]
    return reads or [f.base, f.base]


def s_batch(longest):
    """an upload whose longest read has `longest` bases: that family (without the members extended past it) and the families of the short
    lengths, whose reads leave most of their S words spare"""
    reads = []
    for L in LENGTHS:
        if L == longest or (L < longest and L <= 97):
            f = family(L)
            reads += [m for m in f.members if len(m) <= longest] + [a for a, _ in f.aliases]
    return _mixed(random.Random(2000 + longest), reads)


def size_batch(n):
    """n read-ends of 40 bases drawn from about n / 3 sequences"""
    rng = random.Random(3000 + n)
    pool = [random_seq(rng, 40) for _ in range(max(1, n // 3))]
    return [pool[rng.randrange(len(pool))] for _ in range(n)]


def all_identical(n=257):
    return [random_seq(random.Random(3500), 40)] * n


def all_distinct(n=257):
    rng = random.Random(3600)
    seen = []
    while len(seen) < n:
        s = random_seq(rng, 40)
        if s not in seen:
            seen.append(s)
    return seen


def multiplicities():
    """(reads, counts): a shuffle in which sequence k occurs counts[k] times, 1 <= counts[k] <= 300, both ends included"""
    rng = random.Random(3700)
    counts = [1, 300, 2, 299, 255, 256, 257] + [rng.randint(1, 300) for _ in range(13)]
    seqs = all_distinct(len(counts))
    reads = [s for s, c in zip(seqs, counts) for _ in range(c)]
    rng.shuffle(reads)
    return reads, dict(zip(seqs, counts))


def draw_read(rng, alleles, L, errors=True):
    """L bases of an allele that has them, either strand; one time in three with a substitution or two"""
    a = rng.choice([x for x in alleles if len(x) >= L])
    st = rng.randrange(len(a) - L + 1)
    r = a[st:st + L]
    if rng.random() < 0.5:
        r = revcomp(r)
    if errors and L >= 20 and rng.random() < 0.33:
        for _ in range(rng.randint(1, 2)):
            p = rng.randrange(L)
            r = r[:p] + rng.choice([c for c in "ACGT" if c != r[p]]) + r[p + 1:]
    return r


def aligning_reads(alleles, seed, n_distinct, n, lengths, fixed=()):
    """(reads, weights): n read-ends over n_distinct draws from the alleles -- the first of the lengths `fixed`, the others of lengths chosen from
    `lengths` -- every draw used at least once, the rest repeats; weights in 0 .. 5"""
    rng = random.Random(seed)
    drawn = [draw_read(rng, alleles, fixed[i] if i < len(fixed) else rng.choice(lengths)) for i in range(n_distinct)]
    reads = drawn + [rng.choice(drawn) for _ in range(n - n_distinct)]
    rng.shuffle(reads)
    return reads, [rng.randrange(6) for _ in reads]


def expand(reads, weights):
    """the reads with read i repeated weights[i] times: what an upload with weights stands for"""
    return [r for r, w in zip(reads, weights) for _ in range(w)]


# ---- windows for the table across windows ---------------------------------------------------------------------------
XWIN_LONGEST = (150, 1000, 40, 160)   # S = 6, 33, 3, 6
XWIN_REPEATED_LENGTHS = (0, 32, 64, 160)
TWIN_FAMILIES = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97)


def xwin_windows(alleles):
    """Four windows (reads, weights) and the read that window 0 holds 3 times and window 2 holds 5 times.

    window 0 (longest read 150): reads of the alleles, among them the empty read and reads of 32 and 64 bases; the base sequences of
             TWIN_FAMILIES;
    window 1 (longest 1000): a third of window 0's sequences again (the empty read and the reads of 32 and 64 bases among them), reads of
             its own up to 1000 bases with one of 160, and every OTHER member of the families -- near twins of what window 0 holds;
    window 2 (longest 40): sequences of windows 0 and 1 of up to 40 bases again, reads of its own, and of the families of up to 33 bases
             all members and all aliases (a lower-case base or R where window 1 saw N), and near twins of ten earlier short reads;
    window 3 (longest 160): window 1's reads of 160 bases and some of every earlier window again, reads of its own.
    Reads occur several times inside a window; the weights are 0 .. 5.  Every window begins with 40 random bases of its own, so that its
    distinct read-end 0 has an empty list: a linked read-end that took the entry of index 0 shows as one without rows."""
    rng = random.Random(4100)
    out = []
    marked = draw_read(rng, alleles, 40, errors=False)
    # window 0
    r0, _ = aligning_reads(alleles, 4101, 90, 150, (36, 40, 75, 100, 149, 150), fixed=(0, 32, 64, 150, 32, 64, 40, 40))
    fixed0 = [r for r in dict.fromkeys(r0) if len(r) in (0, 32, 64)]
    r0 += [family(L).base for L in TWIN_FAMILIES]
    r0 = [r for r in r0 if r != marked]
    rng.shuffle(r0)
    w0 = [rng.randrange(6) for _ in r0]
    for _ in range(3):
        at = rng.randrange(len(r0) + 1)
        r0.insert(at, marked)
        w0.insert(at, 1)
    out.append((r0, w0))
    # window 1
    d0 = list(dict.fromkeys(r0))
    own1, _ = aligning_reads(alleles, 4102, 60, 90, (36, 40, 100, 150, 321, 640), fixed=(1000, 160, 160, 1000, 999, 40, 32))
    r1 = own1 + fixed0 + rng.sample(d0, len(d0) // 3)
    for L in TWIN_FAMILIES:
        r1 += family(L).members[1:]
    r1 = [r for r in r1 if r != marked]
    rng.shuffle(r1)
    out.append((r1, [rng.randrange(6) for _ in r1]))
    # window 2
    short = [r for r in dict.fromkeys(r0 + r1) if len(r) <= 40 and r != marked]
    own2, _ = aligning_reads(alleles, 4103, 40, 60, (20, 31, 32, 33, 40), fixed=(40, 32))
    r2 = own2 + rng.sample(short, len(short) // 2) + [""]
    for L in TWIN_FAMILIES:
        if L <= 33:
            f = family(L)
            r2 += [m for m in f.members if len(m) <= 40] + [a for a, _ in f.aliases]
    known = set(r0 + r1)
    for s in [r for r in short if 20 <= len(r) < 40][:10]:   # near twins of earlier reads of its own making: they must not link
        p = rng.choice((0, 31, len(s) - 1)) if len(s) > 32 else rng.choice((0, len(s) - 1))
        r2 += [t for t in (s[:p] + rng.choice([c for c in "ACGT" if c != s[p]]) + s[p + 1:], s[:p] + "N" + s[p + 1:], s + "A", s[:-1]) if t not in known]
    r2 = [r for r in r2 if r != marked]
    rng.shuffle(r2)
    w2 = [rng.randrange(6) for _ in r2]
    for _ in range(5):
        at = rng.randrange(len(r2) + 1)
        r2.insert(at, marked)
        w2.insert(at, 1)
    out.append((r2, w2))
    # window 3
    earlier = [r for r in dict.fromkeys(r0 + r1 + r2) if r != marked]
    own3, _ = aligning_reads(alleles, 4104, 30, 40, (40, 100, 150), fixed=(160,))
    r3 = own3 + [r for r in earlier if len(r) == 160] + rng.sample([r for r in earlier if len(r) <= 160], 40) + ["", fixed0[0]]
    rng.shuffle(r3)
    out.append((r3, [rng.randrange(6) for _ in r3]))
    for reads, weights in out:   # every window begins with random bases of its own: distinct read-end 0 has no overlap list
        reads.insert(0, random_seq(rng, 40))
        weights.insert(0, 2)
    return out, marked


def undersized_windows(alleles):
    """1 500 distinct reads of 40 bases, then 500 of them again among 500 new ones"""
    rng = random.Random(4200)
    seen = {}
    while len(seen) < 2000:
        seen.setdefault(draw_read(rng, alleles, 40, errors=True), None)
    seqs = list(seen)
    first, new = seqs[:1500], seqs[1500:]
    second = rng.sample(first, 500) + new
    rng.shuffle(second)
    return first, second


# ---- the job-level sample -----------------------------------------------------------------------------------------
def job_fragments(alleles):
    """paired fragments (mate 1, mate 2) for a run in windows of 8 .. 32 fragments: 8 fragments of 150-base reads; 72 fragments, most of
    1000-base reads, every sixth of 40-base reads, every ninth a copy of one of the first eight; 104 fragments of 40-base reads, every
    other one with the mates of an earlier 40-base fragment (in the other order every fourth time).  A window is cut after 8 fragments
    and then after at most 32: the first has S = 6, the windows cut from the middle part hold a 1000-base read (S = 33), and at
    least one window lies inside the last part (S = 3): a window that begins in the middle part ends at most 31 fragments into the last one."""
    rng = random.Random(4300)

    def frag(L, span):
        a = rng.choice([x for x in alleles if len(x) >= span])
        st = rng.randrange(len(a) - span + 1)
        f = a[st:st + span]
        m1, m2 = f[:L], revcomp(f[-L:])
        return (m1, m2) if rng.random() < 0.5 else (m2, m1)

    frags = [frag(150, 350) for _ in range(8)]
    short = []
    for i in range(72):
        if i % 9 == 4:
            frags.append(frags[rng.randrange(8)])
        elif i % 6 == 1:
            frags.append(frag(40, 200))
            short.append(frags[-1])
        else:
            frags.append(frag(1000, 1400))
    for i in range(104):
        if i % 2:
            m1, m2 = rng.choice(short)
            frags.append((m2, m1) if i % 4 == 1 else (m1, m2))
        else:
            frags.append(frag(40, 200))
    return frags
