"""Designed references for the index t1k_ref_upload builds (tests/refindex_ref.py restates it): every case is made from a seed, says
what it is for (`what`) and carries in `meta` what tests/test_refindex_cpu.py needs to prove that it is.  tests/test_gpu_refindex.py
holds the kernels to the same cases.

Groups: lengths, rule, n, straddle, order, haspre, dir, transpose.  The rule, n and order cases exist for every world of RULE_WORLDS
(k = 9, 11, 12 with N coded as A and as T) and are the ones compared with the reference's own KmerIndex; the others use the
genotyper's world (k = 11, N coded as T), the straddle case also k = 15."""
import random

import refindex_ref as rr

RULE_WORLDS = [(k, n) for k in (9, 11, 12) for n in (0, 3)]
GENO = (11, 3)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def plain(rng, n, k, avoid=()):
    """n random bases none of whose k-mers repeats inside it or occurs in `avoid` (texts), and that holds no homopolymer of k bases"""
    while True:
        s = rand_seq(rng, n)
        ws = [s[i:i + k] for i in range(max(0, n - k + 1))]
        if len(set(ws)) == len(ws) and not any(w in a for w in ws for a in avoid) and not any(a in s for a in avoid if len(a) <= k):
            return s


class Case:
    def __init__(self, name, group, k, n_code, seqs, what, meta=None, exon=None, vs_reference=False, transpose=True, slices=False):
        self.name, self.group, self.k, self.n_code, self.seqs, self.what = "%s_k%d_n%d" % (name, k, n_code), group, k, n_code, list(seqs), what
        self.kind = name
        self.meta, self.exon, self.vs_reference, self.transpose, self.slices = meta or {}, exon, vs_reference, transpose, slices
        self._ref = {}

    def ref(self, mutation=None):
        """the restatement's index of the case (kept: the tests share it)"""
        if mutation not in self._ref:
            self._ref[mutation] = rr.build(self.seqs, self.k, self.n_code, self.exon, mutation, self.transpose)
        return self._ref[mutation]


# ---- rule, n, order: one set per world -------------------------------------------------------------------------------------------
def rule_cases(k, n_code, seed=1):
    rng = random.Random(seed * 1000 + k * 10 + n_code)
    X = "ACGT"[n_code]            # the base an N is coded as
    Y = "ACGT"[(n_code + 1) & 3]  # another one
    out = []

    def add(name, group, seqs, what, **meta):
        out.append(Case(name, group, k, n_code, seqs, what, meta, vs_reference=True))

    add("rule_all_a", "rule", ["A" * (k + 2) + plain(rng, 6, k), plain(rng, k + 3, k)],
        "an all-A first window is left out (compared with code 0), the second, all-A too, is inserted (i == k), the third is not")
    add("rule_homopolymer", "rule", [b * (2 * k + 3) for b in "ACGT"] + [plain(rng, 5, k) + b * (2 * k + 1) + plain(rng, 5, k) for b in "ACGT"],
        "a run of one base longer than 2k: from the allele's start, and inside an allele where no `i == k` helps")
    add("rule_tandem", "rule", ["AC" * (k + 3), "GT" * (k + 2) + "G", "ACG" * (k + 1), "TTG" * k + "TT"],
        "tandem repeats of period 2 and 3: consecutive windows always differ, every window is posted")
    pal = "AC" + "A" * (k - 4) + "CA"
    add("rule_first_window", "rule", ["A" * (k - 1) + "C" + plain(rng, 4, k), "C" + "A" * (k - 1) + plain(rng, 4, k), "A" * (k - 1) + "T", "T" + "A" * (k - 1),
                                       pal + plain(rng, 3, k), "A" * k, "A" * (k + 1)],
        "first windows that differ from all-A in their first or their last base only (code 1 in one bit order, 4^(k-1) in the other), "
        "one that reads the same in both orders, and all-A alleles of k and k + 1 bases", pal=pal)
    # N
    L = 3 * k + 2
    seqs = []
    for at in ([0], [k - 1], [k], [L - 1], [k + 2, k + 2 + k - 1], [4, 5], [0, L - 1]):
        s = list(plain(rng, L, k))
        for p in at:
            s[p] = "N"
        seqs.append("".join(s))
    add("n_positions", "n", seqs, "an N at offsets 0, k - 1, k and len - 1, two Ns k - 1 apart, two adjacent, one at either end", at=[0, k - 1, k, L - 1])
    head = plain(rng, 5, k)
    add("n_then_same", "n", [head + "N" + b * (k + 3) + plain(rng, 4, k) for b in (X, Y)] + ["N" + b * (k + 2) for b in (X, Y)] + [head + "NN" + X * (k + 1)],
        "an N followed by k and more copies of the base it is coded as: the first valid window equals its invalid predecessor and is left out; "
        "with another base it is inserted; with the N at offset 0 the first valid window is the one `i == k` inserts anyway", X=X, Y=Y, n_at=5)
    # sort order and kMulti
    m1, m2, m3 = (plain(rng, k, k) for _ in range(3))
    while len({m1, m2, m3}) < 3 or any(a[1:] == b[:-1] for a in (m1, m2, m3) for b in (m1, m2, m3)):
        m1, m2, m3 = (plain(rng, k, k) for _ in range(3))
    av = (m1, m2, m3)

    def f(n):
        return plain(rng, n, k, av)

    while True:  # (fillers next to a motif could make another copy of one: the CPU test proves they did not)
        a0 = f(9) + m1 + f(7) + m1 + f(8) + m1 + f(3) + m2 + f(4) + m3
        a1 = f(2) + m1 + f(5) + m2 + f(6) + m3
        a2 = f(3) + m3 + f(1) + m1 + f(20) + m2 + f(12) + m2
        if all(sum(1 for i in range(len(s) - k + 1) if s[i:i + k] == m) == n for s, ns in ((a0, (3, 1, 1)), (a1, (1, 1, 1)), (a2, (1, 2, 1))) for m, n in zip(av, ns)):
            break
    add("order_multi", "order", [a0, a1, a2],
        "a k-mer three times in allele 0 and once in two others (the repeated pair opens the list, and offset order differs from allele order); one "
        "twice in the LAST allele only (the pair closes the list); one once in every allele (kMulti clear)", m1=m1, m2=m2, m3=m3)
    return out


# ---- the others ---------------------------------------------------------------------------------------------------------------------
def lengths_case(seed=2):
    k, n = GENO
    rng = random.Random(seed)
    lens = [0, 1, k - 1, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65, 96]
    order = lens + [32, 0, 64, 96, 0]  # (word-filling alleles next to each other and next to empty ones, an empty one last)
    seqs = [rand_seq(rng, l) for l in order]
    exon = [[rng.randrange(2) for _ in s] for s in seqs]
    return Case("lengths", "lengths", k, n, seqs, "alleles of 0, 1, k - 1, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65 and 96 bases in one reference, with exon masks: "
                "an allele that fills its last word takes one more, and no window crosses from one allele into the next", dict(lens=lens), exon=exon)


def other_letters_case(seed=3):
    k, n = GENO
    rng = random.Random(seed)
    seqs = []
    for letter, at in (("R", 3), ("Y", k), ("K", 20), ("M", 0), ("W", 2 * k)):
        s = list(plain(rng, 2 * k + 6, k))
        s[at] = letter
        seqs.append("".join(s))
    seqs.append(plain(rng, 6, k) + "R" + "T" * (k + 2))  # (coded as T like an N: the first valid window repeats its invalid predecessor)
    return Case("other_letters", "n", k, n, seqs, "letters outside ACGTN are N on the device (include/t1k_gpu.h: `anything else is treated as N`); the reference codes "
                "them as T and keeps their windows valid, so this case is not compared with it")


def straddle_case(k, n_code, seed=4):
    rng = random.Random(seed + k)
    L = 100
    a0 = plain(rng, L, k)

    def with_n(at):
        s = list(plain(rng, L, k))
        for p in at:
            s[p] = "N"
        return "".join(s)

    seqs = [a0, with_n([31 + k]), with_n([31]), with_n([32]), with_n([63, 64]), with_n([31, 32])]
    return Case("straddle", "straddle", k, n_code, seqs, "windows that start at every one of the 32 in-word positions and cross into the next word at every split; Ns in the "
                "last position of a word, the first of the next, and both; `posted` bits 31 and 0 of adjacent words set together and one without the other",
                slices=k > 12)


def haspre_case(seed=5):
    k, n = GENO
    rng = random.Random(seed)
    kp = max(1, k - 2)

    def canon_is_self(t):
        return rr.encode(t) < rr.encode(rr.revcomp(t))

    while True:
        rc_one = rand_seq(rng, k)          # its canonical form is its reverse complement
        p = rand_seq(rng, kp)
        t1, t2 = p + "AC", p + "GT"        # both canonical as they are, one prefix
        absent = rand_seq(rng, k)          # never in the reference: its prefix stays clear
        ok = not canon_is_self(rc_one) and canon_is_self(t1) and canon_is_self(t2) and canon_is_self(absent)
        if ok and len({rr.canonical_prefix(rr.encode(t), k) for t in (rc_one, t1, absent)}) == 3:
            break
    seqs = [rc_one + "A", "C" + t1, t2, rand_seq(rng, k)]
    return Case("haspre", "haspre", k, n, seqs, "a code whose canonical form is its reverse complement, two codes with one canonical (k - 2)-prefix, and a prefix that only "
                "an absent code has", dict(rc_one=rc_one, t1=t1, t2=t2, absent=absent))


def _with_motifs(rng, k, n_alleles, lists, body=None):
    """n_alleles alleles of k + 1 random bases, and for every (motif, alleles) of `lists` the motif appended to those alleles behind
    one more random base"""
    seqs = [rand_seq(rng, k + 1) for _ in range(n_alleles)] if body is None else body
    for m, where in lists:
        for a in where:
            seqs[a] += rand_seq(rng, 1) + m
    return seqs


def dir_cases(seed=6):
    k, n = GENO
    rng = random.Random(seed)
    out = []

    def motif():
        return plain(rng, k, k)

    m32, m33 = motif(), motif()
    out.append(Case("dir_32_33", "dir", k, n, _with_motifs(rng, k, 40, [(m32, range(3, 35)), (m33, range(2, 35))]),
                    "a list of 32 postings (no directory row) beside one of 33 (a row)", dict(m32=m32, m33=m33)))
    for A in (511, 512, 513, 1025):
        last = A - 1
        ma, mb = motif(), motif()
        la = list(range(0, 64, 2)) + [last]                 # 33 postings: chunk 0 and the last allele
        lb = list(range(100, 140))                          # a second row, all in chunk 0
        out.append(Case("dir_A%d" % A, "dir", k, n, _with_motifs(rng, k, A, [(ma, la), (mb, lb)]),
                        "%d alleles: a list with 32 postings in chunk 0 and one in the last allele%s, and a second row" % (
                            A, " (allele 1024 = the first of chunk 2: chunk 1 is empty, its directory cells are equal)" if A == 1025 else ""),
                        dict(A=A, ma=ma, mb=mb, la=la, lb=lb)))
    ml = motif()
    out.append(Case("dir_last_chunk", "dir", k, n, _with_motifs(rng, k, 600, [(ml, range(560, 600))]),
                    "600 alleles: a list whose 40 postings all lie in the last chunk (alleles 512 on)", dict(ml=ml)))
    return out


def dir_two_mask_words_case(seed=7):
    """(its own function: the one case of about a million positions)"""
    k, n = GENO
    rng = random.Random(seed)
    A = 64 * rr.constants()["T1K_SEED_CHUNK"] + 1
    m = plain(rng, k, k)
    body = [rand_seq(rng, k + 1) for _ in range(A - 1)]
    body.append("".join(m + "ACGT"[(i + 1 + rr.BASE[m[0]]) & 3] for i in range(33)))  # (a list of more than 32 postings needs a longer allele than k + 1 bases)
    return Case("dir_two_mask_words", "dir", k, n, body, "64 * 512 + 1 alleles, all but the last of k + 1 bases: kDirMaskWords is 2, and the list of a k-mer that the last "
                "allele alone holds (33 times) has bit 0 of its second mask word set and no other", dict(A=A, m=m))


def transpose_cases(seed=8):
    k, n = GENO
    rng = random.Random(seed)
    out = []
    for A in (63, 64, 65, 129):
        lens = [rng.choice((0, 5, 20, 31, 32, 33, 50, 64, 70, 95)) for _ in range(A)]
        if A >= 64:
            lens[63] = 130  # the longest of block 0 is its last
        if A == 129:
            lens[128] = 97  # a last block of one allele
            lens[64] = 160  # the longest of block 1 is its first
        out.append(Case("transpose_A%d" % A, "transpose", k, n, [rand_seq(rng, l) for l in lens],
                        "%d alleles of unequal lengths: zero words behind every allele's last word, zero columns in a last block of fewer than 64 alleles" % A, dict(A=A)))
    c = out[2]
    out.append(Case("transpose_off", "transpose", k, n, c.seqs, "T1K_REF_TRANSPOSE=0: no basesT / blockT, everything else as in transpose_A65", dict(A=65), transpose=False))
    return out


_kept = {}


def all_cases():
    """every case, made once"""
    if not _kept:
        cs = [c for k, n in RULE_WORLDS for c in rule_cases(k, n)]
        cs += [lengths_case(), other_letters_case(), straddle_case(11, 3), straddle_case(15, 0), haspre_case()] + dir_cases() + [dir_two_mask_words_case()] + transpose_cases()
        assert len({c.name for c in cs}) == len(cs)
        _kept.update((c.name, c) for c in cs)
    return list(_kept.values())


def by_group(group, k=None, n_code=None):
    return [c for c in all_cases() if c.group == group and (k is None or c.k == k) and (n_code is None or c.n_code == n_code)]


def get(name):
    all_cases()
    return _kept[name]
