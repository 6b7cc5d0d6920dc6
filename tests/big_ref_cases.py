"""Designed references of 32 768 .. 131 073 sequences for the assign stage's reference-size regimes (DESIGN: reference-size regimes),
in plain Python and numpy, seeded.  tests/test_big_ref_cpu.py proves from the oracle's index and lists that every case hits the edge
it is named for; tests/test_gpu_big_ref.py runs the cases on the GPU.

A reference is a sequence of families that follow each other in allele order.  A family is a random root of L bases and members that
differ from it in up to six variable sites at the two ends (positions 0, L-1, 1, L-2, 2, L-3, in this order: member j carries the
base-4 digits of j there), so all members are distinct and share the window [3, L-3): a read from the window ties across the family.
The plan puts designed families at fixed allele indices; background families of 250 .. 350 members and 64 .. 100 bases fill the rest.

Designed families (those that do not fit below A, in front of the last family, are left out of the case; case["families"] lists the rest):
  low          300 members at 300: the family whose copy is `paralog`
  straddle64   300 members at 32 600 .. 32 899: lists with postings in the chunks 63 and 64 (T1K_SEED_CHUNK = 512)
  small64 / small128 / small255
               12 / 20 / 3 members at 32 900 (chunk 64), 65 580 (chunk 128) and 130 700 (chunk 255) whose k-mers, on either strand,
               occur nowhere else in the reference: no list of a read of theirs has a chunk-directory row
  long320      40 members of 340 bases at 32 912; long320_top: the same in front of the last family (A >= 106 496)
  xlong        30 members of 450 bases at 32 952
  paralog      the low family's root with 7 of the window's 94 bases substituted (about 8 %), 300 members at 65 600
  tie1200      1 200 members of 100 bases at 64 380 .. 65 579, across allele 65 536; tie2100: 2 100 members at 61 000 .. 63 099
  last         the last 300 alleles [A - 300, A): `last_full` when A is a multiple of 512, else `last_partial`
"""
import numpy as np

K = 11
CHUNK = 512
DIR_MINLEN = 32
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = str.maketrans("ACGT", "TGCA")
ROT = {"A": "C", "C": "G", "G": "T", "T": "A"}
CASES = (32768, 32769, 33300, 57344, 57345, 66200, 106496, 106497, 131072)
PARALOG_SUBS = (5, 9, 14, 52, 57, 90, 93)   # window offsets: clean stretches of 37 and 32 bases stay


def revcomp(s):
    return s[::-1].translate(COMP)


def plan_for(A):
    """(name, first allele, members, bases) of the designed families of a reference of A sequences, in allele order"""
    fixed = [("low", 300, 300, 100), ("straddle64", 32600, 300, 80), ("small64", 32900, 12, 90), ("long320", 32912, 40, 340),
             ("xlong", 32952, 30, 450), ("tie2100", 61000, 2100, 100), ("tie1200", 64380, 1200, 100), ("small128", 65580, 20, 90),
             ("paralog", 65600, 300, 100), ("small255", 130700, 3, 90)]
    last = A - 300
    top = [("long320_top", last - 40, 40, 340)] if A >= 106496 else []
    body = [f for f in fixed if f[1] + f[2] <= (top[0][1] if top else last)]
    return sorted(body + top + [("last_full" if A % CHUNK == 0 else "last_partial", last, 300, 80)], key=lambda f: f[1])


def members(root, m):
    """[m, L] base codes: member j of the family of `root`"""
    L = len(root)
    M = np.tile(root, (m, 1))
    j = np.arange(m)
    for d, p in enumerate((0, L - 1, 1, L - 2, 2, L - 3)):
        M[:, p] = (root[p] + ((j >> (2 * d)) & 3)) & 3
    return M


def kmer_codes(M):
    """[m, L - K + 1] codes of the k-mers of every row, and of their reverse complements"""
    n = M.shape[1] - K + 1
    f = np.zeros((M.shape[0], n), dtype=np.int64)
    r = np.zeros((M.shape[0], n), dtype=np.int64)
    for i in range(K):
        f = f << 2 | M[:, i:i + n]
        r = r | (3 - M[:, i:i + n].astype(np.int64)) << (2 * i)
    return f, r


def family_codes(M):
    """the distinct k-mers of a family without looking at every row's window: the root's, and every row's at the variable ends"""
    f, _ = kmer_codes(M[:1])
    a, _ = kmer_codes(M[:, :K + 2])
    b, _ = kmer_codes(M[:, -(K + 2):])
    return np.concatenate([f.ravel(), a.ravel(), b.ravel()])


def make_reference(A, plan, seed):
    """the sequences in allele order, all distinct, and the families as name -> (first allele, members, bases)"""
    rng = np.random.default_rng(seed)
    fams, at = [], 0   # [name, first, members, bases]
    for name, first, m, L in plan:
        assert first >= at, (name, first, at)
        while at < first:   # background families up to the next designed one
            n = min(int(rng.integers(250, 351)), first - at)
            fams.append([None, at, n, int(rng.integers(64, 101))])
            at += n
        fams.append([name, first, m, L])
        at = first + m
    assert at == A, (at, A)
    roots = [None] * len(fams)
    occupied = np.zeros(1 << (2 * K), dtype=bool)
    mats = [None] * len(fams)
    small = [i for i, f in enumerate(fams) if f[0] and f[0].startswith("small")]
    for i, (name, first, m, L) in enumerate(fams):
        if i in small:
            continue
        root = rng.integers(0, 4, L).astype(np.uint8)
        if name == "paralog":
            root = roots[[f[0] for f in fams].index("low")].copy()
            for p in PARALOG_SUBS:
                root[3 + p] = (root[3 + p] + 1) & 3
        roots[i] = root
        mats[i] = members(root, m)
        occupied[family_codes(mats[i])] = True
    for i in small:   # k-mers that occur nowhere else, on either strand: drawn again until none of them is taken
        name, first, m, L = fams[i]
        for _ in range(20000):
            root = rng.integers(0, 4, L).astype(np.uint8)
            M = members(root, m)
            f, r = kmer_codes(M)
            mid = "".join("ACGT"[c] for c in M[m // 2, 3:L - 3])   # the designed reads with edits bring k-mers of their own
            ef, er = kmer_codes(np.array([["ACGT".index(c) for c in e[:L - 7]] for e in edits(mid)], dtype=np.uint8))
            if not (occupied[f].any() or occupied[r].any() or occupied[ef].any() or occupied[er].any()) and len(np.unique(f[0])) == f.shape[1]:
                break
        else:
            raise AssertionError("no free root for " + name)
        roots[i], mats[i] = root, M
        occupied[f.ravel()] = True
        occupied[r.ravel()] = True
    seqs = []
    for M in mats:
        text = ACGT[M]
        seqs += [b.decode() for b in text.view("S%d" % M.shape[1]).ravel().tolist()]
    return seqs, {f[0]: (f[1], f[2], f[3]) for f in fams if f[0]}


def make_case(A, seed=2024):
    plan = plan_for(A)
    seqs, families = make_reference(A, plan, seed + A)
    return {"A": A, "seqs": seqs, "families": families, "seed": seed}


def write_fasta(path, case):
    """one record per sequence; a family's alleles share a gene name only within blocks of 8 100 (names as tests/test_gpu_select_tail.py)"""
    with open(path, "w") as o:
        o.write("".join(">G%d*01:%02d:%02d\n%s\n" % (i // 8100, i // 90 % 90, i % 90 + 1, s) for i, s in enumerate(case["seqs"])))
    return path


def edits(read):
    """the read with two substitutions (at one and two thirds), and with one base deleted in the middle"""
    n = len(read)
    a, b = n // 3, 2 * n // 3
    sub = read[:a] + ROT[read[a]] + read[a + 1:b] + ROT[read[b]] + read[b + 1:]
    return sub, read[:n // 2] + read[n // 2 + 1:]


def read_window(name, L):
    """the part of a member that a designed read covers (0-based, end exclusive)"""
    if name.startswith("tie"):
        return 10, 90          # 80 of the window's 94 bases: every member ties on class
    if name.startswith("long320"):
        return 3, 323          # 320 bases
    if name == "xlong":
        return 20, 420         # 400 bases
    return 3, L - 3


def designed_reads(case):
    """(label, read) for every designed family: its middle member's window forward ("fwd"), reverse-complemented ("rc"), with two
    substitutions ("sub") and with one base deleted ("del"; for long320 these two are 260 and 200 bases long); then about 40 background reads
    ("bg/<allele>", half of them from alleles >= 32 768 where the reference has them) and two reads that match nothing ("none/<n>")"""
    seqs, A = case["seqs"], case["A"]
    rng = np.random.default_rng(case["seed"] + 7 * A)
    out = []
    for name, (first, m, L) in sorted(case["families"].items(), key=lambda kv: kv[1][0]):
        s = seqs[first + m // 2]
        w0, w1 = read_window(name, L)
        read = s[w0:w1]
        out += [(name + "/fwd", read), (name + "/rc", revcomp(read))]
        if name.startswith("long320"):
            sub, _ = edits(s[40:300])
            _, dele = edits(s[100:301])
        else:
            sub, dele = edits(read)
        out += [(name + "/sub", sub), (name + "/del", dele)]
    lo = rng.choice(min(A, 32768), 40 if A < 33000 else 20, replace=False).tolist()   # (a reference that ends at 32 768: all from below)
    hi = (32768 + rng.choice(A - 32768, 20, replace=False)).tolist() if A >= 33000 else []
    for a in lo + hi:
        s = seqs[a]
        read = s[3:len(s) - 3][:150]
        out.append(("bg/%d" % a, read if a % 2 else revcomp(read)))
    for n in range(2):
        out.append(("none/%d" % n, "".join("ACGT"[c] for c in rng.integers(0, 4, 100))))
    return out


def short_reads(reads):
    """the reads of at most 150 bases (a batch of them alone runs the narrow seeding kernel)"""
    return [(l, r) for l, r in reads if len(r) <= 150]


def long_reads(reads):
    """the reads of 161 .. 320 bases (one of them makes its batch run the wide seeding kernel)"""
    return [(l, r) for l, r in reads if 160 < len(r) <= 320]


def pair_mates(case):
    """mates for the pairing test of the 66 200 case: (label, mate 1, mate 2) -- the low family's window against its paralog's, and the
    two ends of tie1200's window"""
    seqs, fam = case["seqs"], case["families"]
    low, par, tie = seqs[fam["low"][0] + 7], seqs[fam["paralog"][0] + 7], seqs[fam["tie1200"][0] + 600]
    return [("low+paralog", low[3:83], revcomp(par[20:97])), ("tie1200", tie[3:73], revcomp(tie[27:97]))]
