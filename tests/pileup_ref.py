"""The per-base pileup of the analyzer (--pileup, t1k_pileup_*) restated sequentially in numpy, a generator of synthetic
alignment tables for the kernel test, and a parser / writer of <prefix>_allele_pileup.tsv.

The quantity: every kept assignment of every assigned fragment contributes its overlap o1 and, with a mate pair, o2.  An overlap's
edit string (0 match, 1 mismatch, 2 insert, 3 delete) is walked from allele position seq_start and read position read_start of the
strand-corrected read-end; ops 0 / 1 book the read base at the allele position, 3 books `del` there, 2 books `ins` at the allele
position consumed last (seq_start if none yet, clamped to the allele's last position).  `all` counts every alignment once, `uniq` only
those of fragments with exactly one assignment.  Table: int [14, positions], row = counter (t1k_amd.PILEUP_COUNTERS), column =
allele_off[a] + p."""
import numpy as np

import t1k_amd

COUNTERS = t1k_amd.PILEUP_COUNTERS
HEADER = "#allele\tpos\texon_pos\tref\t" + "\t".join(COUNTERS)
N, DEL, INS, UNIQ = 4, 5, 6, 7
CODE = np.full(256, N, np.int64)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_KEEP = bytes(c if c in b"ACGT" else ord("N") for c in range(256))


def as_bytes(s):
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


def revcomp(read):
    """the read-end on the other strand; a byte that is not A/C/G/T becomes N"""
    return as_bytes(read).translate(_KEEP).translate(_COMP)[::-1]


def offsets(allele_len):
    off = np.zeros(len(allele_len) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(allele_len, np.uint64))
    return off


def walk(counts, off, length, seq_start, read, p0, ops, w_all=1, w_uniq=0):
    """one alignment, column by column (plain loop): `read` is the strand-corrected read-end, p0 its read_start; counts[:, off + p] is the
    allele's part of the table"""
    t, p, consumed = int(seq_start), int(p0), False
    for op in ops:
        op = int(op)
        if op in (0, 1):
            plane, pos = int(CODE[read[p]]), t
            t, p, consumed = t + 1, p + 1, True
        elif op == 3:
            plane, pos = DEL, t
            t, consumed = t + 1, True
        elif op == 2:
            plane, pos = INS, min(t - 1 if consumed else int(seq_start), length - 1)
            p += 1
        else:
            raise ValueError("op %d" % op)
        if not 0 <= pos < length:
            raise ValueError("the walk leaves the allele")
        counts[plane, off + pos] += w_all
        counts[UNIQ + plane, off + pos] += w_uniq
    return t, p


def to_records(asg_ptr, asg, reads1, reads2=None):
    """(asg_ptr, asg, reads) -> one PILEUP_ALN_DTYPE record per alignment (o1, and o2 with a mate pair; w_all 1, w_uniq 1 when the fragment
    has exactly one assignment; ops_at as in asg) and the text their read_at points into.  o2 is on read 2; o1 on read 2 when o1_from_r2 is
    set on an assignment without a mate pair, else on read 1; strand -1 reads the reverse complement."""
    recs, text, at, size = [], [], {}, 0
    for f in range(len(asg_ptr) - 1):
        lo, hi = int(asg_ptr[f]), int(asg_ptr[f + 1])
        uniq = 1 if hi - lo == 1 else 0
        for a in asg[lo:hi]:
            mate = int(a["has_mate_pair"]) != 0
            ends = [(a["o1"], 1 if (int(a["o1_from_r2"]) != 0 and not mate) else 0, a["ops1"], a["n_ops1"])]
            if mate:
                ends.append((a["o2"], 1, a["ops2"], a["n_ops2"]))
            for o, end, ops_at, n_ops in ends:
                key = (f, end, int(o["strand"]))
                if key not in at:
                    read = as_bytes((reads2 if end else reads1)[f])
                    read = revcomp(read) if key[2] == -1 else read
                    at[key] = size
                    text.append(read)
                    size += len(read)
                recs.append((int(a["allele_idx"]), int(o["seq_start"]), at[key] + int(o["read_start"]), int(ops_at), int(n_ops), 1, uniq, 0))
    aln = np.array(recs, dtype=t1k_amd.PILEUP_ALN_DTYPE) if recs else np.zeros(0, t1k_amd.PILEUP_ALN_DTYPE)
    return aln, b"".join(text)


def book(allele_off, aln, text, ops):
    """the table of the records: every column of every record located by prefix sums inside its record, then np.add.at"""
    off = np.asarray(allele_off).astype(np.int64)
    length = np.diff(off)
    counts = np.zeros((14, int(off[-1])), np.int64)
    text = np.frombuffer(as_bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    ops = np.asarray(ops, np.int8)
    n_ops = aln["n_ops"].astype(np.int64)
    if n_ops.sum() == 0:
        return counts.astype(np.int32)
    rec = np.repeat(np.arange(len(aln)), n_ops)
    first = (np.cumsum(n_ops) - n_ops)[rec]
    col = np.arange(len(rec)) - first
    e = ops[aln["ops_at"].astype(np.int64)[rec] + col].astype(np.int64)
    if ((e < 0) | (e > 3)).any():
        raise ValueError("an op outside 0 .. 3")
    is_t, is_p = (e != 2).astype(np.int64), (e != 3).astype(np.int64)
    ex_t, ex_p = np.cumsum(is_t) - is_t, np.cumsum(is_p) - is_p    # exclusive sums over everything ...
    ex_t, ex_p = ex_t - ex_t[first], ex_p - ex_p[first]             # ... and inside the record
    start = aln["seq_start"].astype(np.int64)[rec]
    alen = length[aln["allele"].astype(np.int64)[rec]]
    pos = start + ex_t
    ins = e == 2
    pos[ins] = np.minimum(np.where(ex_t[ins] > 0, pos[ins] - 1, start[ins]), alen[ins] - 1)
    if ((pos < 0) | (pos >= alen)).any():
        raise ValueError("a walk leaves its allele")
    plane = np.where(e == 3, DEL, INS)
    base = e <= 1
    rp = aln["read_at"].astype(np.int64)[rec] + ex_p
    if (rp[e != 3] >= len(text)).any():
        raise ValueError("a walk leaves the text")
    plane[base] = CODE[text[rp[base]]]
    cell = off[aln["allele"].astype(np.int64)[rec]] + pos
    np.add.at(counts, (plane, cell), aln["w_all"].astype(np.int64)[rec])
    np.add.at(counts, (plane + UNIQ, cell), aln["w_uniq"].astype(np.int64)[rec])
    assert counts.max() < 2 ** 31
    return counts.astype(np.int32)


def restate(asg_ptr, asg, ops, reads1, reads2, allele_len):
    aln, text = to_records(asg_ptr, asg, reads1, reads2)
    return book(offsets(allele_len), aln, text, ops)


def restate_by_loops(asg_ptr, asg, ops, reads1, reads2, allele_len):
    """the same through walk(): every alignment column by column"""
    off = offsets(allele_len).astype(np.int64)
    counts = np.zeros((14, int(off[-1])), np.int64)
    aln, text = to_records(asg_ptr, asg, reads1, reads2)
    for r in aln:
        a = int(r["allele"])
        walk(counts, int(off[a]), int(allele_len[a]), r["seq_start"], text, int(r["read_at"]), ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])], int(r["w_all"]), int(r["w_uniq"]))
    return counts.astype(np.int32)


# ---- assignment tables by hand -----------------------------------------------------------------------------------------------------
def overlap(allele, read_start, read_end, seq_start, seq_end, strand=1):
    return (allele, read_start, read_end, seq_start, seq_end, strand, 0, 0, 0, 0, 1.0)


def assignments(frags):
    """frags: per fragment a list of (allele, o1, ops1[, o2, ops2[, o1_from_r2]]) with o = overlap(...) -> (asg_ptr, asg, ops)"""
    rows, ops, ptr = [], [], [0]
    zero = (0,) * 10 + (0.0,)
    for fr in frags:
        for a in fr:
            allele, o1, e1 = a[0], a[1], list(a[2])
            o2, e2 = (a[3], list(a[4])) if len(a) > 3 and a[3] is not None else (None, [])
            from2 = a[5] if len(a) > 5 else 0
            at1 = len(ops)
            ops += e1
            at2 = len(ops)
            ops += e2
            rows.append((allele, 1 if o2 else 0, from2, 0, o1, o2 or zero, at1, at2, len(e1), len(e2)))
        ptr.append(len(rows))
    asg = np.array(rows, dtype=t1k_amd.FRAG_ASG_DTYPE) if rows else np.zeros(0, t1k_amd.FRAG_ASG_DTYPE)
    return np.array(ptr, np.uint64), asg, np.array(ops, np.int8)


def random_assignments(seed, fragments=300, allele_len=(400, 260, 90), read_len=60):
    """a table of paired fragments with one to three assignments each, gapped edit strings, both strands, some without a mate pair (half
    of those through read 2), Ns in the reads: (asg_ptr, asg, ops, reads1, reads2, allele_len)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTN", np.uint8)

    def read():
        return letters[rng.choice(5, read_len, p=[0.24, 0.24, 0.24, 0.24, 0.04])].tobytes()

    def one(allele):
        n = int(rng.integers(1, read_len + 1))
        e = rng.choice(4, n, p=[0.8, 0.08, 0.06, 0.06])
        n_t, n_p = int((e != 2).sum()), int((e != 3).sum())
        rs = int(rng.integers(0, read_len - n_p + 1))
        ss = int(rng.integers(0, allele_len[allele] - n_t + 1))
        return overlap(allele, rs, rs + n_p - 1, ss, ss + n_t - 1, int(rng.choice([1, -1]))), e.tolist()
    frags, r1, r2 = [], [], []
    for _ in range(fragments):
        r1.append(read())
        r2.append(read())
        fr = []
        for allele in rng.choice(len(allele_len), int(rng.integers(1, 4)), replace=False):
            o1, e1 = one(int(allele))
            if rng.random() < 0.7:
                o2, e2 = one(int(allele))
                fr.append((int(allele), o1, e1, o2, e2))
            else:
                fr.append((int(allele), o1, e1, None, [], int(rng.integers(0, 2))))
        frags.append(fr)
    return assignments(frags) + (r1, r2, list(allele_len))


# ---- record tables for the kernel ------------------------------------------------------------------------------------------------
class Records:
    pass


def generate(seed=1, records=30000, allele_len=(1, 63, 64, 65, 1000, 4097), hot=0.7, text_bytes=1 << 20):
    """records with weights 0 .. 5 (w_uniq <= w_all) on alleles of the given lengths.  Edit strings of 1, 63, 64, 65, 128 and up to 300
    columns; gap columns forced at the first and the last column and across the 64-column seam; all-insert records (one of them behind its
    allele's last position); windows that touch position 0 and the last position; `hot` of the records inside one 200-base region of the
    longest allele; a text with N and other bytes that are not A/C/G/T, one record ending on its last byte."""
    rng = np.random.default_rng(seed)
    t = Records()
    t.allele_len = list(allele_len)
    t.allele_off = offsets(allele_len)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, text_bytes)].copy()
    odd = rng.random(text_bytes) < 0.03
    text[odd] = np.frombuffer(b"NNNnXa-", np.uint8)[rng.integers(0, 7, int(odd.sum()))]
    t.text = text
    big = int(np.argmax(allele_len))
    region = (allele_len[big] // 2, allele_len[big] // 2 + 200)
    lens = [1, 63, 64, 65, 128]
    recs, ops, kinds = [], [], {}
    at = 0
    for i in range(records):
        is_hot = rng.random() < hot
        n = lens[int(rng.integers(0, 5))] if rng.random() < 0.5 else int(rng.integers(1, 201 if is_hot else 301))
        e = rng.choice(4, n, p=[0.86, 0.08, 0.03, 0.03]).astype(np.int8)
        kind = int(rng.integers(0, 12))
        if kind == 0:
            e[0] = 2
        elif kind == 1:
            e[0] = 3
        elif kind == 2:
            e[-1] = 2
        elif kind == 3:
            e[-1] = 3
        elif kind == 4 and n >= 67:
            e[62:66] = 2
        elif kind == 5 and n >= 67:
            e[61:67] = 3
        elif kind == 6 and n >= 129:
            e[126:130] = int(rng.integers(2, 4))
        elif kind == 7 and i % 5 == 0:
            e[:] = 2
        else:
            kind = 11
        kinds[kind] = kinds.get(kind, 0) + 1
        n_t, n_p = int((e != 2).sum()), int((e != 3).sum())
        if is_hot and n_t <= 200:
            allele, ss = big, int(rng.integers(region[0], region[1] - n_t + 1))
        else:
            fits = [a for a, l in enumerate(allele_len) if l >= n_t and l > 0]
            allele = fits[int(rng.integers(0, len(fits)))]
            where = int(rng.integers(0, 4))
            ss = 0 if where == 0 else allele_len[allele] - n_t if where == 1 else int(rng.integers(0, allele_len[allele] - n_t + 1))
        w_all = int(rng.integers(0, 6))
        w_uniq = int(rng.integers(0, w_all + 1))
        read_at = text_bytes - n_p if i == 7 else int(rng.integers(0, text_bytes - n_p + 1))
        recs.append((allele, ss, read_at, at, n, w_all, w_uniq, 0))
        ops.append(e)
        at += n
    t.aln = np.array(recs, dtype=t1k_amd.PILEUP_ALN_DTYPE)
    t.ops = np.concatenate(ops)
    t.kinds = kinds
    t.region = (big, region)
    return t


# ---- <prefix>_allele_pileup.tsv ------------------------------------------------------------------------------------------------------
def table_text(names, seqs, exon_masks, counts):
    """the file the analyzer writes for this table: one line per base of every allele, in order"""
    out = [HEADER]
    at = 0
    for name, sq, mask in zip(names, seqs, exon_masks):
        exonic = 0
        for p, b in enumerate(sq):
            if mask[p]:
                exonic += 1
            out.append("%s\t%d\t%s\t%s\t%s" % (name, p + 1, exonic if mask[p] else ".", b, "\t".join("%d" % v for v in counts[:, at + p])))
        at += len(sq)
    return "\n".join(out) + "\n"


def parse(path):
    """-> (header line, rows): a row = (allele, pos, exon_pos or None, ref, {counter: value})"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    rows = []
    for line in lines[1:-1]:
        f = line.split("\t")
        assert len(f) == 4 + len(COUNTERS), line
        rows.append((f[0], int(f[1]), None if f[2] == "." else int(f[2]), f[3], dict(zip(COUNTERS, (int(v) for v in f[4:])))))
    return lines[0], rows
