"""The indel table of the analyzer (--indels, t1k_indel_*) restated sequentially, a generator of synthetic record / booking
tables for the kernel test, and a parser / writer of <prefix>_allele_indel.tsv.

The quantity: an event is a maximal run of columns of one gap op (3 deletion, 2 insertion) of a record's edit string that holds neither the
first nor the last column; a run that does is an edge run, whose columns are only counted.  A deletion of L allele bases from p on is (DEL,
p, L); read bases S in front of allele base p are (INS, p, L, S).  Both are shifted left against the allele's bases (an N equals nothing):
  DEL: while p > 0 and allele[p-1] == allele[p+L-1]: p -= 1
  INS: while p > 0 and allele[p-1] == S[-1]: S = allele[p-1] + S[:-1]; p -= 1
A record books every event of its own once per entry of its booking list (uniq 0 / 1), under
  key = ((((g << 2 | type) << 27 | payload) << 1 | strand) << 1) | (1 - uniq),  g = allele_off[allele] + p,
type 0 DEL (payload L), 1 short INS (L <= 13, ACGT only: payload 1 << 2L | the bases), 2 long INS (payload min(L, 2^27 - 1)).

The restatement's form, a Table: .ev = {(g, type, payload, strand): [bookings, uniq bookings]}, the four integers of t1k_indel_stats
(.events, .shifted, .edge_del, .edge_ins) and, for the tests of the generator, .trace: one entry per event of a record."""
import re

import numpy as np

import pileup_ref
import t1k_amd

COLUMNS = ("count", "count_uniq", "fwd", "rev")
HEADER = "#allele\tpos\texon_pos\ttype\tlen\tseq\t" + "\t".join(COLUMNS)
DEL, INS, LONG = 0, 1, 2
SHORT_MAX, PAYLOAD_MAX = 13, (1 << 27) - 1
N = ord("N")
_ACGT = b"ACGT"
_REDUCE = bytes(c if c in _ACGT else N for c in range(256))


class Table:
    def __init__(self):
        self.ev, self.trace = {}, []
        self.events = self.shifted = self.edge_del = self.edge_ins = 0


def reduce(text):
    """bytes with everything but A/C/G/T as N"""
    return (text.tobytes() if isinstance(text, np.ndarray) else pileup_ref.as_bytes(text)).translate(_REDUCE)


def same(a, b):
    return a == b and a != N


def normalise_del(allele, p, length):
    while p > 0 and same(allele[p - 1], allele[p + length - 1]):
        p -= 1
    return p


def normalise_ins(allele, p, seq):
    while p > 0 and same(allele[p - 1], seq[-1]):
        seq = allele[p - 1:p] + seq[:-1]
        p -= 1
    return p, seq


def payload_of(seq):
    """(type, payload) of an insertion's normalised bases"""
    if len(seq) > SHORT_MAX or N in seq:
        return LONG, min(len(seq), PAYLOAD_MAX)
    v = 1
    for b in seq:
        v = v << 2 | _ACGT.index(b)
    return INS, v


def seq_of(payload):
    """the bases of a short insertion's payload"""
    out = []
    while payload > 1:
        out.append(_ACGT[payload & 3])
        payload >>= 2
    return bytes(out[::-1])


def key_of(g, typ, payload, strand, uniq):
    return ((((g << 2 | typ) << 27 | payload) << 1 | strand) << 1) | (1 - uniq)


def runs_by_loops(ops):
    """the gap runs of one edit string, column by column: [(op, first column, columns, allele bases in front, read bases in front)]"""
    out, start, t, p, t0, p0 = [], None, 0, 0, 0, 0
    for c, op in enumerate(ops):
        if start is not None and op != ops[start]:
            out.append((int(ops[start]), start, c - start, t0, p0))
            start = None
        if op in (2, 3) and start is None:
            start, t0, p0 = c, t, p
        if op != 2:
            t += 1
        if op != 3:
            p += 1
    if start is not None:
        out.append((int(ops[start]), start, len(ops) - start, t0, p0))
    return out


def runs_by_regex(ops):
    """the same from the op string"""
    s = "".join("%d" % o for o in ops)
    return [(int(m.group()[0]), m.start(), m.end() - m.start(), m.start() - s.count("2", 0, m.start()), m.start() - s.count("3", 0, m.start()))
            for m in re.finditer(r"2+|3+", s)]


def restate(allele_off, allele_text, aln, strand, book_ptr, book_uniq, text, ops, runs=runs_by_loops):
    off = [int(v) for v in allele_off]
    ref, text = reduce(allele_text), reduce(text)
    ops = np.asarray(ops, np.int8)
    t = Table()
    for i, r in enumerate(aln):
        a, start, read_at, n = int(r["allele"]), int(r["seq_start"]), int(r["read_at"]), int(r["n_ops"])
        allele = ref[off[a]:off[a + 1]]
        mine = [int(u) for u in book_uniq[int(book_ptr[i]):int(book_ptr[i + 1])]]
        e = ops[int(r["ops_at"]):int(r["ops_at"]) + n].tolist()
        assert all(0 <= o <= 3 for o in e)
        for op, col, length, in_t, in_p in runs(e):
            if col == 0 or col + length == n:                       # an edge run
                if op == 3:
                    t.edge_del += length * len(mine)
                else:
                    t.edge_ins += length * len(mine)
                continue
            p = start + in_t
            if op == 3:
                assert p + length <= len(allele)
                q = normalise_del(allele, p, length)
                typ, payload, seq = DEL, length, None
            else:
                raw = text[read_at + in_p:read_at + in_p + length]
                assert len(raw) == length and p <= len(allele)
                q, seq = normalise_ins(allele, p, raw)
                typ, payload = payload_of(seq)
            t.events += 1
            t.shifted += q != p
            t.trace.append((i, col, length, op, p, q, seq))
            x = t.ev.setdefault((off[a] + q, typ, payload, int(strand[i])), [0, 0])
            x[0] += len(mine)
            x[1] += sum(mine)
    t.ev = {k: v for k, v in t.ev.items() if v[0]}                   # (records without a booking have events, and book nothing)
    return t


def restate_by_regex(*args):
    return restate(*args, runs=runs_by_regex)


def stats(t):
    return (t.events, t.shifted, t.edge_del, t.edge_ins)


def expected_runs(t):
    """the runs t1k_indel_get has to return for the Table: (keys, counts), ascending"""
    runs = []
    for (g, typ, payload, strand), (n, u) in t.ev.items():
        runs += [(key_of(g, typ, payload, strand, q), v) for q, v in ((1, u), (0, n - u)) if v]
    runs.sort()
    return [k for k, _ in runs], [v for _, v in runs]


def from_runs(keys, counts):
    """the runs of t1k_indel_get -> .ev of the restatement; a uniq booking is stored once, under the even key"""
    ev = {}
    for k, c in zip(np.asarray(keys).astype(np.uint64).tolist(), np.asarray(counts).astype(np.int64).tolist()):
        assert k < 1 << 63
        x = ev.setdefault((k >> 31, (k >> 29) & 3, (k >> 2) & PAYLOAD_MAX, (k >> 1) & 1), [0, 0])
        x[0] += c
        if (k & 1) == 0:
            x[1] += c
    return ev


def lines(ev, allele_off, seqs, min_count=1):
    """{(allele, pos, type 0 DEL / 1 INS, len, seq): (count, count_uniq, fwd, rev)}: what the file holds, pos as the file prints it"""
    off = np.asarray(allele_off).astype(np.int64)
    cells = {}
    for (g, typ, payload, strand), (n, u) in ev.items():
        a = int(np.searchsorted(off, g, side="right")) - 1
        p = g - int(off[a])
        if typ == DEL:
            k = (a, p + 1, 0, payload, pileup_ref.as_bytes(seqs[a][p:p + payload]).decode())
        elif typ == INS:
            s = seq_of(payload)
            k = (a, p, 1, len(s), s.decode())
        else:
            k = (a, p, 1, payload, "*")
        x = cells.setdefault(k, [0, 0, 0, 0])
        x[0] += n
        x[1] += u
        x[2 + strand] += n
    return {k: tuple(v) for k, v in cells.items() if v[0] >= min_count}


def table_text(names, seqs, exon_masks, rows):
    """the file the analyzer writes: rows = lines(...); by allele, pos, DEL before INS, len, seq"""
    out = [HEADER]
    for k in sorted(rows):
        a, pos, ins, length, seq = k
        mask = exon_masks[a]
        exon = "%d" % int(np.asarray(mask[:pos], np.int64).sum()) if pos >= 1 and mask[pos - 1] else "."
        out.append("%s\t%d\t%s\t%s\t%d\t%s\t%s" % (names[a], pos, exon, "INS" if ins else "DEL", length, seq, "\t".join("%d" % v for v in rows[k])))
    return "\n".join(out) + "\n"


def parse_text_rows(text):
    """the lines behind the header: a row = (allele, pos, exon_pos or None, type, len, seq, {column: value})"""
    text = text.split("\n")
    assert text[-1] == ""
    rows = []
    for line in text[1:-1]:
        f = line.split("\t")
        assert len(f) == 6 + len(COLUMNS) and f[3] in ("DEL", "INS"), line
        rows.append((f[0], int(f[1]), None if f[2] == "." else int(f[2]), f[3], int(f[4]), f[5], dict(zip(COLUMNS, (int(v) for v in f[6:])))))
    return rows


def parse(path):
    """-> (header line, rows)"""
    text = open(path).read()
    return text.split("\n")[0], parse_text_rows(text)


def analyzer_records(asg_ptr, asg, reads1, reads2=None):
    """pileup_ref.to_records (one record per assignment overlap) plus what the analyzer hands to t1k_indel_add: per record its strand and one
    booking, uniq when the fragment has one assignment -> (aln, text, strand, book_ptr, book_uniq).  (The analyzer walks an alignment that
    several assignments share once, with several bookings: the table and the booked edge columns are the same, `events` and `shifted` are not)"""
    aln, text = pileup_ref.to_records(asg_ptr, asg, reads1, reads2)
    strand = []
    for f in range(len(asg_ptr) - 1):
        for a in asg[int(asg_ptr[f]):int(asg_ptr[f + 1])]:
            strand.append(1 if int(a["o1"]["strand"]) == -1 else 0)
            if int(a["has_mate_pair"]) != 0:
                strand.append(1 if int(a["o2"]["strand"]) == -1 else 0)
    assert len(strand) == len(aln)
    return aln, text, np.array(strand, np.uint8), np.arange(len(aln) + 1, dtype=np.uint64), aln["w_uniq"].astype(np.uint8)


def run_around(seq, at):
    """the homopolymer run of seq that holds position `at` (0-based): (first, one behind the last)"""
    lo, hi = at, at + 1
    while lo > 0 and seq[lo - 1] == seq[at]:
        lo -= 1
    while hi < len(seq) and seq[hi] == seq[at]:
        hi += 1
    return lo, hi


def planted_deletion_sample(tmp, at=399, **reads_kw):
    """util.novel_snp_sample's reference; the reads are drawn from a copy in which every allele of the first gene loses the last base of the
    homopolymer run that holds position `at`, with substitution and indel errors on top; genotyped against the ORIGINAL reference
    -> (reference, read prefix, {allele of the gene: (first base of the run, one behind its last)})"""
    import os
    import util
    ref_fa = os.path.join(tmp, "ref.fa")
    util.synth_ref("ref-rna", ref_fa, genes=4, scale=0.05, seed=31)
    recs = util.read_fa(ref_fa)
    gene0 = sorted(set(name.split("*")[0] for name, _, _ in recs))[0]
    mut, runs = os.path.join(tmp, "ref_mut.fa"), {}
    with open(mut, "w") as o:
        for name, head, sq in recs:
            if name.split("*")[0] == gene0 and len(sq) > at + 1:
                lo, hi = run_around(sq, at)
                runs[name] = (lo, hi)
                sq = sq[:hi - 1] + sq[hi:]
            o.write(head + "\n" + sq + "\n")
    pfx = os.path.join(tmp, "r")
    kw = dict(pairs=3000, len=150, seed=5, barcodes=50, sub=0.002, indel=0.002)
    kw.update(reads_kw)
    util.synth_reads(mut, pfx, **kw)
    return ref_fa, pfx, runs


# ---- tables for the kernel -----------------------------------------------------------------------------------------------------------
ALLELE_LEN = (63, 64, 65, 140, 1000, 4097)
HOMOPOLYMER, DINUCLEOTIDE, N_STOP = (20, 28), (50, 62), 80         # of the 140-base allele: A x 8, CA x 6, an N in front of TTTT


def _alleles(rng):
    out = []
    for n in ALLELE_LEN:
        s = np.frombuffer(_ACGT, np.uint8)[rng.integers(0, 4, n)].copy()
        if n >= 140:
            at = 100
            while at + 30 < n:                                      # a homopolymer or a dinucleotide repeat every 60 .. 120 bases, an N now and then
                if rng.random() < 0.5:
                    s[at:at + int(rng.integers(4, 10))] = _ACGT[int(rng.integers(0, 4))]
                else:
                    u = rng.choice(4, 2, replace=False)
                    k = int(rng.integers(3, 7))
                    s[at:at + 2 * k] = np.tile(np.frombuffer(_ACGT, np.uint8)[u], k)
                if rng.random() < 0.3:
                    s[at - 1] = N
                at += int(rng.integers(60, 121))
        if n == 140:
            s[:6] = ord("G")                                        # a shift that reaches p == 0
            s[6], s[19], s[49] = ord("T"), ord("C"), ord("G")
            s[HOMOPOLYMER[0]:HOMOPOLYMER[1]] = ord("A")
            s[HOMOPOLYMER[1]] = ord("G")
            s[DINUCLEOTIDE[0]:DINUCLEOTIDE[1]] = np.tile(np.frombuffer(b"CA", np.uint8), 6)
            s[DINUCLEOTIDE[1]] = ord("T")
            s[N_STOP] = N
            s[N_STOP + 1:N_STOP + 5] = ord("T")
            s[N_STOP + 5] = ord("G")
        out.append(s.tobytes())
    return out


def _random_record(rng, allele, start, columns, p_gap):
    """an alignment of `columns` columns or a few more from allele position `start`: (ops, read bases)"""
    ops, read, t = [], [], start
    while len(ops) < columns:
        u = rng.random()
        if u < p_gap:
            length = int(rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 13, 14, 20]))
            if rng.random() < 0.5 and t + length <= len(allele):
                ops += [3] * length
                t += length
            else:
                how = rng.random()
                if how < 0.4 and t - length >= 0:
                    s = allele[t - length:t]                        # a tandem duplication: it shifts
                elif how < 0.6 and t + length <= len(allele):
                    s = allele[t:t + length]
                else:
                    s = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), length, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
                ops += [2] * length
                read += list(s)
        elif t < len(allele):
            b = allele[t]
            if rng.random() < 0.05:
                ops.append(1)
                read.append(_ACGT[(_ACGT.find(b) + 1 + int(rng.integers(0, 3))) % 4])
            else:
                ops.append(0)
                read.append(b if rng.random() < 0.98 else ord("n"))  # (a byte that is not A/C/G/T: an N)
            t += 1
        else:
            break
    return ops, bytes(read)


def _designed(alleles):
    """records by hand on the 140-base allele (index 3) and the 1000-base one (4): (allele, seq_start, ops, read)"""
    a, b = alleles[3], alleles[4]
    out = []

    def rec(allele_idx, start, parts):
        """parts: ("M", n) matches, ("D", n) a deletion, ("I", bases) an insertion"""
        al = alleles[allele_idx]
        ops, read, t = [], b"", start
        for kind, v in parts:
            if kind == "M":
                ops += [0] * v
                read += al[t:t + v].replace(b"N", b"A")
                t += v
            elif kind == "D":
                ops += [3] * v
                t += v
            else:
                ops += [2] * len(v)
                read += v
        assert t <= len(al)
        out.append((allele_idx, start, ops, read))
    # gap runs against the 64-column seam: ending at column 63, at column 64, starting at column 64
    rec(4, 100, [("M", 60), ("D", 4), ("M", 30)])
    rec(4, 100, [("M", 62), ("D", 3), ("M", 30)])
    rec(4, 100, [("M", 64), ("I", b"GT"), ("M", 30)])
    rec(4, 100, [("M", 61), ("I", b"ACG"), ("M", 30)])
    # a run longer than a whole step: columns 30 .. 149, and a deletion from column 10 to 139
    rec(4, 200, [("M", 30), ("I", bytes(b"ACGT"[i % 4] for i in range(120))), ("M", 40)])
    rec(4, 200, [("M", 10), ("D", 130), ("M", 40)])
    # three events in one step; an insertion touching a deletion, in both orders
    rec(4, 300, [("M", 5), ("D", 1), ("M", 5), ("I", b"G"), ("M", 5), ("D", 2), ("M", 5)])
    rec(4, 300, [("M", 8), ("I", b"TT"), ("D", 3), ("M", 8)])
    rec(4, 300, [("M", 8), ("D", 3), ("I", b"TT"), ("M", 8)])
    # runs at column 0 and at the last column; an edit string that is one gap run
    rec(4, 400, [("D", 2), ("M", 10), ("I", b"AC")])
    rec(4, 400, [("I", b"CCC"), ("M", 10), ("D", 1)])
    rec(4, 400, [("D", 5)])
    rec(4, 400, [("I", b"ACGTA")])
    rec(4, 400, [("I", b"AC"), ("D", 2), ("M", 4)])                 # an edge insertion touching an interior deletion
    # insertions of 13 and of 14 bases, one with an N, and next to the N of the 140-base allele
    rec(4, 500, [("M", 10), ("I", b"ACGTACGTACGTA"), ("M", 10)])
    rec(4, 500, [("M", 10), ("I", b"ACGTACGTACGTAC"), ("M", 10)])
    rec(4, 500, [("M", 10), ("I", b"ACNT"), ("M", 10)])
    rec(3, 70, [("M", N_STOP + 5 - 70), ("I", b"T"), ("M", 20)])     # T behind TTTT: shifts four bases and stops at the N
    # a shift that reaches p == 0 (a G into GGGGGG, a deletion of one of them), a shift longer than the insertion
    rec(3, 0, [("M", 6), ("I", b"G"), ("M", 20)])
    rec(3, 0, [("M", 5), ("D", 1), ("M", 20)])
    rec(3, 10, [("M", HOMOPOLYMER[1] - 10), ("I", b"A"), ("M", 20)])
    rec(3, 10, [("M", HOMOPOLYMER[1] - 10), ("I", b"AA"), ("M", 20)])
    # the same indel at several offsets of one repeat: a deleted A at each of the eight As, CA / AC inserted along the CA repeat
    for k in range(HOMOPOLYMER[0], HOMOPOLYMER[1]):
        rec(3, 5, [("M", k - 5), ("D", 1), ("M", 30)])
    for k in range(DINUCLEOTIDE[0], DINUCLEOTIDE[1] + 1):
        rec(3, 30, [("M", k - 30), ("I", b"CA" if (k - DINUCLEOTIDE[0]) % 2 == 0 else b"AC"), ("M", 30)])
    return out


def generate(seed=1, records=6000):
    """alignments on alleles of 63, 64, 65, 140, 1000 and 4097 bases that hold homopolymers, dinucleotide repeats and Ns: `records` random
    ones (edit strings of 1, 63 .. 66, 128 .. 130 and up to 300 columns; gap runs of 1 .. 5, 13, 14 and 20 columns, insertions that repeat
    the bases in front of them; half of the records inside one 300-base region of the 1000-base allele), then the designed ones of
    _designed().  .strand: 0 / 1; .book_ptr / .book_uniq: 0 .. 5 bookings per record, four records with 256, both uniq values.
    .designed: the index of the first designed record"""
    rng = np.random.default_rng(seed)
    t = pileup_ref.Records()
    alleles = _alleles(rng)
    t.alleles = alleles
    t.allele_len = [len(a) for a in alleles]
    t.allele_off = pileup_ref.offsets(t.allele_len)
    t.allele_text = b"".join(alleles)
    made = []
    lens = [1, 2, 63, 64, 65, 66, 128, 129, 130]
    for _ in range(records):
        n = lens[int(rng.integers(0, len(lens)))] if rng.random() < 0.4 else int(rng.integers(3, 301))
        if rng.random() < 0.5:
            a, start = 4, int(rng.integers(90, 390 - min(n, 250)))
        else:
            a = int(rng.integers(0, len(alleles)))
            start = 0 if rng.random() < 0.2 else int(rng.integers(0, max(1, len(alleles[a]) - n // 2)))
        ops, read = _random_record(rng, alleles[a], start, n, float(rng.choice([0.0, 0.02, 0.05, 0.3])))
        if not ops:
            ops, read = [2], b"A"
        made.append((a, start, ops, read))
    t.designed = len(made)
    made += _designed(alleles)
    recs, ops, text = [], [], []
    at_ops = at_text = 0
    for a, start, e, read in made:
        recs.append((a, start, at_text, at_ops, len(e), 0, 0, 0))
        ops += e
        text.append(read)
        at_ops += len(e)
        at_text += len(read)
    t.aln = np.array(recs, dtype=t1k_amd.PILEUP_ALN_DTYPE)
    t.ops = np.array(ops, np.int8)
    t.text = np.frombuffer(b"".join(text), np.uint8)
    n_rec = len(recs)
    t.strand = rng.integers(0, 2, n_rec).astype(np.uint8)
    n = rng.integers(0, 6, n_rec)
    n[t.designed:] = 1 + np.arange(n_rec - t.designed) % 3           # every designed record books,
    n[[t.designed, t.designed + 4, t.designed + 6]] = 256            # three of them (one, one and three events) 256 times
    t.book_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    t.book_uniq = (rng.random(int(n.sum())) < 0.4).astype(np.uint8)
    t.records = records
    return t


def args(t):
    return (t.allele_off, t.allele_text, t.aln, t.strand, t.book_ptr, t.book_uniq, t.text, t.ops)
