"""The SAM output of the analyzer (--sam, t1k_cigar_batch): the encoder restated in plain loops, an independent decoder
written from the SAM specification, a SAM line parser, the pileup of a SAM file, and the file the analyzer writes for a table of
assignments.

Edit columns: 0 match, 1 mismatch, 2 insert (a read base the allele does not have), 3 delete (an allele base the read does not have)."""
import re

import numpy as np

import pileup_ref

HD = "@HD\tVN:1.6\tSO:unsorted\tGO:query"
PG = "@PG\tID:t1k-analyzer\tPN:analyzer"


# ---- the encoder, column by column --------------------------------------------------------------------------------------------------
def encode(ops, seq_start, allele, clip=(0, 0)):
    """-> (cigar, md, nm, span) of the edit string walked from position seq_start of `allele` (its bases, str or bytes)"""
    allele = allele.decode("ascii") if isinstance(allele, (bytes, bytearray)) else allele
    runs = []                        # CIGAR: maximal runs of one class
    md, matches, in_del = [], 0, False
    t, nm, span = int(seq_start), 0, 0
    for op in ops:
        op = int(op)
        if op not in (0, 1, 2, 3):
            raise ValueError("op %d" % op)
        letter = "M" if op <= 1 else "I" if op == 2 else "D"
        if runs and runs[-1][1] == letter:
            runs[-1][0] += 1
        else:
            runs.append([1, letter])
        if op != 0:
            nm += 1
        if op != 2:
            if not 0 <= t < len(allele):
                raise ValueError("the walk leaves the allele")
            span += 1
        if op == 0:
            matches += 1
        elif op == 1:
            md.append("%d%s" % (matches, allele[t]))
            matches = 0
        elif op == 3:
            md.append(allele[t] if in_del else "%d^%s" % (matches, allele[t]))
            matches = 0
        in_del = op == 3
        if op != 2:
            t += 1
    md.append("%d" % matches)
    if not runs:
        raise ValueError("an empty edit string")
    front, back = int(clip[0]), int(clip[1])
    cigar = ("%dS" % front if front else "") + "".join("%d%s" % (n, c) for n, c in runs) + ("%dS" % back if back else "")
    return cigar, "".join(md), nm, span


# ---- the decoder, from the SAM specification (SAMv1 1.4.6 CIGAR, SAMtags MD) ---------------------------------------------------------
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
_MD = re.compile(r"(\d+)|(\^[A-Za-z]+)|([A-Za-z])")


def cigar_items(cigar):
    items = [(int(n), c) for n, c in _CIGAR.findall(cigar)]
    assert items and "".join("%d%s" % x for x in items) == cigar, cigar
    return items


def decode(cigar, md, seq):
    """-> (ops, reference bases under the alignment).  The CIGAR says which columns consume the read, the reference or both; MD says, for
    the columns that consume the reference, which of them match (a number), which differ (the reference base) and which are deleted
    (^ and the reference bases).  A matching column's reference base is the read's."""
    ref_cols = []                    # per reference-consuming column: ("=", None) | ("X", base) | (group number, base)
    at = 0
    group = 0
    for m in _MD.finditer(md):
        assert m.start() == at, (md, at)
        at = m.end()
        if m.group(1) is not None:
            ref_cols += [("=", None)] * int(m.group(1))
        elif m.group(2) is not None:
            group += 1
            ref_cols += [(group, b) for b in m.group(2)[1:]]
        else:
            ref_cols.append(("X", m.group(3)))
    assert at == len(md) and re.match(r"^\d+(([A-Za-z]|\^[A-Za-z]+)\d+)*$", md), md
    ops, ref = [], []
    q = c = 0
    for n, kind in cigar_items(cigar):
        if kind == "S":
            q += n
        elif kind == "I":
            ops += [2] * n
            q += n
        elif kind == "M":
            for _ in range(n):
                what, base = ref_cols[c]
                assert what in ("=", "X"), (cigar, md)
                ops.append(0 if what == "=" else 1)
                ref.append(seq[q] if what == "=" else base)
                q += 1
                c += 1
        elif kind == "D":
            groups = set()
            for _ in range(n):
                what, base = ref_cols[c]
                assert isinstance(what, int), (cigar, md)
                groups.add(what)
                ops.append(3)
                ref.append(base)
                c += 1
            assert len(groups) == 1 and (c == len(ref_cols) or ref_cols[c][0] != what), (cigar, md)   # one D run = one whole ^ item
        else:
            raise AssertionError("CIGAR operation %s" % kind)
    assert q == len(seq) and c == len(ref_cols), (cigar, md, len(seq))
    return ops, "".join(ref)


# ---- SAM lines ---------------------------------------------------------------------------------------------------------------------
def parse_line(line):
    f = line.split("\t")
    assert len(f) >= 11, line
    tags = {}
    for t in f[11:]:
        name, kind, value = t.split(":", 2)
        tags[name] = int(value) if kind == "i" else value
    return dict(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5], rnext=f[6], pnext=int(f[7]), tlen=int(f[8]), seq=f[9], qual=f[10], tags=tags)


def parse(path):
    """-> (header lines, [(name, length)] of @SQ, records)"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = [l for l in lines[:-1] if l.startswith("@")]
    assert lines[:len(head)] == head
    sq = []
    for l in head:
        if l.startswith("@SQ\t"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            sq.append((f["SN"], int(f["LN"])))
    return head, sq, [parse_line(l) for l in lines[len(head):-1]]


def pileup_from_sam(lines):
    """the 14 counters of the per-base pileup (pileup_ref: A C G T N del ins, all and uniq) booked from POS, CIGAR, SEQ and NH of the
    records, int32 [14, positions] over the @SQ alleles in header order"""
    sq, recs = [], []
    for l in lines:
        if l.startswith("@SQ\t"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            sq.append((f["SN"], int(f["LN"])))
        elif l and not l.startswith("@"):
            recs.append(parse_line(l))
    off, total = {}, 0
    for name, n in sq:
        off[name] = (total, n)
        total += n
    counts = np.zeros((14, total), np.int64)
    for r in recs:
        base, length = off[r["rname"]]
        uniq = 1 if r["tags"]["NH"] == 1 else 0
        start = t = r["pos"] - 1
        q = 0
        consumed = False

        def book(plane, pos):
            assert 0 <= pos < length, r
            counts[plane, base + pos] += 1
            counts[pileup_ref.UNIQ + plane, base + pos] += uniq
        for n, kind in cigar_items(r["cigar"]):
            for _ in range(n):
                if kind == "S":
                    q += 1
                elif kind == "M":
                    book(int(pileup_ref.CODE[ord(r["seq"][q])]), t)
                    t, q, consumed = t + 1, q + 1, True
                elif kind == "D":
                    book(pileup_ref.DEL, t)
                    t, consumed = t + 1, True
                elif kind == "I":
                    book(pileup_ref.INS, min(t - 1 if consumed else start, length - 1))
                    q += 1
                else:
                    raise AssertionError(kind)
        assert q == len(r["seq"])
    return counts.astype(np.int32)


# ---- the file of a table of assignments ---------------------------------------------------------------------------------------------
def mapq(k):
    return 60 if k == 1 else 3 if k == 2 else 1 if k <= 4 else 0


def header(names, seqs):
    return [HD] + ["@SQ\tSN:%s\tLN:%d" % (n, len(s)) for n, s in zip(names, seqs)] + [PG]


def sam_lines(names, seqs, ids, asg_ptr, asg, ops, reads1, reads2=None):
    """the records the analyzer writes for these assignments (tests/pileup_ref.py: the same table), in its order: fragments, their
    assignments, mate 1 before mate 2"""
    paired = reads2 is not None
    out = []
    for f in range(len(asg_ptr) - 1):
        lo, hi = int(asg_ptr[f]), int(asg_ptr[f + 1])
        k = hi - lo
        for hi_idx, a in enumerate(asg[lo:hi], 1):
            mate = int(a["has_mate_pair"]) != 0
            ends = [(a["o1"], 1 if (int(a["o1_from_r2"]) != 0 and not mate) else 0, int(a["ops1"]), int(a["n_ops1"]))]
            if mate:
                ends.append((a["o2"], 1, int(a["ops2"]), int(a["n_ops2"])))
            enc = []
            for o, end, ops_at, n_ops in ends:
                read = pileup_ref.as_bytes((reads2 if end else reads1)[f])
                read = pileup_ref.revcomp(read) if int(o["strand"]) == -1 else read
                clip = (int(o["read_start"]), len(read) - 1 - int(o["read_end"]))
                enc.append(encode(ops[ops_at:ops_at + n_ops], int(o["seq_start"]), seqs[int(a["allele_idx"])], clip) + (read.decode("ascii"),))
            for m, (o, end, _, _) in enumerate(ends):
                cigar, md, nm, span, read = enc[m]
                flag = (0x1 if paired else 0) | (0x10 if int(o["strand"]) == -1 else 0) | (0x100 if hi_idx > 1 else 0)
                rnext, pnext, tlen = "*", 0, 0
                if mate:
                    om, span_m = ends[1 - m][0], enc[1 - m][3]
                    flag |= 0x2 | (0x40 if m == 0 else 0x80) | (0x20 if int(om["strand"]) == -1 else 0)
                    pos, pos_m = int(o["seq_start"]) + 1, int(om["seq_start"]) + 1
                    rnext, pnext = "=", pos_m
                    tlen = max(pos + span - 1, pos_m + span_m - 1) - min(pos, pos_m) + 1
                    if pos > pos_m or (pos == pos_m and m == 1):
                        tlen = -tlen
                elif paired:
                    flag |= 0x8 | (0x80 if end else 0x40)
                out.append("\t".join([ids[f], "%d" % flag, names[int(a["allele_idx"])], "%d" % (int(o["seq_start"]) + 1), "%d" % mapq(k), cigar, rnext, "%d" % pnext, "%d" % tlen,
                                      read, "*", "NM:i:%d" % nm, "MD:Z:" + md, "NH:i:%d" % k, "HI:i:%d" % hi_idx]))
    return out


# ---- record tables for the kernel: tests/pileup_ref.py's generator, with alleles' bases, clips and hand-placed strings ---------------------
def allele_text(allele_len, seed=2, n_rate=0.02):
    rng = np.random.default_rng(seed)
    total = int(sum(allele_len))
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total)].copy()
    text[rng.random(total) < n_rate] = ord("N")
    return text


def restate(aln, ops, allele_off, text, clip=None):
    """encode() over a batch -> dict like Context.cigar_batch's: cigar_ptr, cigar, md_ptr, md (uint8 arenas), nm, ref_span"""
    off = np.asarray(allele_off).astype(np.int64)
    text = bytes(np.asarray(text, np.uint8)) if not isinstance(text, (bytes, bytearray)) else bytes(text)
    cig, md, nm, span = [], [], [], []
    for i, r in enumerate(aln):
        a = int(r["allele"])
        c, m, x, s = encode(ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])], int(r["seq_start"]), text[off[a]:off[a + 1]], (0, 0) if clip is None else clip[i])
        cig.append(c.encode("ascii")); md.append(m.encode("ascii")); nm.append(x); span.append(s)

    def arena(parts):
        ptr = np.zeros(len(parts) + 1, np.uint64)
        ptr[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64) if parts else []
        return ptr, np.frombuffer(b"".join(parts), np.uint8)
    cp, ca = arena(cig)
    mp, ma = arena(md)
    return dict(cigar_ptr=cp, cigar=ca, md_ptr=mp, md=ma, nm=np.array(nm, np.uint32), ref_span=np.array(span, np.uint32))


def hand_strings():
    """edit strings for what can go wrong in a kernel that takes 64 columns a step: (name, ops, where, clip) with where = "start" | "end"
    (the window touches the allele's first / last position)"""
    rng = np.random.default_rng(11)
    out = []

    def add(name, e, where="start", clip=(0, 0)):
        out.append((name, np.asarray(e, np.int8), where, clip))
    for n in (1, 63, 64, 65, 127, 128, 129, 1000):
        add("random %d" % n, rng.choice(4, n, p=[0.7, 0.1, 0.1, 0.1]))
        add("matches %d" % n, [0] * n, "end")
    for cls, other in ((0, 2), (1, 3), (2, 0), (3, 0)):
        for e in (63, 64, 65):                        # a run whose last column is e - 1
            add("run of %d ends at %d" % (cls, e), [other] * (e - 5) + [cls] * 5 + [other] * (130 - e))
        add("run of %d over three steps" % cls, [other] * 60 + [cls] * 140 + [other] * 3)
        for length in (9, 10, 99, 100, 999, 1000):
            add("run of %d x %d" % (length, cls), [other] + [cls] * length + [other], "end")
            add("run of %d x %d alone" % (length, cls), [cls] * length)
    for a, b in ((0, 2), (0, 3), (2, 3), (3, 2), (3, 1), (1, 2), (0, 1)):
        add("%d %d alternating" % (a, b), [a, b] * 64)
        add("%d %d alternating, odd" % (a, b), [a, b] * 64 + [a], "end")
    add("all insert", [2] * 100)
    add("all insert at the end", [2] * 3, "end")
    add("all delete", [3] * 100, "end")
    add("3 2 3", [3, 2, 3])
    for op in (1, 2, 3):
        add("%d first" % op, [op] + [0] * 70)
        add("%d last" % op, [0] * 70 + [op], "end")
        add("%d first and last" % op, [op] + [0] * 62 + [op], "end")
    add("deletion then mismatch", [0, 3, 1, 0])
    add("deletion open over the seam, insert first", [0] * 60 + [3] * 4 + [2] + [3] * 3 + [0] * 10)
    add("deletion over the seam", [0] * 60 + [3] * 8 + [0] * 10)
    add("mismatch run over the seam", [0] * 60 + [1] * 8 + [0] * 10)
    for c in (0, 9, 10, 100, 1000):
        add("clips %d" % c, rng.choice(4, 70, p=[0.7, 0.1, 0.1, 0.1]), "start", (c, 1000 - c if c else 0))
    add("largest clips", [0, 2] * 64, "start", (4294967295, 4294967295))
    return out


class Table:
    pass


def kernel_table(seed=1, records=30000):
    """pileup_ref.generate's records (alleles of 1, 63, 64, 65, 1000 and 4097 bases) with bases for the alleles (N among them) and clips,
    and hand_strings() behind them, on the longest allele"""
    g = pileup_ref.generate(seed=seed, records=records)
    t = Table()
    t.allele_off, t.allele_len = g.allele_off, g.allele_len
    t.text = allele_text(g.allele_len)
    rng = np.random.default_rng(seed + 100)
    pick = np.array([0, 0, 0, 9, 10, 99, 100, 1000, 12345], np.uint32)
    clip = pick[rng.integers(0, len(pick), (len(g.aln), 2))]
    big = int(np.argmax(g.allele_len))
    recs, strings, clips, names = [], [], [], []
    at = len(g.ops)
    for name, e, where, c in hand_strings():
        n_t = int((e != 2).sum())
        recs.append((big, 0 if where == "start" else g.allele_len[big] - n_t, 0, at, len(e), 0, 0, 0))
        strings.append(e)
        clips.append(c)
        names.append(name)
        at += len(e)
    t.aln = np.concatenate([g.aln, np.array(recs, dtype=g.aln.dtype)])
    t.ops = np.concatenate([g.ops] + strings)
    t.clip = np.concatenate([clip, np.array(clips, np.uint32)])
    t.hand = len(g.aln)              # the first hand-placed record
    t.names = names
    return t
