"""The support table of the analyzer (--siteSupport, t1k_support_*) restated sequentially in numpy, a generator of synthetic
record / booking / site tables for the kernel test, and a parser / writer of <prefix>_allele_support.tsv.

The quantity: what pileup_ref describes, restricted to a list of sites (allele, 0-based position) and split by the evidence behind each
booking.  A record is a window of a read-end: rec = (read_len, clip_front, strand 0 / 1).  It books once per entry of its booking list, an
entry being (flags = uniq | mate << 1 | orient << 2, t_start, t_end).  A column of state 0 .. 6 (A C G T N - +) that books at a site, at
allele position pos, with c = clip_front + the read bases of the window in front of it, has the end distance d = min(c, L - 1 - c) where it
consumes base c (ops 0, 1, 2) and min(c, L - c) for op 3, saturated at 511.  Its template is told apart by orient and its distances from
the site, dStart = pos - t_start and dEnd = t_end - pos, each clamped to 0 .. 4095.

The restatement's form, a Table: .a = {(site, state, strand, mate, d): [bookings, uniq bookings]} and .b = {(site, state, orient, dStart,
dEnd): bookings}; lines() folds it into what the file holds, {(site, state): (count, count_uniq, fwd, rev, mate1, mate2, end_min, end_med,
near_end, templates)}."""
import numpy as np

import pileup_ref
import sitepile_ref
import t1k_amd

STATES = t1k_amd.SUPPORT_STATES
COLUMNS = ("count", "count_uniq", "fwd", "rev", "mate1", "mate2", "end_min", "end_med", "near_end", "templates")
HEADER = "#allele\tpos\texon_pos\tref\tvar\tobs\t" + "\t".join(COLUMNS)
FAMILY_B = 1 << 57
D_MAX, T_MAX = 511, 4095
ALLELE_LEN = (1, 63, 64, 65, 1000, 4097, 9000)


class Table:
    def __init__(self):
        self.a, self.b = {}, {}


class Hits:
    pass


def hits(allele_off, aln, rec, text, ops, site_allele, site_pos):
    """the columns that book at a site: .rec, .col, .op, .state, .site, .pos (the allele position they book at), .c (clip_front + the read
    bases of the window in front of the column), .d (the saturated end distance) and .raw_d (before saturation)"""
    c = sitepile_ref.columns(allele_off, aln, text, ops)
    is_p = (c.op != 3).astype(np.int64)
    ex_p = np.cumsum(is_p) - is_p
    if len(ex_p):
        ex_p = ex_p - ex_p[np.arange(len(ex_p)) - c.col]
    g = sitepile_ref.site_cells(allele_off, site_allele, site_pos)
    if len(g) == 0:
        keep, idx = np.zeros(len(c.cell), bool), np.zeros(len(c.cell), np.int64)
    else:
        idx = np.minimum(np.searchsorted(g, c.cell), len(g) - 1)
        keep = g[idx] == c.cell
    rec = np.asarray(rec)
    length, clip = rec["read_len"].astype(np.int64), rec["clip_front"].astype(np.int64)
    used = np.zeros(len(aln), np.int64)
    np.add.at(used, c.rec, is_p)
    if (clip + used > length).any():
        raise ValueError("a read window leaves its read")
    h = Hits()
    h.rec, h.col, h.op, h.state, h.site = c.rec[keep], c.col[keep], c.op[keep], c.plane[keep], idx[keep]
    h.pos = c.cell[keep] - np.asarray(allele_off).astype(np.int64)[aln["allele"].astype(np.int64)[h.rec]]
    h.c = clip[h.rec] + ex_p[keep]
    h.raw_d = np.minimum(h.c, np.where(h.op == 3, length[h.rec] - h.c, length[h.rec] - 1 - h.c))
    assert (h.raw_d >= 0).all()
    h.d = np.minimum(h.raw_d, D_MAX)
    return h


def bookings(h, book_ptr):
    """every (hit, booking): (index into the hits, index into book)"""
    bp = np.asarray(book_ptr).astype(np.int64)
    nb = np.diff(bp)[h.rec]
    rep = np.repeat(np.arange(len(h.rec)), nb)
    k = np.arange(len(rep)) - (np.cumsum(nb) - nb)[rep]
    return rep, bp[h.rec[rep]] + k


def clamp(v):
    return np.clip(v, 0, T_MAX)


def restate(allele_off, aln, rec, book_ptr, book, text, ops, site_allele, site_pos):
    """the Table: every hit column once per booking of its record (vectorised)"""
    h = hits(allele_off, aln, rec, text, ops, site_allele, site_pos)
    rep, at = bookings(h, book_ptr)
    t = Table()
    if len(rep) == 0:
        return t
    book = np.asarray(book)
    flags = book["flags"].astype(np.int64)[at]
    uniq, mate, orient = flags & 1, (flags >> 1) & 1, (flags >> 2) & 1
    cell = h.site[rep] * 7 + h.state[rep]
    strand = np.asarray(rec)["strand"].astype(np.int64)[h.rec[rep]]
    ka = ((cell * 2 + strand) * 2 + mate) * 512 + h.d[rep]
    ids, inv = np.unique(ka, return_inverse=True)
    n_all, n_uniq = np.bincount(inv), np.bincount(inv, weights=uniq).astype(np.int64)
    for k, x, y in zip(ids.tolist(), n_all.tolist(), n_uniq.tolist()):
        t.a[(k // 2048 // 7, k // 2048 % 7, (k >> 10) & 1, (k >> 9) & 1, k & 511)] = [x, y]
    pos = h.pos[rep]
    kb = ((cell * 2 + orient) << 24) | (clamp(pos - book["t_start"].astype(np.int64)[at]) << 12) | clamp(book["t_end"].astype(np.int64)[at] - pos)
    ids, n = np.unique(kb, return_counts=True)
    for k, x in zip(ids.tolist(), n.tolist()):
        t.b[((k >> 25) // 7, (k >> 25) % 7, (k >> 24) & 1, (k >> 12) & T_MAX, k & T_MAX)] = x
    return t


def restate_by_loops(allele_off, aln, rec, book_ptr, book, text, ops, site_allele, site_pos):
    """the same, record by record, column by column and booking by booking (small tables only)"""
    off = [int(v) for v in allele_off]
    site_of = {off[int(a)] + int(p): i for i, (a, p) in enumerate(zip(site_allele, site_pos))}
    text = pileup_ref.as_bytes(text) if not isinstance(text, np.ndarray) else text.tobytes()
    t = Table()
    for i, r in enumerate(aln):
        a, start = int(r["allele"]), int(r["seq_start"])
        alen = off[a + 1] - off[a]
        length, clip, strand = int(rec[i]["read_len"]), int(rec[i]["clip_front"]), int(rec[i]["strand"])
        mine = book[int(book_ptr[i]):int(book_ptr[i + 1])]
        pos_t, p, consumed = start, 0, False
        for op in ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])]:
            op = int(op)
            c = clip + p
            if op in (0, 1):
                state, pos, d = int(pileup_ref.CODE[text[int(r["read_at"]) + p]]), pos_t, min(c, length - 1 - c)
                pos_t, p, consumed = pos_t + 1, p + 1, True
            elif op == 3:
                state, pos, d = 5, pos_t, min(c, length - c)
                pos_t, consumed = pos_t + 1, True
            else:
                assert op == 2
                state, pos, d = 6, min(pos_t - 1 if consumed else start, alen - 1), min(c, length - 1 - c)
                p += 1
            assert 0 <= pos < alen and d >= 0
            s = site_of.get(off[a] + pos)
            if s is None:
                continue
            for e in mine:
                f = int(e["flags"])
                x = t.a.setdefault((s, state, strand, (f >> 1) & 1, min(d, D_MAX)), [0, 0])
                x[0] += 1
                x[1] += f & 1
                kb = (s, state, (f >> 2) & 1, min(max(pos - int(e["t_start"]), 0), T_MAX), min(max(int(e["t_end"]) - pos, 0), T_MAX))
                t.b[kb] = t.b.get(kb, 0) + 1
        assert clip + p <= length
    return t


def expected_runs(t):
    """the runs t1k_support_get has to return for the Table: (keys, counts), ascending"""
    runs = []
    for (s, state, strand, mate, d), (n, u) in t.a.items():
        k = ((((s * 7 + state) * 2 + strand) * 2 + mate) * 512 + d) * 2
        runs += [(k + 1 - q, v) for q, v in ((1, u), (0, n - u)) if v]
    for (s, state, orient, ds, de), n in t.b.items():
        runs.append((FAMILY_B | (((s * 7 + state) * 2 + orient) << 24) | (ds << 12) | de, n))
    runs.sort()
    return [k for k, _ in runs], [v for _, v in runs]


def from_runs(keys, counts, n_sites):
    """the runs of t1k_support_get -> the restatement's form.  Below 2^57: key = ((((site * 7 + state) * 2 + strand) * 2 + mate) * 512 + d) * 2
    + (1 - uniq), a uniq booking stored once, under the even key; from 2^57 on: 2^57 | ((site * 7 + state) * 2 + orient) << 24 | dStart << 12
    | dEnd"""
    t = Table()
    for k, c in zip(np.asarray(keys).astype(np.int64).tolist(), np.asarray(counts).astype(np.int64).tolist()):
        if k < FAMILY_B:
            cell = k >> 12
            assert cell // 7 < n_sites
            x = t.a.setdefault((cell // 7, cell % 7, (k >> 11) & 1, (k >> 10) & 1, (k >> 1) & 511), [0, 0])
            x[0] += c
            if (k & 1) == 0:
                x[1] += c
        else:
            k ^= FAMILY_B
            assert k < FAMILY_B and (k >> 25) // 7 < n_sites
            kb = ((k >> 25) // 7, (k >> 25) % 7, (k >> 24) & 1, (k >> 12) & T_MAX, k & T_MAX)
            assert kb not in t.b
            t.b[kb] = c
    return t


def same(x, y):
    return x.a == y.a and x.b == y.b


def lines(t, end=10):
    """{(site, state): the ten columns of its line}"""
    cells = {}
    for (s, state, strand, mate, d), (n, u) in t.a.items():
        x = cells.setdefault((s, state), {"n": 0, "u": 0, "strand": [0, 0], "mate": [0, 0], "d": {}, "templates": 0})
        x["n"] += n
        x["u"] += u
        x["strand"][strand] += n
        x["mate"][mate] += n
        x["d"][d] = x["d"].get(d, 0) + n
    for (s, state, _, _, _) in t.b:
        cells[(s, state)]["templates"] += 1
    out = {}
    for key, x in cells.items():
        ds = sorted(x["d"])
        cum, med = 0, None
        for d in ds:
            cum += x["d"][d]
            if med is None and 2 * cum >= x["n"]:
                med = d
        out[key] = (x["n"], x["u"], x["strand"][0], x["strand"][1], x["mate"][0], x["mate"][1], ds[0], med, sum(v for d, v in x["d"].items() if d < end), x["templates"])
    return out


# ---- tables for the kernel -----------------------------------------------------------------------------------------------------------
def generate(seed=1, records=6000):
    """pileup_ref.generate's records on alleles of 1, 63, 64, 65, 1000, 4097 and 9000 bases, with
    .site_allele / .site_pos: every position of the four short alleles; 64k - 1, 64k, 64k + 1 of the 4097-base allele; 48 positions at the start
    of the region where most records start; 4 % random positions; the last position of every allele; three special sites (below);
    .rec: a third of the records unclipped at the front, a third at the back (d = 0 at either end; a deletion column at c = 0 or c = L), 6 % with
    100 .. 700 clipped bases on both sides (the distances in between), 4 % with 520 .. 700 (d saturates), the others with 0 .. 30;
    .book_ptr / .book: 0 .. 5 bookings per record (six records: 200), a third uniq, mates and orients even; templates that reach 0 .. 300 bases
    beyond the record, 5 % anywhere on the allele (the site may lie outside: both distances clamp at 0), 5 % the whole allele (on the
    9000-base allele both distances pass 4095).
    Three records are appended on the 9000-base allele, each a match and an insert at a site of its own where no other record books an
    insert, so that the cell (site, +) is theirs alone: .special = {"one": site whose 200 bookings share one template, "all": site whose 200
    bookings all differ, "far": site with two templates that differ only beyond the clamp}."""
    t = pileup_ref.generate(seed=seed, records=records, allele_len=ALLELE_LEN)
    rng = np.random.default_rng(seed + 2000)
    off = t.allele_off.astype(np.int64)
    lens = np.diff(off)
    big = int(np.argmax(lens))
    assert lens[big] == 9000
    # the special records: where no generated record books an insert, 4150 .. 4850 of the longest allele (more than 4095 bases from both ends)
    cols = sitepile_ref.columns(t.allele_off, t.aln, t.text, t.ops)
    taken = set(cols.cell[cols.plane == sitepile_ref.INS].tolist())
    free = [p for p in range(4150, 4850) if int(off[big]) + p not in taken]
    spots = [free[0], free[len(free) // 2], free[-1]]
    ops_at, text_at = len(t.ops), int(np.nonzero(t.text == ord("A"))[0][0])
    extra = [(big, p, text_at, ops_at + 2 * i, 2, 0, 0, 0) for i, p in enumerate(spots)]
    t.aln = np.concatenate([t.aln, np.array(extra, t1k_amd.PILEUP_ALN_DTYPE)])
    t.ops = np.concatenate([t.ops, np.array([0, 2] * 3, np.int8)])
    n_rec = len(t.aln)
    # sites
    g = set(int(off[big]) + p for p in spots)
    for a in range(len(lens)):
        if lens[a] <= 65:
            g.update(range(int(off[a]), int(off[a + 1])))
        g.add(int(off[a + 1]) - 1)
    mid = ALLELE_LEN.index(4097)
    for k in range(0, 4097 + 1, 64):
        g.update(int(off[mid]) + p for p in (k - 1, k, k + 1) if 0 <= p < 4097)
    lo = t.region[1][0]
    t.dense = (int(off[big]) + lo, int(off[big]) + lo + 48)
    g.update(range(*t.dense))
    g.update(np.nonzero(rng.random(int(off[-1])) < 0.04)[0].tolist())
    g = np.array(sorted(g), np.int64)
    t.site_allele = (np.searchsorted(off, g, side="right") - 1).astype(np.uint32)
    t.site_pos = (g - off[t.site_allele]).astype(np.uint32)
    t.special = dict(zip(("one", "all", "far"), (int(np.searchsorted(g, int(off[big]) + p)) for p in spots)))
    # the read-ends
    n_ops = t.aln["n_ops"].astype(np.int64)
    col_rec = np.repeat(np.arange(n_rec), n_ops)
    first = (np.cumsum(n_ops) - n_ops)[col_rec]
    e = t.ops[t.aln["ops_at"].astype(np.int64)[col_rec] + np.arange(len(col_rec)) - first]
    n_p, n_t = np.bincount(col_rec, weights=e != 3, minlength=n_rec).astype(np.int64), np.bincount(col_rec, weights=e != 2, minlength=n_rec).astype(np.int64)
    kind = rng.random(n_rec)
    front, back = rng.integers(0, 31, n_rec), rng.integers(0, 31, n_rec)
    front[kind < 0.33] = 0
    back[(kind >= 0.25) & (kind < 0.58)] = 0                                               # (a twelfth of the records: neither clip)
    deep = kind >= 0.9
    front[deep], back[deep] = rng.integers(100, 701, int(deep.sum())), rng.integers(100, 701, int(deep.sum()))
    front[kind >= 0.96], back[kind >= 0.96] = front[kind >= 0.96] % 181 + 520, back[kind >= 0.96] % 181 + 520
    back[(front + n_p + back) == 0] = 1                                                    # an all-deletion window of a read-end of one base
    t.rec = np.zeros(n_rec, t1k_amd.SUPPORT_REC_DTYPE)
    t.rec["read_len"], t.rec["clip_front"], t.rec["strand"] = front + n_p + back, front, rng.integers(0, 2, n_rec)
    # the bookings
    n = rng.integers(0, 6, n_rec)
    n[rng.choice(records, 6, replace=False)] = 200
    n[records:] = (200, 200, 2)
    t.book_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    total = int(n.sum())
    of = np.repeat(np.arange(n_rec), n)
    alen = lens[t.aln["allele"].astype(np.int64)][of]
    start = t.aln["seq_start"].astype(np.int64)[of]
    stop = np.minimum(np.maximum(start + n_t[of] - 1, start), alen - 1)
    start = np.minimum(start, alen - 1)
    t_start, t_end = np.maximum(start - rng.integers(0, 301, total), 0), np.minimum(stop + rng.integers(0, 301, total), alen - 1)
    how = rng.random(total)
    x, y = (rng.random(total) * alen).astype(np.int64), (rng.random(total) * alen).astype(np.int64)
    anywhere, whole = how < 0.05, how >= 0.95
    t_start[anywhere], t_end[anywhere] = np.minimum(x, y)[anywhere], np.maximum(x, y)[anywhere]
    t_start[whole], t_end[whole] = 0, alen[whole] - 1
    flags = (rng.random(total) < 0.33).astype(np.int64) | (rng.integers(0, 2, total) << 1) | (rng.integers(0, 2, total) << 2)
    b0 = [int(v) for v in t.book_ptr[records:]]
    t_start[b0[0]:b0[1]], t_end[b0[0]:b0[1]], flags[b0[0]:b0[1]] = 10, 8990, 5              # one template, 200 times
    t_start[b0[1]:b0[2]], t_end[b0[1]:b0[2]] = spots[1] - np.arange(200), spots[1] + 5      # 200 templates
    flags[b0[1]:b0[2]] = 2
    t_start[b0[2]:b0[3]], t_end[b0[2]:b0[3]], flags[b0[2]:b0[3]] = (0, 1), (8999, 8998), 0   # two templates that differ beyond the clamp only
    t.book = np.zeros(total, t1k_amd.SUPPORT_BOOK_DTYPE)
    t.book["flags"], t.book["t_start"], t.book["t_end"] = flags, t_start, t_end
    t.records = records
    return t


def args(t):
    return (t.allele_off, t.aln, t.rec, t.book_ptr, t.book, t.text, t.ops, t.site_allele, t.site_pos)


# ---- <prefix>_allele_support.tsv -----------------------------------------------------------------------------------------------------
def table_text(names, seqs, exon_masks, site_allele, site_pos, var_of, rows):
    """the file the analyzer writes: rows = lines(table, end); var_of = {(allele, pos): "A" or "A,C"}; by site (= allele, then pos), then state"""
    out = [HEADER]
    for (s, state) in sorted(rows):
        a, p = int(site_allele[s]), int(site_pos[s])
        mask = exon_masks[a]
        exonic = int(np.asarray(mask[:p + 1], np.int64).sum())
        out.append("%s\t%d\t%s\t%s\t%s\t%s\t%s" % (names[a], p + 1, exonic if mask[p] else ".", seqs[a][p], var_of.get((a, p), "."), STATES[state],
                                                   "\t".join("%d" % v for v in rows[(s, state)])))
    return "\n".join(out) + "\n"


def parse(path):
    """-> (header line, rows): a row = (allele, pos, exon_pos or None, ref, var, obs, {column: value})"""
    text = open(path).read().split("\n")
    assert text[-1] == ""
    rows = []
    for line in text[1:-1]:
        f = line.split("\t")
        assert len(f) == 6 + len(COLUMNS) and f[5] in STATES, line
        rows.append((f[0], int(f[1]), None if f[2] == "." else int(f[2]), f[3], f[4], f[5], dict(zip(COLUMNS, (int(v) for v in f[6:])))))
    return text[0], rows


def analyzer_records(asg_ptr, asg, reads1, reads2=None):
    """pileup_ref.to_records (one record per assignment overlap) plus what the analyzer hands to t1k_support_add: per record the length of
    its read-end, its read_start and its strand; one booking each: uniq when the fragment has one assignment, mate when the read-end comes
    from file 2, the template's extent over both mates, orient = file 1 on the reverse strand (a file-2 read-end alone: on the forward one)
    -> (aln, text, rec, book_ptr, book)"""
    aln, text = pileup_ref.to_records(asg_ptr, asg, reads1, reads2)
    rec, book = [], []
    for f in range(len(asg_ptr) - 1):
        lo, hi = int(asg_ptr[f]), int(asg_ptr[f + 1])
        uniq = 1 if hi - lo == 1 else 0
        for a in asg[lo:hi]:
            pair = int(a["has_mate_pair"]) != 0
            from2 = int(a["o1_from_r2"]) != 0 and not pair
            o1, o2 = a["o1"], a["o2"]
            t_start = min(int(o1["seq_start"]), int(o2["seq_start"])) if pair else int(o1["seq_start"])
            t_end = max(int(o1["seq_end"]), int(o2["seq_end"])) if pair else int(o1["seq_end"])
            orient = int(int(o1["strand"]) == 1) if from2 else int(int(o1["strand"]) == -1)
            for o, second in [(o1, from2)] + ([(o2, True)] if pair else []):
                read = (reads2 if second else reads1)[f]
                rec.append((len(read), int(o["read_start"]), 1 if int(o["strand"]) == -1 else 0))
                book.append((uniq | (int(second) << 1) | (orient << 2), t_start, t_end))
    assert len(rec) == len(aln)
    return (aln, text, np.array(rec, t1k_amd.SUPPORT_REC_DTYPE).reshape(-1), np.arange(len(aln) + 1, dtype=np.uint64),
            np.array(book, t1k_amd.SUPPORT_BOOK_DTYPE).reshape(-1))
