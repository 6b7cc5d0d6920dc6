"""The per-barcode pileup at sites of the analyzer (--barcodePileup, t1k_sitepile_*) restated sequentially in numpy, a
generator of synthetic record / booking / site tables for the kernel test, and a parser / writer of <prefix>_barcode_pileup.tsv.

The quantity: what pileup_ref describes, restricted to a list of sites (allele, 0-based position) and split by barcode.  A record books
once per entry of its booking list, an entry being barcode << 1 | uniq; a booking with uniq set counts in the plain counter and in the
_uniq one.  Result: {(barcode, site index): int64[14]} with only the cells whose first seven counters are not all zero."""
import numpy as np

import pileup_ref
import t1k_amd

COUNTERS = t1k_amd.PILEUP_COUNTERS
HEADER = "#barcode\tallele\tpos\texon_pos\tref\tvar\t" + "\t".join(COUNTERS)
N, DEL, INS, UNIQ = pileup_ref.N, pileup_ref.DEL, pileup_ref.INS, pileup_ref.UNIQ


class Columns:
    pass


def columns(allele_off, aln, text, ops):
    """every edit column of every record, located by prefix sums inside its record: .rec, .col (index inside the record), .op, .plane
    (0 .. 6) and .cell (allele_off[allele] + the position it books at)"""
    off = np.asarray(allele_off).astype(np.int64)
    length = np.diff(off)
    text = np.frombuffer(pileup_ref.as_bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    ops = np.asarray(ops, np.int8)
    n_ops = aln["n_ops"].astype(np.int64)
    c = Columns()
    c.rec = np.repeat(np.arange(len(aln)), n_ops)
    first = (np.cumsum(n_ops) - n_ops)[c.rec]
    c.col = np.arange(len(c.rec)) - first
    e = ops[aln["ops_at"].astype(np.int64)[c.rec] + c.col].astype(np.int64)
    if ((e < 0) | (e > 3)).any():
        raise ValueError("an op outside 0 .. 3")
    is_t, is_p = (e != 2).astype(np.int64), (e != 3).astype(np.int64)
    ex_t, ex_p = np.cumsum(is_t) - is_t, np.cumsum(is_p) - is_p
    if len(e):
        ex_t, ex_p = ex_t - ex_t[first], ex_p - ex_p[first]
    allele = aln["allele"].astype(np.int64)[c.rec]
    start, alen = aln["seq_start"].astype(np.int64)[c.rec], length[allele]
    pos = start + ex_t
    ins = e == 2
    pos[ins] = np.minimum(np.where(ex_t[ins] > 0, pos[ins] - 1, start[ins]), alen[ins] - 1)
    if ((pos < 0) | (pos >= alen)).any():
        raise ValueError("a walk leaves its allele")
    plane = np.where(e == 3, DEL, INS)
    base = e <= 1
    rp = aln["read_at"].astype(np.int64)[c.rec] + ex_p
    if (rp[e != 3] >= len(text)).any():
        raise ValueError("a walk leaves the text")
    plane[base] = pileup_ref.CODE[text[rp[base]]]
    c.op, c.plane, c.cell = e, plane, off[allele] + pos
    return c


def site_cells(allele_off, site_allele, site_pos):
    g = np.asarray(allele_off).astype(np.int64)[np.asarray(site_allele, np.int64)] + np.asarray(site_pos, np.int64)
    assert (np.diff(g) > 0).all(), "sites ascending by (allele, pos), no duplicates"
    return g


def hits(allele_off, aln, text, ops, site_allele, site_pos):
    """the columns that book at a site: (Columns restricted to them, with .site = the site's index)"""
    c = columns(allele_off, aln, text, ops)
    g = site_cells(allele_off, site_allele, site_pos)
    h = Columns()
    if len(g) == 0:
        keep, idx = np.zeros(len(c.cell), bool), np.zeros(len(c.cell), np.int64)
    else:
        idx = np.minimum(np.searchsorted(g, c.cell), len(g) - 1)
        keep = g[idx] == c.cell
    for k in ("rec", "col", "op", "plane", "cell"):
        setattr(h, k, getattr(c, k)[keep])
    h.site = idx[keep]
    return h


def _fold(cell, plane, uniq):
    """(cell id, plane, uniq flag) per booking (at least one) -> (cell ids, int64 [cells, 14])"""
    ids, inv = np.unique(cell, return_inverse=True)
    table = np.zeros((len(ids), 14), np.int64)
    np.add.at(table, (inv, plane), 1)
    np.add.at(table, (inv[uniq != 0], plane[uniq != 0] + UNIQ), 1)
    return ids, table


def restate(allele_off, aln, book_ptr, book, text, ops, site_allele, site_pos):
    """{(barcode, site): int64[14]}: every hit column once per booking of its record"""
    h = hits(allele_off, aln, text, ops, site_allele, site_pos)
    bp, book = np.asarray(book_ptr).astype(np.int64), np.asarray(book).astype(np.int64)
    nb = np.diff(bp)[h.rec]
    rep = np.repeat(np.arange(len(h.rec)), nb)
    if len(rep) == 0:
        return {}
    k = np.arange(len(rep)) - (np.cumsum(nb) - nb)[rep]
    e = book[bp[h.rec[rep]] + k]
    n_sites = len(site_allele)
    ids, table = _fold((e >> 1) * n_sites + h.site[rep], h.plane[rep], e & 1)
    return {(int(i) // n_sites, int(i) % n_sites): table[j] for j, i in enumerate(ids)}


def restate_by_loops(allele_off, aln, book_ptr, book, text, ops, site_allele, site_pos):
    """the same, record by record and booking by booking through pileup_ref.walk (small tables only)"""
    off = np.asarray(allele_off).astype(np.int64)
    site_of = {int(g): i for i, g in enumerate(site_cells(allele_off, site_allele, site_pos))}
    out = {}
    for i, r in enumerate(aln):
        a = int(r["allele"])
        one = np.zeros((14, int(off[-1])), np.int64)
        pileup_ref.walk(one, int(off[a]), int(off[a + 1] - off[a]), r["seq_start"], text, int(r["read_at"]), ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])], 1, 1)
        for e in book[int(book_ptr[i]):int(book_ptr[i + 1])]:
            for g in np.nonzero(one[:7].sum(axis=0))[0]:
                if int(g) in site_of:
                    c = out.setdefault((int(e) >> 1, site_of[int(g)]), np.zeros(14, np.int64))
                    c[:7] += one[:7, g]
                    if int(e) & 1:
                        c[7:] += one[7:, g]
    return out


def from_runs(keys, counts, n_sites):
    """the runs of t1k_sitepile_get -> the restatement's form.  key = ((barcode * nSites + site) * 7 + plane) * 2 + (1 - uniq); the reader
    adds the even (uniq) run of a cell to its plain counter as well"""
    keys, counts = np.asarray(keys).astype(np.int64), np.asarray(counts).astype(np.int64)
    out = {}
    for k, c in zip(keys.tolist(), counts.tolist()):
        cell, plane, uniq = k // 14, (k % 14) >> 1, 1 - (k & 1)
        t = out.setdefault((cell // n_sites, cell % n_sites), np.zeros(14, np.int64))
        t[plane] += c
        if uniq:
            t[UNIQ + plane] += c
    return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def dense(cells, allele_off, site_allele, site_pos):
    """summed over barcodes: int64 [14, positions], zero away from the sites"""
    g = site_cells(allele_off, site_allele, site_pos)
    out = np.zeros((14, int(np.asarray(allele_off)[-1])), np.int64)
    for (_, s), c in cells.items():
        out[:, g[s]] += c
    return out


# ---- tables for the kernel -----------------------------------------------------------------------------------------------------------
def generate(seed=1, records=30000, barcodes=300, hot_barcode=7):
    """pileup_ref.generate's records on alleles of 1, 63, 64, 65, 1000 and 4097 bases (their boundaries fall inside bitmap words), plus
    .site_allele / .site_pos: every position of the four short alleles; 64k - 1, 64k, 64k + 1 of the longest; one fully set bitmap word;
    48 positions at the start of the region where most records start; 5 % random positions; the last position of every allele;
    .book_ptr / .book: 0 .. 5 bookings per record (a few records: 200) over `barcodes` barcodes, about half of them on hot_barcode, a third
    of them uniq."""
    t = pileup_ref.generate(seed=seed, records=records)
    rng = np.random.default_rng(seed + 1000)
    off = t.allele_off.astype(np.int64)
    lens = np.diff(off)
    big = int(np.argmax(lens))
    g = set()
    for a in range(len(lens)):
        if lens[a] <= 65:
            g.update(range(int(off[a]), int(off[a + 1])))
        g.add(int(off[a + 1]) - 1)
    for k in range(0, int(lens[big]) + 1, 64):
        g.update(int(off[big]) + p for p in (k - 1, k, k + 1) if 0 <= p < lens[big])
    t.full_word = (int(off[big]) + 1000) // 64 + 1
    g.update(range(t.full_word * 64, t.full_word * 64 + 64))
    lo = t.region[1][0]
    t.dense = (int(off[big]) + lo, int(off[big]) + lo + 48)
    g.update(range(*t.dense))
    g.update(np.nonzero(rng.random(int(off[-1])) < 0.05)[0].tolist())
    g = np.array(sorted(g), np.int64)
    t.site_allele = (np.searchsorted(off, g, side="right") - 1).astype(np.uint32)
    t.site_pos = (g - off[t.site_allele]).astype(np.uint32)
    n = rng.integers(0, 6, len(t.aln))
    n[rng.choice(len(t.aln), 12, replace=False)] = 200
    t.book_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    total = int(n.sum())
    bc = np.where(rng.random(total) < 0.5, hot_barcode, rng.integers(0, barcodes, total))
    t.book = ((bc << 1) | (rng.random(total) < 0.33)).astype(np.uint32)
    t.n_barcodes, t.hot_barcode = barcodes, hot_barcode
    return t


# ---- <prefix>_barcode_pileup.tsv -----------------------------------------------------------------------------------------------------
def table_text(barcode_names, names, seqs, exon_masks, site_allele, site_pos, var_of, cells):
    """the file the analyzer writes: cells = {(barcode id, site): 14 counters}; var_of = {(allele, pos): "A" or "A,C"}; lines by barcode
    id, then site (= allele, then pos)"""
    out = [HEADER]
    for (b, s) in sorted(cells):
        a, p = int(site_allele[s]), int(site_pos[s])
        mask = exon_masks[a]
        exonic = int(np.asarray(mask[:p + 1], np.int64).sum())
        out.append("%s\t%s\t%d\t%s\t%s\t%s\t%s" % (barcode_names[b], names[a], p + 1, exonic if mask[p] else ".", seqs[a][p], var_of.get((a, p), "."),
                                               "\t".join("%d" % v for v in cells[(b, s)])))
    return "\n".join(out) + "\n"


def parse(path):
    """-> (header line, rows): a row = (barcode, allele, pos, exon_pos or None, ref, var, {counter: value})"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    rows = []
    for line in lines[1:-1]:
        f = line.split("\t")
        assert len(f) == 6 + len(COUNTERS), line
        rows.append((f[0], f[1], int(f[2]), None if f[3] == "." else int(f[3]), f[4], f[5], dict(zip(COUNTERS, (int(v) for v in f[6:])))))
    return lines[0], rows


def barcode_ids(barcodes):
    """the analyzer's barcode ids: first appearance over all loaded fragments -> (names in id order, id per fragment)"""
    ids, names = {}, []
    of = []
    for b in barcodes:
        if b not in ids:
            ids[b] = len(names)
            names.append(b)
        of.append(ids[b])
    return names, of


def analyzer_records(asg_ptr, asg, reads1, reads2, bc_of):
    """pileup_ref.to_records plus the booking lists the analyzer builds: one booking per record, barcode of its fragment, uniq when the
    fragment has one assignment"""
    aln, text = pileup_ref.to_records(asg_ptr, asg, reads1, reads2)
    per_asg = 1 + (asg["has_mate_pair"] != 0).astype(np.int64)
    frag_of_asg = np.repeat(np.arange(len(asg_ptr) - 1), np.diff(np.asarray(asg_ptr).astype(np.int64)))
    frag = np.repeat(frag_of_asg, per_asg)
    assert len(frag) == len(aln)
    book = ((np.asarray(bc_of, np.int64)[frag] << 1) | aln["w_uniq"].astype(np.int64)).astype(np.uint32)
    return aln, text, np.arange(len(aln) + 1, dtype=np.uint64), book
