"""The read-backed phasing of site pairs of the analyzer (--phase, t1k_phase_*) restated sequentially in numpy and by plain
loops, a generator of synthetic record / booking / site tables for the kernel test, and a parser / writer of <prefix>_allele_phase.tsv.

The quantity: a record (one alignment) observes a site with the column of its edit string that consumes that allele position: ops 0 / 1
give the read base (state 0 .. 3 = A C G T, 4 = N for anything else), op 3 gives state 5 = del; insert columns observe nothing.  A booking
is a fragment-assignment (rec1, rec2 or NO_MATE, uniq).  Its observations are the union of its records': a site both show in the same
state counts once, a site they show in different states is dropped for this booking (discordant); rec1 == rec2 gives that record's own
list.  Every unordered pair of a booking's observed sites s < t in states x, y adds 1 to cell (s, t, x, y), and to its _uniq count when
uniq is set.  Result: {(s, t, x, y): int64[2] = (count, count_uniq)} with only the cells that received a booking."""
import numpy as np

import pileup_ref
import sitepile_ref
import t1k_amd

NO_MATE = t1k_amd.PHASE_NO_MATE
STATES = t1k_amd.PHASE_STATES
HEADER = "#allele\tpos1\tpos2\texon_pos1\texon_pos2\tref1\tref2\tvar1\tvar2\tobs1\tobs2\tcount\tcount_uniq"
N, DEL, INS = pileup_ref.N, pileup_ref.DEL, pileup_ref.INS


class Stats:
    """what t1k_phase_stats reports of a table"""

    def __init__(self, observations=0, bookings=0, keys=0, discordant=0):
        self.observations, self.bookings, self.keys, self.discordant = observations, bookings, keys, discordant

    def same(self, d):
        return (self.observations, self.bookings, self.keys, self.discordant) == (d["observations"], d["bookings"], d["keys"], d["discordant"])


def observations(allele_off, aln, text, ops, site_allele, site_pos):
    """(obs_ptr int64 [records + 1], site, state): the records' observations, record by record, ascending in site inside a record"""
    h = sitepile_ref.hits(allele_off, aln, text, ops, site_allele, site_pos)
    keep = h.op != 2
    rec, site, state = h.rec[keep], h.site[keep], h.plane[keep]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=len(aln)))]).astype(np.int64)
    return ptr, site.astype(np.int64), state.astype(np.int64)


def _book(book_rec, book_uniq):
    br = np.asarray(book_rec).astype(np.int64).reshape(-1, 2)
    return br[:, 0], br[:, 1], np.asarray(book_uniq).astype(np.int64)


def _gather(ptr, recs):
    """indices of the observations of `recs`, list by list, and the list each belongs to"""
    n = ptr[recs + 1] - ptr[recs]
    of = np.repeat(np.arange(len(recs)), n)
    return ptr[recs][of] + np.arange(len(of)) - (np.cumsum(n) - n)[of], of


def merged(allele_off, aln, book_rec, book_uniq, text, ops, site_allele, site_pos):
    """(booking, site, state) of every surviving observation, sorted by (booking, site); per booking its discordant sites; the observations"""
    ptr, site, state = observations(allele_off, aln, text, ops, site_allele, site_pos)
    r1, r2, _ = _book(book_rec, book_uniq)
    two = np.nonzero((r2 != NO_MATE) & (r2 != r1))[0]
    i1, b1 = _gather(ptr, r1)
    i2, b2 = _gather(ptr, r2[two])
    b = np.concatenate([b1, two[b2]])
    s, x = np.concatenate([site[i1], site[i2]]), np.concatenate([state[i1], state[i2]])
    n_sites = max(len(site_allele), 1)
    order = np.argsort(b * n_sites + s, kind="stable")
    b, s, x = b[order], s[order], x[order]
    k = b * n_sites + s
    twin_next, twin_prev = np.zeros(len(k), bool), np.zeros(len(k), bool)
    twin_next[:-1] = k[1:] == k[:-1]                              # same booking and site as the next entry: seen by both mates
    twin_prev[1:] = twin_next[:-1]
    same = twin_next & (x == np.roll(x, -1))
    clash = twin_next & ~same
    drop = twin_prev | clash                                      # the second copy always; the first when the states differ
    disc = np.bincount(b[clash], minlength=len(r1))
    return b[~drop], s[~drop], x[~drop], disc, len(site)


def restate(allele_off, aln, book_rec, book_uniq, text, ops, site_allele, site_pos):
    """-> ({(s, t, x, y): int64[2]}, Stats)"""
    b, s, x, disc, n_obs = merged(allele_off, aln, book_rec, book_uniq, text, ops, site_allele, site_pos)
    _, _, uniq = _book(book_rec, book_uniq)
    n_sites = len(site_allele)
    m = np.bincount(b, minlength=len(uniq))
    start = (np.cumsum(m) - m)[b]
    later = m[b] - 1 - (np.arange(len(b)) - start)               # entries of the same booking behind this one
    first = np.repeat(np.arange(len(b)), later)
    second = first + 1 + np.arange(len(first)) - (np.cumsum(later) - later)[first]
    cell = ((s[first] * n_sites + s[second]) * 36 + x[first] * 6 + x[second])
    st = Stats(n_obs, int((m >= 2).sum()), len(cell), int(disc.sum()))
    if len(cell) == 0:
        return {}, st
    ids, inv = np.unique(cell, return_inverse=True)
    table = np.zeros((len(ids), 2), np.int64)
    np.add.at(table, (inv, 0), 1)
    np.add.at(table, (inv, 1), uniq[b[first]] != 0)
    return {_cell(int(i), n_sites): table[j] for j, i in enumerate(ids)}, st


def _cell(i, n_sites):
    return (i // 36 // n_sites, i // 36 % n_sites, i % 36 // 6, i % 6)


def restate_by_loops(allele_off, aln, book_rec, book_uniq, text, ops, site_allele, site_pos):
    """the same, record by record through pileup_ref.walk and booking by booking (small tables only)"""
    off = np.asarray(allele_off).astype(np.int64)
    g = sitepile_ref.site_cells(allele_off, site_allele, site_pos)
    seen = []
    for r in aln:
        a = int(r["allele"])
        one = np.zeros((14, int(off[-1])), np.int64)
        pileup_ref.walk(one, int(off[a]), int(off[a + 1] - off[a]), r["seq_start"], text, int(r["read_at"]), ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])], 1, 0)
        mine = {}
        for i, cell in enumerate(g):
            col = one[:6, cell]                                  # (the ins plane observes nothing)
            if col.any():
                assert col.sum() == 1
                mine[i] = int(np.argmax(col))
        seen.append(mine)
    out, st = {}, Stats(observations=sum(len(d) for d in seen))
    for (r1, r2), uniq in zip(np.asarray(book_rec).astype(np.int64).reshape(-1, 2).tolist(), np.asarray(book_uniq).tolist()):
        obs = dict(seen[r1])
        if r2 != NO_MATE and r2 != r1:
            for site, state in seen[r2].items():
                if site not in seen[r1]:
                    obs[site] = state
                elif seen[r1][site] != state:
                    del obs[site]
                    st.discordant += 1
        sites = sorted(obs)
        st.bookings += len(sites) >= 2
        for i, s in enumerate(sites):
            for t in sites[i + 1:]:
                c = out.setdefault((s, t, obs[s], obs[t]), np.zeros(2, np.int64))
                c += (1, 1 if uniq else 0)
                st.keys += 1
    return out, st


def from_runs(keys, counts, n_sites):
    """the runs of t1k_phase_get -> the restatement's form.  key = (((s * nSites + t) * 36 + x * 6 + y) << 1) | (1 - uniq); the reader adds
    the even (uniq) run of a cell to its plain counter as well"""
    out = {}
    for k, c in zip(np.asarray(keys).astype(np.int64).tolist(), np.asarray(counts).astype(np.int64).tolist()):
        t = out.setdefault(_cell(k >> 1, n_sites), np.zeros(2, np.int64))
        t[0] += c
        if not k & 1:
            t[1] += c
    return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ---- tables for the kernel -----------------------------------------------------------------------------------------------------------
def generate(seed=1, records=6000, bookings=9000, clones=600, density=0.08):
    """pileup_ref.generate's records (the record generator of §11.3), plus `clones` records that repeat an earlier record's alignment on a
    copy of its read window with a tenth of the bases edited (a mate that overlaps it on every site, agreeing on most).
    .site_allele / .site_pos: every position of the four short alleles, the last position of every allele, and `density` of all positions.
    .book_rec / .book_uniq: a fifth single records, a tenth rec1 == rec2, a fifth a record with its clone, the rest two random records of
    one allele; a third of them uniq."""
    t = pileup_ref.generate(seed=seed, records=records)
    rng = np.random.default_rng(seed + 2000)
    off = t.allele_off.astype(np.int64)
    lens = np.diff(off)
    # clones
    src = rng.choice(records, clones, replace=False)
    text, recs = [t.text], []
    at = len(t.text)
    for i in src:
        r = t.aln[i]
        e = t.ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])]
        n_p = int((e != 3).sum())
        w = t.text[int(r["read_at"]):int(r["read_at"]) + n_p].copy()
        edit = rng.random(n_p) < 0.1
        w[edit] = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, int(edit.sum()))]
        recs.append((r["allele"], r["seq_start"], at, r["ops_at"], r["n_ops"], 1, 0, 0))
        text.append(w)
        at += n_p
    t.aln = np.concatenate([t.aln, np.array(recs, t1k_amd.PILEUP_ALN_DTYPE)])
    t.text = np.concatenate(text)
    t.clone_of = dict(zip(range(records, records + clones), src.tolist()))
    # sites
    g = set()
    for a in range(len(lens)):
        if lens[a] <= 65:
            g.update(range(int(off[a]), int(off[a + 1])))
        g.add(int(off[a + 1]) - 1)
    g.update(np.nonzero(rng.random(int(off[-1])) < density)[0].tolist())
    g = np.array(sorted(g), np.int64)
    t.site_allele = (np.searchsorted(off, g, side="right") - 1).astype(np.uint32)
    t.site_pos = (g - off[t.site_allele]).astype(np.uint32)
    # bookings
    by_allele = [np.nonzero(t.aln["allele"] == a)[0] for a in range(len(lens))]
    kind = rng.choice(4, bookings, p=[0.2, 0.1, 0.2, 0.5])
    r1 = rng.integers(0, len(t.aln), bookings)
    r2 = np.full(bookings, NO_MATE, np.int64)
    r2[kind == 1] = r1[kind == 1]
    k2 = np.nonzero(kind == 2)[0]
    r2[k2] = records + rng.integers(0, clones, len(k2))
    r1[k2] = src[r2[k2] - records]
    for b in np.nonzero(kind == 3)[0]:
        group = by_allele[int(t.aln["allele"][r1[b]])]
        r2[b] = group[int(rng.integers(0, len(group)))]
    t.book_rec = np.stack([r1, r2], axis=1).astype(np.uint32)
    t.book_uniq = (rng.random(bookings) < 0.33).astype(np.uint8)
    t.book_kind = kind
    return t


def table_args(t):
    return (t.allele_off, t.aln, t.book_rec, t.book_uniq, t.text, t.ops, t.site_allele, t.site_pos)


# ---- <prefix>_allele_phase.tsv -------------------------------------------------------------------------------------------------------
def table_text(names, seqs, exon_masks, site_allele, site_pos, var_of, cells):
    """the file the analyzer writes: cells = {(s, t, x, y): (count, count_uniq)}; var_of = {(allele, pos): "A" or "A,C"}; lines by site
    pair (= allele, then pos1, pos2), then obs1, obs2 in state order"""
    out = [HEADER]

    def exon(a, p):
        return "%d" % int(np.asarray(exon_masks[a][:p + 1], np.int64).sum()) if exon_masks[a][p] else "."
    for (s, t, x, y) in sorted(cells):
        a, p, q = int(site_allele[s]), int(site_pos[s]), int(site_pos[t])
        assert int(site_allele[t]) == a and p < q
        c = cells[(s, t, x, y)]
        out.append("\t".join([names[a], "%d" % (p + 1), "%d" % (q + 1), exon(a, p), exon(a, q), seqs[a][p], seqs[a][q], var_of.get((a, p), "."), var_of.get((a, q), "."),
                              STATES[x], STATES[y], "%d" % c[0], "%d" % c[1]]))
    return "\n".join(out) + "\n"


def parse(path):
    """-> (header line, rows): a row = (allele, pos1, pos2, exon_pos1 or None, exon_pos2 or None, ref1, ref2, var1, var2, obs1, obs2, count, count_uniq)"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    rows = []
    for line in lines[1:-1]:
        f = line.split("\t")
        assert len(f) == 13 and f[9] in STATES and f[10] in STATES, line
        rows.append((f[0], int(f[1]), int(f[2]), None if f[3] == "." else int(f[3]), None if f[4] == "." else int(f[4])) + tuple(f[5:11]) + (int(f[11]), int(f[12])))
    return lines[0], rows


def analyzer_records(asg_ptr, asg, reads1, reads2):
    """pileup_ref.to_records plus the bookings the analyzer builds: one per assignment -- its o1 record, its o2 record with a mate pair,
    uniq when the fragment has one assignment"""
    aln, text = pileup_ref.to_records(asg_ptr, asg, reads1, reads2)
    mate = asg["has_mate_pair"] != 0
    first = np.cumsum(1 + mate.astype(np.int64)) - (1 + mate.astype(np.int64))
    assert len(aln) == (int(first[-1]) + 1 + int(mate[-1]) if len(asg) else 0)
    book_rec = np.stack([first, np.where(mate, first + 1, NO_MATE)], axis=1).astype(np.uint32)
    n_asg = np.diff(np.asarray(asg_ptr).astype(np.int64))
    book_uniq = np.repeat(n_asg == 1, n_asg).astype(np.uint8)
    return aln, text, book_rec, book_uniq
