"""The look-up rule of seeding as the kernels decide it, read-end by read-end, against its plain restatement (tests/seed_ref.py, pinned to
the oracle and to the reference's own code by tests/test_seed_cpu.py) on the designed cases of tests/seed_cases.py: every comparison is
integer equality.  The kernels' decision is read through the seed report (Context.seed_report: used k-mers per strand, their offsets
and list lengths, the used-offset masks) and through the look-up / posting counters of Context.stats() and Context.extract()."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_assign_check  # noqa: E402
import seed_cases as sc  # noqa: E402
import seed_ref  # noqa: E402
import util  # noqa: E402
import t1k_amd  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("read_ends", "lookups", "postings", "hits", "groups", "candidates", "extended", "near_best", "dp_calls", "rows", "batches", "dp_cells")


@pytest.fixture(scope="module")
def geno(built, tmp_path_factory):
    """the genotyper's world (k = 11, N coded as T), its reference as the product loads it, and the restatement's answers"""
    e = sc.Expect(sc.World(11, 3), str(tmp_path_factory.mktemp("seed")))
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(e.fasta)
    assert list(seqs) == list(e.w.alleles)  # nothing merged: the lists are the construction's
    e.ref = (seqs, masks)
    return e


def assign(e, reads, ranges=None, report=True, routes=False, lists=True):
    """the read set assigned range by range (None: as one batch) -> dict: the seed report, the ranges' summed counters, and the context's
    overlaps / coverage / route totals where asked for"""
    ctx = t1k_amd.Context(ref_seq_similarity=0.8)
    try:
        ctx.ref_upload(*e.ref)
        ctx.reads_upload(reads)
        if report:
            ctx.seed_report_enable()
        if routes:
            ctx.route_report_enable()
        tot = {k: 0 for k in COUNTERS}
        for first, count in (ranges or [(0, len(reads))]):
            ctx.assign_range(first, count)
            st = ctx.stats()
            for k in COUNTERS:
                tot[k] += st[k]
        out = dict(stats=tot)
        if report:
            out["report"] = ctx.seed_report()
        if routes:
            out["routes"] = ctx.route_report()[0]
        if lists:
            out["overlaps"] = ctx.overlaps()
            out["coverage"] = ctx.coverage()
    finally:
        ctx.close()
    return out


def want_arrays(e, read):
    f = e.flat(read)
    return (np.array([s for s, _, _ in f], np.uint8), np.array([o for _, o, _ in f], np.uint32), np.array([l for _, _, l in f], np.uint32))


def check_report(e, reads, report, what):
    """every read-end's record equals the restatement's: counts per strand, offsets in order, list lengths, and the masks' bits"""
    seen, counts, masks, ptr, used = report
    assert seen.all(), "%s: read-ends %s were never reported" % (what, np.nonzero(seen == 0)[0][:8])
    kept = {}
    for i, r in enumerate(reads):
        if r not in kept:
            st, off, ln = want_arrays(e, r)
            m = np.zeros((2, t1k_amd.SEED_MASK_WORDS), np.uint32)
            if len(r) <= 320:
                for s, o in zip(st, off):
                    m[s, o >> 5] |= np.uint32(1 << (o & 31))
            kept[r] = (st, off, ln, m, (int((st == 0).sum()), int((st == 1).sum())))
        st, off, ln, m, n01 = kept[r]
        g = used[ptr[i]:ptr[i + 1]]
        where = "%s: read-end %d (%d bases, %s)" % (what, i, len(r), "replay" if e.of(r)["replay"] else "parallel form")
        assert tuple(int(x) for x in counts[i]) == n01, "%s: used k-mers per strand %s, restatement %s" % (where, counts[i], n01)
        assert np.array_equal(g["strand"], st) and np.array_equal(g["read_off"], off), "%s: used offsets differ: kernel %s restatement %s" % (
            where, list(zip(g["strand"].tolist(), g["read_off"].tolist()))[:12], list(zip(st.tolist(), off.tolist()))[:12])
        assert np.array_equal(g["list_len"], ln), "%s: list lengths differ at %s" % (where, np.nonzero(g["list_len"] != ln)[0][:8])
        assert np.array_equal(masks[i], m), "%s: used-offset masks differ" % where


def sums(e, reads):
    return sum(e.of(r)["lookups"] for r in reads), sum(e.of(r)["postings"] for r in reads)


@pytest.fixture(scope="module")
def shapes(geno):
    return dict(geno.w.shapes())


@pytest.mark.parametrize("shape", ["nw5", "nw10", "xlong"])
def test_used_kmers_per_read_end(geno, shapes, shape):
    """1. the three kernel shapes, each as one range: masks of 5 words, of 10 words, and a range with read-ends beyond 320 bases"""
    cs = shapes[shape]
    reads = [c.read for c in cs]
    out = assign(geno, reads, routes=True)
    t = out["routes"]
    assert (t["ranges"], t["ranges_nw5"], t["ranges_nw10"], t["ranges_xlong"]) == {"nw5": (1, 1, 0, 0), "nw10": (1, 0, 1, 0), "xlong": (1, 0, 1, 1)}[shape]
    for i, c in enumerate(cs):  # (named: the first case that differs is the message)
        check_report(geno, [c.read], _one(out["report"], i), "%s / %s" % (shape, c.name))
    want = sums(geno, reads)
    assert (out["stats"]["lookups"], out["stats"]["postings"]) == want, "%s: look-ups, postings %s, restatement %s" % (shape, (out["stats"]["lookups"], out["stats"]["postings"]), want)
    assert out["stats"]["read_ends"] == len(reads)


def _one(report, i):
    """the report cut down to read-end i"""
    seen, counts, masks, ptr, used = report
    return seen[i:i + 1], counts[i:i + 1], masks[i:i + 1], np.array([0, ptr[i + 1] - ptr[i]]), used[ptr[i]:ptr[i + 1]]


def ranges_of(n, size):
    return [(a, min(size, n - a)) for a in range(0, n, size)]


def test_order_and_range_independence(geno, shapes):
    """2. what a workgroup carries from one read-end to the next (sFallback, sUMask, the overlaid accumulators) and from one range to the
    next must not matter: the same read-ends reversed and interleaved (replay / parallel form / too short / long in turn), in ranges of
    1, 7 and 64 -- every read-end's record is the restatement's again, the counters' sums are the same"""
    cs = shapes["xlong"]
    by = {}
    for c in cs:
        r = geno.of(c.read)
        key = "tiny" if len(c.read) <= geno.w.k else "long" if len(c.read) > 320 else "replay" if r["replay"] else "parallel"
        by.setdefault(key, []).append(c.read)
    assert all(by.get(k) for k in ("tiny", "long", "replay", "parallel"))
    inter = []
    for j in range(max(len(v) for v in by.values())):
        inter += [v[j % len(v)] for _, v in sorted(by.items())]
    runs = [("reversed", [c.read for c in cs][::-1], (1, 7, 64)), ("interleaved", inter, (7, 64)), ("short reversed", [c.read for c in shapes["nw5"]][::-1], (7,))]
    for name, reads, sizes in runs:
        want = sums(geno, reads)
        for size in sizes:
            out = assign(geno, reads, ranges=ranges_of(len(reads), size))
            check_report(geno, reads, out["report"], "%s, ranges of %d" % (name, size))
            assert (out["stats"]["lookups"], out["stats"]["postings"]) == want, (name, size)


def test_workgroups_that_take_a_second_read_end(geno, shapes):
    """3. the seeding grid is capped at 32 768 workgroups: in one range of 32 768 + 600 read-ends the last 600 (designed cases) are each the
    second read-end of a workgroup whose first was a short read chosen to leave state behind -- a replay, big runs on both strands, hits"""
    w = geno.w
    rng = random.Random(5)
    pool = []
    for s, en, d in w.spans2:
        pool += [w.R2[s - 5:s + 50], seed_ref.revcomp(w.R2[s - 9:s + 40])]
    for s, en, d in w.spans0:
        pool += [w.B0[s - 3:s + 45]]
    pool += [w.R1[a:a + ln] for a, ln in zip(range(30, 330, 9), [45, 52, 60, 58, 47] * 8)]
    pool += [w.alleles[-2][a:a + 55] for a in (0, 50, 100)] + [sc.rand_seq(random.Random(9), 50), w.R1[200:225] + "N" + w.R1[226:255], w.R1[7:7 + w.k], "ACGT"]
    assert max(len(r) for r in pool) <= 60 and any(geno.of(r)["replay"] for r in pool)
    first = [pool[rng.randrange(len(pool))] for _ in range(32768)]
    designed = [c.read for c in shapes["nw5"]]
    last = [designed[i % len(designed)] for i in range(600)]
    reads = first + last
    out = assign(geno, reads, lists=False)
    check_report(geno, reads, out["report"], "33 368 read-ends")
    assert (out["stats"]["lookups"], out["stats"]["postings"]) == sums(geno, reads)


def test_end_results_equal_the_oracle(geno, shapes):
    """4. overlap lists and coverage of all cases: what a difference in 1-3 would cost downstream"""
    reads = [c.read for c in shapes["xlong"]]
    assert gpu_assign_check.compare(geno.fasta, reads, 0.8, False, "seed cases") == 0


def extract_counts(e, ctx, reads):
    ctx.reads_upload(reads)
    good, st = ctx.extract(1)
    return good, st["lookups"], st["postings"]


@pytest.mark.parametrize("k", [9, 12, 15])
def test_the_extractors_copies(built, tmp_path, k):
    """5. t1k_extract.hip holds the rule twice more (parallel form with three positions a thread, eight when the batch holds a read beyond
    320 bases; the replay), with N coded as A and k/2 + 1 = 5, 7, 8.  Its two counters are per batch: every case alone in a batch, then
    all in one batch at both shapes.  Only the read-ends its screen lets through are seeded: not of low complexity
    (orc_is_low_complexity), at least k bases, and -- with hit_len_required = k, one hit suffices -- some k-mer on either strand with
    a list; the expected counters are the restatement's over those."""
    e = sc.Expect(sc.World(k, 0), str(tmp_path))
    cases = [c for c in e.w.cases]

    def screened(r):
        if len(r) < k or e.orc.low_complexity(r):
            return False
        return any(valid and e.list_len(text) for s in (r, seed_ref.revcomp(r)) for _, text, valid in seed_ref.kmers(s, k, 0))

    def want(reads):
        kept = [r for r in reads if screened(r)]
        return sums(e, kept)

    ctx = t1k_amd.Context(kmer_length=k, hit_len_required=k, ref_seq_similarity=0.8, n_base_code=0)
    try:
        ctx.ref_upload(e.w.alleles)
        assert sum(1 for c in cases if screened(c.read)) > len(cases) // 2
        for c in cases:
            good, lk, po = extract_counts(e, ctx, [c.read])
            assert (lk, po) == want([c.read]), "k = %d, %s (%d bases, %s): look-ups, postings %s, restatement %s" % (
                k, c.name, len(c.read), "replay" if e.of(c.read)["replay"] else "parallel form", (lk, po), want([c.read]))
            assert list(good) == [1 if e.orc.good(c.read) else 0], c.name
        fast = [c.read for c in cases if len(c.read) <= 320]
        every = [c.read for c in cases]
        for name, reads in (("<= 320 bases", fast), ("with long reads", every), ("reversed", every[::-1])):
            good, lk, po = extract_counts(e, ctx, reads)
            assert (lk, po) == want(reads), "k = %d, one batch %s" % (k, name)
            assert list(good) == [1 if e.orc.good(r) else 0 for r in reads], name
    finally:
        ctx.close()
        e.orc.close()


def test_report_off_is_today(geno, shapes):
    """6. the report only reads: overlap bytes, coverage and every counter of a range are the same with it off and on; asking for it while
    it is off is T1K_ERR_STATE"""
    reads = [c.read for c in shapes["xlong"]]
    on, off = assign(geno, reads, report=True), assign(geno, reads, report=False)
    assert np.array_equal(on["overlaps"][0], off["overlaps"][0]) and on["overlaps"][1].tobytes() == off["overlaps"][1].tobytes()
    assert np.array_equal(on["coverage"], off["coverage"])
    assert on["stats"] == off["stats"]
    ctx = t1k_amd.Context(ref_seq_similarity=0.8)
    try:
        with pytest.raises(t1k_amd.T1kError, match=r"t1k_seed_report_get failed \(-5\).*the seed report is off"):
            ctx.seed_report()
        ctx.seed_report_enable()
        ctx.seed_report_enable(False)
        with pytest.raises(t1k_amd.T1kError, match=r"\(-5\)"):
            ctx.seed_report()
    finally:
        ctx.close()
