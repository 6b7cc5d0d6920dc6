"""The two stages every fragment passes before anything is seeded (t1k_dedupe.hip), against their restatement (pytest -m gpu).

t1k_reads_dedupe collapses the identical read-ends of a window; t1k_xwin_link / t1k_xwin_resolve do the same across the windows of a job.
A wrong merge is silent -- a read-end takes another sequence's overlap list, or its weight lands on another representative, and every
later stage agrees with itself -- so everything here is compared with dedupe_ref.py (plain strings and dictionaries) or with a control
context that never collapsed or never linked, integer for integer.  The inputs come from dedupe_cases.py (checked by
test_dedupe_cpu.py): lengths at the 32-base word edges, reads that differ in one base at a word edge, in the N mask alone or in their
length alone, uploads at the edges of S and of the 256-thread blocks, windows of different S, a table too small for its windows.

Both stages compare word by word only where 64-bit hashes are equal, which no input of this size brings about.  The library's test-only
switches T1K_TEST_DEDUPE_HASH_BITS / T1K_TEST_XWIN_HASH_BITS (read once per process) cut the hashes to no bits at all, and the last two
tests run this file again in child processes under each of them: the collapse then merges neighbours only (dedupe_ref.collapse_neighbours,
as exact as collapse), and the table across windows must behave exactly as before -- its compares now decide every probe.

In the table tests a window is a context of its own sharing one reference; the calls follow host/job.cpp: upload, dedupe, link, assign,
resolve, pair.  Coverage is deferred there, as in a job that uses the table."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dedupe_cases as dc
import dedupe_ref as dr
import t1k_amd
import util

pytestmark = pytest.mark.gpu
GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
FIELDS = ("seq_idx", "read_start", "read_end", "seq_start", "seq_end", "strand", "match_cnt", "left_clip", "right_clip", "relaxed_match_cnt", "similarity")
T1K_ERR_ARG, T1K_ERR_STATE = -1, -5
COLLIDING = os.environ.get("T1K_TEST_DEDUPE_HASH_BITS") == "0"   # as t1k_dedupe.hip reads it: every read-end has the same hash
restate = dr.collapse_neighbours if COLLIDING else dr.collapse


# ---- t1k_reads_dedupe on the packed layout's edges ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(built):
    """one context for every batch without a reference: the bDedup* buffers and the scratch are reused from batch to batch"""
    ctx = t1k_amd.Context()
    yield ctx
    ctx.close()


def collapse_and_compare(ctx, reads, weights=None):
    ctx.reads_upload(reads, weights)
    got = ctx.reads_dedupe()
    want, reps, _ = restate(reads, weights)
    assert ctx.n_read_ends == len(reps), "%d distinct read-ends, the restatement has %d" % (ctx.n_read_ends, len(reps))
    diff = np.nonzero(got != np.asarray(want, np.uint32))[0]
    assert len(diff) == 0, "distinct_of differs at %d of %d read-ends, first at %d: %d, the restatement has %d (%r)" % (
        len(diff), len(reads), diff[0], got[diff[0]], want[diff[0]], reads[diff[0]][:50])
    return got, reps


@pytest.mark.parametrize("L", dc.LENGTHS)
def test_length_family(plain, L):
    """a sequence of L bases and its near twins -- another base or N at the first base, the last base, index 31, index 32; one A or 32 A more;
    a lower-case base or R for N -- numbered exactly as the restatement numbers them"""
    collapse_and_compare(plain, dc.family_batch(L))


@pytest.mark.parametrize("L", dc.LENGTHS)
def test_twins_as_neighbours(plain, L):
    """the same family with every pair of twins side by side, and every alias beside its member: the order in which the compare of
    k_dedupe_mark meets them when their hashes are equal"""
    collapse_and_compare(plain, dc.twin_neighbours(L))


@pytest.mark.parametrize("longest,S", dc.S_OF_LONGEST)
def test_stride_set_by_the_longest_read(plain, longest, S):
    """uploads whose longest read puts S at 2, 2, 3, 11, 12 and 33, short reads beside it: their spare words neither tell equal reads apart nor
    merge different ones"""
    reads = dc.s_batch(longest)
    assert dc.stride(reads) == S
    collapse_and_compare(plain, reads)


@pytest.mark.parametrize("n", dc.SIZES)
def test_batch_size(plain, n):
    """1, 2, 255, 256, 257 and 65 537 read-ends of 40 bases: the edges of the 256-thread blocks and of a 16-bit count"""
    collapse_and_compare(plain, dc.size_batch(n))


def test_all_identical_all_distinct_and_long_runs(plain):
    got, reps = collapse_and_compare(plain, dc.all_identical())
    assert reps == [0] and not got.any()
    got, reps = collapse_and_compare(plain, dc.all_distinct())
    assert reps == list(range(257)) and list(got) == list(range(257))
    reads, counts = dc.multiplicities()
    got, reps = collapse_and_compare(plain, reads)
    if not COLLIDING:
        assert sorted(np.bincount(got).tolist()) == sorted(counts.values())
    got, reps = collapse_and_compare(plain, sorted(reads))
    assert sorted(np.bincount(got).tolist()) == sorted(counts.values())   # runs of 1 .. 300 neighbours


def test_no_read_ends(plain):
    """n = 0: 0 distinct, and the caller's array is not written"""
    plain.reads_upload([])
    out = np.full(4, 0xABABABAB, np.uint32)
    nd = C.c_uint32(77)
    assert t1k_amd.lib().t1k_reads_dedupe(plain.h, out.ctypes.data_as(C.c_void_p), C.byref(nd)) == 0
    assert nd.value == 0 and (out == 0xABABABAB).all()
    assert len(plain.reads_dedupe()) == 0 and plain.n_read_ends == 0
    collapse_and_compare(plain, dc.family_batch(33))   # ... and the context goes on


def test_shared_reads_are_refused(plain):
    plain.reads_upload(dc.family_batch(32))
    other = t1k_amd.Context()
    try:
        other.reads_share(plain)
        with pytest.raises(t1k_amd.T1kError, match=r"t1k_reads_dedupe failed \(%d\).*aliases another context's reads" % T1K_ERR_STATE):
            other.reads_dedupe()
        collapse_and_compare(plain, dc.family_batch(32))   # the owner still can
    finally:
        other.close()


# ---- the collapsed set assigns as the un-collapsed reads do ------------------------------------------------------------------
class World:
    """a small synthetic reference on the GPU and contexts that share it"""

    def __init__(self, tmp, kind, **kw):
        self.ref = os.path.join(tmp, kind + ".fa")
        util.synth_ref(kind, self.ref, genes=3 if kind == "ref-rna" else 2, scale=0.05, seed=41)
        _, self.seqs, self.masks, _ = t1k_amd.load_reference_fasta(self.ref)
        self.kw = dict(kw, store_chunk_mb=64)
        self.root = t1k_amd.Context(**self.kw)
        self.root.ref_upload(self.seqs, self.masks)
        self.made = []

    def ctx(self, deferred=False):
        c = t1k_amd.Context(**self.kw)
        c.ref_share(self.root)
        c.set_coverage_mode(deferred)
        self.made.append(c)
        return c

    def release(self, *ctxs):
        for c in ctxs:
            c.close()
            self.made.remove(c)

    def close(self):
        for c in self.made:
            c.close()
        self.root.close()


@pytest.fixture(scope="module")
def worlds(built, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dedupe"))
    w = {"rna": World(tmp, "ref-rna", ref_seq_similarity=0.97), "dna": World(tmp, "ref-dna", ref_seq_similarity=0.9, relax_intron_align=1)}
    assert all(max(len(s) for s in x.seqs) >= 1000 for x in w.values())
    yield w
    for x in w.values():
        x.close()


_aligning = {}


def aligning(worlds, kind):
    """the aligning reads of a world and what contexts that never collapsed make of them, computed once: the overlap lists of the reads as
    uploaded, their coverage, and the coverage of the reads expanded by their weights"""
    if kind not in _aligning:
        w = worlds[kind]
        reads, weights = dc.aligning_reads(w.seqs, 4000 + len(kind), 100, 260, (40, 75, 100, 150, 150, 150, 321, 1000), fixed=(1000, 1000, 999, 0, 32, 64, 160, 1))
        reads += [reads[0], reads[0].lower()]        # (once more with weight 0, and in lower case: all N, a read-end of its own)
        weights += [0, 3]
        full = w.ctx()
        full.reads_upload(reads)
        full.assign()
        cnt, ovl = full.overlaps()
        cov = full.coverage()
        full.coverage_reset()
        full.reads_upload(dc.expand(reads, weights))
        full.assign()
        cov_w = full.coverage()
        w.release(full)
        # (an allele of the dna reference has a separator every 450 .. 700 bases: its reads of 1000 bases hold one and get no list)
        assert cov.any() and cov_w.any() and any(cnt[i] for i, r in enumerate(reads) if len(r) >= (999 if kind == "rna" else 321)), "the reads do not align"
        _aligning[kind] = (reads, weights, cnt, ovl, cov, cov_w)
    return _aligning[kind]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit_weights", "uploaded_weights"])
@pytest.mark.parametrize("kind", ["rna", "dna"])
def test_collapsed_set_assigns_as_the_uncollapsed_reads(worlds, kind, weighted):
    """reads of 0 .. 1000 bases drawn from the reference (S = 33), with repeats and weights 0 .. 5: after the collapse the list of EVERY
    distinct read-end is the list its representative gets when every read-end is assigned, and the coverage is that of the reads
    repeated by their weights -- the only observable of k_dedupe_scatter's sums and of k_dedupe_gather"""
    reads, weights, cnt_full, ovl_full, cov, cov_w = aligning(worlds, kind)
    ctx = worlds[kind].ctx()
    _, reps = collapse_and_compare(ctx, reads, weights if weighted else None)
    ctx.assign()
    cnt, ovl = ctx.overlaps()
    start = np.concatenate([[0], np.cumsum(cnt_full)]).astype(np.int64)
    assert np.array_equal(cnt, cnt_full[reps])
    want = np.concatenate([ovl_full[start[r]:start[r + 1]] for r in reps])
    for f in FIELDS:
        assert np.array_equal(want[f], ovl[f]), f
    got = ctx.coverage()
    want_cov = cov_w if weighted else cov
    assert np.array_equal(got, want_cov), "coverage differs at %d bases (sum %d, expected %d)" % ((got != want_cov).sum(), got.sum(), want_cov.sum())
    # a second, shorter upload into the same context (S = 6 after 33, fewer read-ends): nothing of the previous batch is left
    short = [r for r in reads if len(r) <= 150][:120]
    sw = [(3 * i) % 6 for i in range(len(short))]
    _, reps = collapse_and_compare(ctx, short, sw if weighted else None)
    ctx.coverage_reset()
    ctx.assign()
    cnt2, _ = ctx.overlaps()
    index = {r: i for i, r in reversed(list(enumerate(reads)))}
    assert np.array_equal(cnt2, cnt_full[[index[short[r]] for r in reps]])
    ref = worlds[kind].ctx()
    ref.reads_upload(dc.expand(short, sw) if weighted else short)
    ref.assign()
    assert np.array_equal(ctx.coverage(), ref.coverage())
    worlds[kind].release(ctx, ref)


# ---- t1k_xwin_*: identical read-ends across windows ---------------------------------------------------------------------------------
def run_window(world, reads, weights, table=None, w=0):
    """one window as host/job.cpp runs it (single-ended fragments, one per read-end); table = None: the control, assigned alone"""
    c = world.ctx(deferred=True)
    c.reads_upload(reads, weights)
    d = c.reads_dedupe()
    n_distinct = c.n_read_ends
    linked = table.link(c, w) if table is not None else 0
    c.assign()
    lookups = c.stats()["lookups"]
    if table is not None:
        table.resolve(c, w)
    c.pair(d, None, [1 if "N" in r else 0 for r in reads])
    counts, assigned, rows = c.rows()
    made = c.overlaps()[0]   # (the lists this context made itself: none for a linked read-end)
    return dict(ctx=c, d=d, n_distinct=n_distinct, linked=linked, lookups=lookups, counts=counts, assigned=assigned, rows=rows, made=made)


def coverage_of(world, runs):
    """per run: the coverage of its read set with all alleles selected, on a context of its own (the read sets stay alive until all are
    scanned: a linked entry points into an earlier window's store)"""
    sets = [r["ctx"].detach_readset() for r in runs]
    cov = world.ctx()
    sel = np.ones(len(world.seqs), np.uint8)
    out = []
    for rs in sets:
        cov.coverage_reset()
        cov.coverage_selected(rs, sel)
        out.append(cov.coverage())
    cov.coverage_reset()
    for rs in sets:
        cov.coverage_selected(rs, sel)
    total = cov.coverage()
    for rs in sets:
        rs.close()
    world.release(cov)
    return out, total


def same_rows(a, b):
    return np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["assigned"], b["assigned"]) and a["rows"].tobytes() == b["rows"].tobytes()


_xwin = {}


def xwin_run(worlds, kind):
    """the four windows of dedupe_cases.xwin_windows through one table, and each of them alone"""
    if kind not in _xwin:
        world = worlds[kind]
        windows, marked = dc.xwin_windows(world.seqs)
        distinct = [[reads[i] for i in dr.collapse(reads)[1]] for reads, _ in windows]
        table = t1k_amd.Xwin(world.root, sum(len(d) for d in distinct), len(windows))   # sized by the true total
        runs = [run_window(world, reads, weights, table, w) for w, (reads, weights) in enumerate(windows)]
        controls = [run_window(world, reads, weights) for reads, weights in windows]
        _, cov_total = coverage_of(world, runs)
        cov_each, cov_sum = coverage_of(world, controls)
        table.close()
        world.release(*[r.pop("ctx") for r in runs + controls])
        _xwin[kind] = dict(windows=windows, marked=marked, distinct=distinct, runs=runs, controls=controls, cov_total=cov_total, cov_each=cov_each, cov_sum=cov_sum)
    return _xwin[kind]


@pytest.mark.parametrize("kind", ["rna", "dna"])
def test_xwin_link_counts_are_exact(worlds, kind):
    """windows whose longest reads are 150, 1000, 40 and 160 bases (S = 6, 33, 3, 6; the fourth repeats the 160-base reads, which only the second
    can hold): every window links exactly the distinct read-ends whose sequence an earlier window holds -- repeats of 0, 32, 64 and 160 bases
    among them -- and none of the near twins"""
    x = xwin_run(worlds, kind)
    want = dr.link(x["distinct"])
    for w, run in enumerate(x["runs"]):
        assert run["n_distinct"] == len(x["distinct"][w]) == x["controls"][w]["n_distinct"]
        assert run["linked"] == len(want[w][0]), "window %d links %d read-ends, the restatement %d" % (w, run["linked"], len(want[w][0]))
    assert x["runs"][0]["linked"] == 0 and all(len(want[w][0]) > 0 for w in (1, 2, 3))


@pytest.mark.parametrize("kind", ["rna", "dna"])
def test_xwin_linked_read_ends_get_their_lists(worlds, kind):
    """after resolve every fragment of every window pairs to the rows of the control that assigned the window alone (rna: lists published by
    k_select in the packed form; dna, --relaxIntronAlign: by k_publish_lists) -- a linked read-end that took the wrong list, an empty one, or
    one the window should have made itself shows here -- and a window with linked read-ends looked up fewer k-mers than its control: the
    skipped read-ends were not seeded"""
    x = xwin_run(worlds, kind)
    for w, (run, ctl) in enumerate(zip(x["runs"], x["controls"])):
        assert np.array_equal(run["d"], ctl["d"])
        assert same_rows(run, ctl), "window %d: rows differ from the control's" % w
        assert ctl["rows"].size > 0 and ctl["assigned"].any()
        assert ctl["made"][0] == 0 and ctl["made"].any()        # read-end 0 has no list, others have
        want = dr.link(x["distinct"])[w][0]
        assert all(run["made"][d] == (0 if d in want else ctl["made"][d]) for d in range(run["n_distinct"]))   # a linked read-end was not assigned here
        if w == 0:
            assert run["lookups"] == ctl["lookups"] > 0
        else:
            assert run["lookups"] < ctl["lookups"], "window %d: %d look-ups with %d read-ends linked, %d alone" % (w, run["lookups"], run["linked"], ctl["lookups"])


@pytest.mark.parametrize("kind", ["rna", "dna"])
def test_xwin_coverage_counts_each_window_with_its_own_weights(worlds, kind):
    """the deferred coverage pass over the kept windows: the sum of the controls' coverage, integer for integer; the read window 0 holds 3
    times and window 2 holds 5 times (linked there) counts 8"""
    x = xwin_run(worlds, kind)
    assert np.array_equal(x["cov_sum"], np.sum(x["cov_each"], axis=0, dtype=np.int64).astype(np.int32))
    assert x["cov_sum"].any()
    diff = x["cov_total"] != x["cov_sum"]
    assert not diff.any(), "coverage differs at %d bases (sum %d, the controls' %d)" % (diff.sum(), x["cov_total"].sum(), x["cov_sum"].sum())
    # the marked read alone: windows that hold nothing else
    world, marked = worlds[kind], x["marked"]
    table = t1k_amd.Xwin(world.root, 16, 3)
    runs = [run_window(world, [marked] * 3, None, table, 0), run_window(world, ["ACGT"], None, table, 1), run_window(world, [marked] * 5, None, table, 2)]
    assert [r["linked"] for r in runs] == [0, 0, 1]
    each, total = coverage_of(world, runs)
    one = run_window(world, [marked], None)
    (unit,), _ = coverage_of(world, [one])
    assert unit.any() and np.array_equal(each[0], 3 * unit) and np.array_equal(each[2], 5 * unit) and np.array_equal(total, 8 * unit)
    table.close()
    world.release(*[r["ctx"] for r in runs + [one]])


def test_xwin_undersized_table(worlds):
    """a table of 1024 slots (maxReadEnds = 8) for 1 500 distinct read-ends, then a window that repeats 500 of them beside 500 new ones: an
    optimisation must not end the job.  Every call returns OK; the insert gives up on 476 read-ends, which stay unknown, so the second
    window links at most 500 and at least 500 - 476; rows and coverage are the controls'"""
    world = worlds["rna"]
    first, second = dc.undersized_windows(world.seqs)
    table = t1k_amd.Xwin(world.root, 8, 2)
    runs = [run_window(world, first, None, table, 0), run_window(world, second, None, table, 1)]
    controls = [run_window(world, first, None), run_window(world, second, None)]
    assert runs[0]["linked"] == 0 and 24 <= runs[1]["linked"] <= 500, runs[1]["linked"]
    for w in (0, 1):
        assert runs[w]["n_distinct"] == len((first, second)[w])
        assert same_rows(runs[w], controls[w]), w
    assert controls[1]["rows"].size > 0
    _, total = coverage_of(world, runs)
    _, want = coverage_of(world, controls)
    assert want.any() and np.array_equal(total, want)
    table.close()
    world.release(*[r["ctx"] for r in runs + controls])


def test_xwin_arguments(worlds):
    """a window number past maxWindows and a reader that aliases another context's reads are refused with T1K_ERR_ARG and leave the table
    usable; an empty window links nothing and its resolve is a no-op"""
    world = worlds["rna"]
    reads = dc.family_batch(33)
    table = t1k_amd.Xwin(world.root, 1000, 3)
    a = world.ctx(deferred=True)
    a.reads_upload(reads)
    a.reads_dedupe()
    assert table.link(a, 3, raw=True) == (T1K_ERR_ARG, 0) and "bad arguments" in table.last_error()
    assert table.resolve(a, 3, raw=True) == T1K_ERR_ARG
    with pytest.raises(t1k_amd.T1kError, match=r"t1k_xwin_link failed \(-1\)"):
        table.link(a, 7)
    alias = world.ctx(deferred=True)
    alias.reads_share(a)
    assert table.link(alias, 0, raw=True) == (T1K_ERR_ARG, 0)
    assert table.link(a, 0) == 0                       # nothing of the refused calls is in the table
    a.assign()
    table.resolve(a, 0)
    empty = world.ctx(deferred=True)
    empty.reads_upload([])
    empty.reads_dedupe()
    assert table.link(empty, 1) == 0
    table.resolve(empty, 1)
    b = world.ctx(deferred=True)
    b.reads_upload(reads[::-1] + ["ACGTTGCA"])
    b.reads_dedupe()
    assert table.link(b, 2) == a.n_read_ends == b.n_read_ends - 1   # the table still knows window 0, and only that
    b.assign()
    table.resolve(b, 2)
    table.close()
    world.release(a, alias, empty, b)


# ---- the job: windows of differing S ---------------------------------------------------------------------------------------
def test_job_links_across_windows_of_differing_stride(worlds, tmp_path):
    """a paired sample on the dna reference cut into windows of 8 .. 32 fragments whose longest reads are 150, 1000 and 40 bases (S = 6, 33, 3:
    dedupe_cases.job_fragments), later fragments repeating mates of earlier ones: every output file, --outputReadAssignment included, equals
    the single-window run's and the run's without the table, and the table saves distinct read-ends"""
    world = worlds["dna"]
    frags = dc.job_fragments(world.seqs)
    for m in (0, 1):
        with open(str(tmp_path / ("r_%d.fq" % (m + 1))), "w") as f:
            for i, fr in enumerate(frags):
                f.write("@f%d/%d\n%s\n+\n%s\n" % (i, m + 1, fr[m], "I" * len(fr[m])))
    args = [GENO, "-f", world.ref, "-1", str(tmp_path / "r_1.fq"), "-2", str(tmp_path / "r_2.fq"), "-s", "0.9", "--relaxIntronAlign", "--outputReadAssignment"]
    small = dict(T1K_FIRST_WINDOW="8", T1K_WINDOW="32", T1K_WINDOW_GROWTH="1", T1K_BATCH="8", T1K_PAIR_BATCH="8", T1K_DEBUG_PHASES="1")
    err = {}
    for tag, env in (("one", dict(T1K_DEBUG_PHASES="1")), ("on", small), ("off", dict(small, T1K_CROSS_WINDOW="0"))):
        r = subprocess.run(args + ["-o", str(tmp_path / tag)], stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        err[tag] = r.stderr
    windows = {tag: int(re.search(r"(\d+) windows,", err[tag]).group(1)) for tag in err}
    # 184 fragments in windows of at most 32 after a first one of 8: the first holds 150-base reads only, every window cut from fragments
    # 8 .. 79 holds a 1000-base read, and a window lies inside the 40-base fragments 80 .. 183 (see dedupe_cases.job_fragments)
    assert windows["one"] == 1 and windows["on"] >= 3 and windows["off"] >= 3, windows
    sufs = ("_genotype.tsv", "_allele.tsv", "_assign.tsv", "_aligned_1.fa", "_aligned_2.fa")
    one = {s: open(str(tmp_path / "one") + s, "rb").read() for s in sufs}
    assert len(one["_aligned_1.fa"]) > 1000 and len(one["_assign.tsv"]) > 1000
    for tag in ("on", "off"):
        for s in sufs:
            assert open(str(tmp_path / tag) + s, "rb").read() == one[s], (tag, s)
    d_on, d_off = (int(re.search(r"read-ends -> (\d+) distinct", err[t]).group(1)) for t in ("on", "off"))
    assert d_on < d_off, (d_on, d_off)


# ---- the compares behind the hashes ------------------------------------------------------------------------------------------
def again_in_a_child_process(env, select):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select],
                       env=dict(os.environ, **env), cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-6000:]


def test_collapse_with_colliding_hashes_in_a_child_process(built):
    """T1K_TEST_DEDUPE_HASH_BITS=0 in a fresh process: every read-end has the same hash, so k_dedupe_mark's compare of length, bases and N
    mask decides alone and only neighbours merge.  The family, stride, size and aligning tests above run there against
    dedupe_ref.collapse_neighbours -- numbering, lists of every distinct read-end, coverage with and without weights"""
    if os.environ.get("T1K_TEST_DEDUPE_HASH_BITS") is not None or os.environ.get("T1K_TEST_XWIN_HASH_BITS") is not None:
        return
    again_in_a_child_process({"T1K_TEST_DEDUPE_HASH_BITS": "0"}, "not child_process and not xwin and not job")


def test_xwin_with_colliding_hashes_in_a_child_process(built):
    """T1K_TEST_XWIN_HASH_BITS=0 in a fresh process: every key of the table is the same, every look-up walks the whole chain and xwinSame decides
    each probe.  The table tests above run there unchanged: the same exact link counts, rows and coverage"""
    if os.environ.get("T1K_TEST_DEDUPE_HASH_BITS") is not None or os.environ.get("T1K_TEST_XWIN_HASH_BITS") is not None:
        return
    again_in_a_child_process({"T1K_TEST_XWIN_HASH_BITS": "0"}, "xwin and not child_process")
