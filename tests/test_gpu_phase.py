"""GPU tests of the read-backed phasing of site pairs (t1k_phase_*, analyzer --phase): the kernels and the fold against the
sequential restatement, every cell and both counts exactly, on a generated table and on hand-built inputs at the kernels' step edges; the
argument errors, none of which may change the table; the analyzer's file against the restatement fed with the CPU oracle's alignments,
line for line; two unknown bases that are always carried together; its sums against --pileup; every other output unchanged; the golden
chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import phase_ref as ref
import pileup_ref
import util
import t1k_amd
from test_variants_host import oracle_dump, parse_dump

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -3, -5
NO = ref.NO_MATE


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(*ref.table_args(table))


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _kernel(ctx, t, cuts=()):
    keys, counts, ms, stats = ctx.phase(t.allele_off, t.site_allele, t.site_pos, t.aln, t.book_rec, t.book_uniq, t.text, t.ops, cuts=cuts)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (counts > 0).all()         # runs ascending by key, one per key
    return ref.from_runs(keys, counts, len(t.site_allele)), ms, stats


# ---- 1. kernels = restatement --------------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement(ctx, table, want):
    got, ms, stats = _kernel(ctx, table)
    print(stats)
    assert 200000 <= want[1].keys <= 5000000 and len(want[0]) > 50000
    assert ref.same(got, want[0]) and want[1].same(stats)
    assert ms > 0 and stats["folds"] == 1


def test_three_calls_give_the_same_table(ctx, table, want):
    got, _, stats = _kernel(ctx, table, cuts=(2001, 6000))
    assert ref.same(got, want[0]) and want[1].observations * 3 == stats["observations"]          # (every call walks all the records)
    assert (want[1].bookings, want[1].keys, want[1].discordant) == (stats["bookings"], stats["keys"], stats["discordant"])


def test_several_folds_give_the_same_table(ctx, table, want, monkeypatch):
    monkeypatch.setenv("T1K_PHASE_PENDING", "1000")           # every one of the five calls emits more: a fold behind each
    got, _, stats = _kernel(ctx, table, cuts=(1800, 3600, 5400, 7200))
    assert stats["folds"] >= 3 and ref.same(got, want[0])


def test_no_sites_gives_no_runs(ctx, table):
    none = np.zeros(0, np.uint32)
    keys, counts, _, stats = ctx.phase(table.allele_off, none, none, table.aln, table.book_rec, table.book_uniq, table.text, table.ops)
    assert len(keys) == 0 and len(counts) == 0 and stats["folds"] == 0 and stats["observations"] == 0


# ---- 2. the step edges of the list kernels, by hand ----------------------------------------------------------------------------------
class Edges:
    """two alleles of 300 and 70 bases; sites: positions 0 .. 139 of the first (bits 63 and 64 of the bitmap among them) and its last,
    the first and the last of the second.  Records of matches only: .rec(allele, start, n, text) covers n positions from `start`"""

    def __init__(self):
        self.allele_off = pileup_ref.offsets([300, 70])
        self.site_allele = np.array([0] * 141 + [1, 1], np.uint32)
        self.site_pos = np.array(list(range(140)) + [299, 0, 69], np.uint32)
        rng = np.random.default_rng(5)
        one = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 300)]
        other = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), one)]     # every base another one
        self.text = np.concatenate([one, other])
        self.ops = np.zeros(300, np.int8)
        self.recs, self.books = [], []

    def rec(self, allele, start, n, other=False):
        self.recs.append((allele, start, start + (300 if other else 0), 0, n, 0, 0, 0))
        return len(self.recs) - 1

    def book(self, r1, r2=NO, uniq=0):
        self.books.append((r1, r2, uniq))

    def done(self):
        self.aln = np.array(self.recs, t1k_amd.PILEUP_ALN_DTYPE)
        self.book_rec = np.array([b[:2] for b in self.books], np.uint32)
        self.book_uniq = np.array([b[2] for b in self.books], np.uint8)
        return self


def _m(t):
    """per booking: its merged observations and its discordant sites, from the restatement"""
    b, _, _, disc, _ = ref.merged(*ref.table_args(t))
    return np.bincount(b, minlength=len(t.book_uniq)).tolist(), disc.tolist()


def _check(ctx, t, m=None, disc=None, cuts=()):
    want, st = ref.restate(*ref.table_args(t))
    if m is not None:
        assert _m(t) == (m, disc if disc is not None else [0] * len(m))
    got, _, stats = _kernel(ctx, t, cuts=cuts)
    assert ref.same(got, want) and sum(int(c[0]) for c in want.values()) == st.keys
    if not cuts:
        assert st.same(stats)
    return want, stats


def test_hit_counts_at_the_ballot_steps(ctx):
    t = Edges()
    for i, h in enumerate((0, 1, 63, 64, 65, 129)):
        t.book(t.rec(0, 150, 20) if h == 0 else t.rec(0, i, h), uniq=i & 1)             # every record alone: m = h
    t.book(1, 0)                                                                         # h = 1 with a mate that observes nothing
    _check(ctx, t.done(), m=[0, 1, 63, 64, 65, 129, 1])


def test_merged_sizes_across_the_pair_stride(ctx):
    t = Edges()
    t.book(t.rec(0, 0, 1), t.rec(0, 5, 1), 1)                # 2
    t.book(t.rec(0, 0, 64), t.rec(0, 64, 1))                 # 65
    t.book(t.rec(0, 1, 65), t.rec(0, 66, 1), 1)              # 66
    t.book(t.rec(0, 70, 65), t.rec(0, 5, 65))                # 130, list 2 in front of list 1: the pairs order themselves
    t.book(t.rec(0, 0, 100), t.rec(0, 60, 80))               # 140, overlapping on 40 sites in equal states
    want, stats = _check(ctx, t.done(), m=[2, 65, 66, 130, 140])
    assert stats["keys"] == 1 + 65 * 32 + 33 * 65 + 65 * 129 + 70 * 139 and stats["bookings"] == 5


def test_mates_on_the_same_sites(ctx):
    t = Edges()
    a, b, c = t.rec(0, 3, 70), t.rec(0, 3, 70), t.rec(0, 3, 70, other=True)
    t.book(a, b, 1)                                          # equal states everywhere: m = h
    t.book(a, c)                                             # different states everywhere: m = 0, every site discordant
    t.book(a, a)                                             # rec1 == rec2: the record's own list
    t.book(c, t.rec(0, 50, 90, other=True), 1)               # 23 sites shared and equal, 3 .. 139 in all
    want, stats = _check(ctx, t.done(), m=[70, 0, 70, 137], disc=[0, 70, 0, 0])
    assert stats["discordant"] == 70 and stats["bookings"] == 3


def test_sites_at_word_seams_and_allele_ends(ctx):
    t = Edges()
    t.book(t.rec(0, 63, 1), t.rec(0, 64, 1), 1)              # bit 63 and bit 64 of the bitmap
    t.book(t.rec(0, 139, 161))                               # the last dense site and the allele's last position
    t.book(t.rec(1, 0, 70), uniq=1)                          # the second allele, first and last position (bits 300 and 369)
    t.book(t.rec(1, 0, 1), t.rec(1, 69, 1))
    want, _ = _check(ctx, t.done(), m=[2, 2, 2, 2])
    assert sorted((s, u) for s, u, _, _ in want) == [(63, 64), (139, 140), (141, 142)] and want[next(k for k in want if k[0] == 141)].tolist() == [2, 1]


def test_a_long_read_with_every_position_a_site(ctx):
    t = Edges()
    t.allele_off = pileup_ref.offsets([1000])
    t.site_allele, t.site_pos = np.zeros(1000, np.uint32), np.arange(1000, dtype=np.uint32)
    rng = np.random.default_rng(9)
    t.text = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, 1000)]
    t.ops = np.zeros(1000, np.int8)
    t.recs.append((0, 0, 0, 0, 1000, 0, 0, 0))
    t.book(0, uniq=1)
    want, stats = _check(ctx, t.done(), m=[1000])
    assert stats["keys"] == 1000 * 999 // 2 == len(want)


def test_fold_merges_a_folded_count_with_pending_keys(ctx, monkeypatch):
    monkeypatch.setenv("T1K_PHASE_PENDING", "1")              # a fold behind each of the two calls
    t = Edges()
    a = t.rec(0, 0, 3)
    for _ in range(4):
        t.book(a)
    t.book(t.rec(0, 0, 2), uniq=1)
    want, stats = _check(ctx, t.done(), cuts=(2,))
    assert stats["folds"] == 2 and sorted(c.tolist() for c in want.values()) == [[4, 0], [4, 0], [5, 1]]


def test_a_second_session_holds_no_more_device_memory(ctx):
    """_end frees every block of the stage: what the context holds behind one begin / add / get / end (its scan and sort scratch stays, by
    design) is what it holds behind the next"""
    t = Edges()
    t.book(t.rec(0, 0, 3))
    _kernel(ctx, t.done())
    held = ctx.mem_bytes()
    _kernel(ctx, t)
    assert ctx.mem_bytes() == held


# ---- 3. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_table_alone(built):
    c = t1k_amd.Context()
    try:
        off = pileup_ref.offsets([8, 5])
        sa, sp = np.array([0, 0, 1, 1], np.uint32), np.array([1, 7, 0, 4], np.uint32)
        text = b"ACGTACGTAC"
        ops = np.array([0, 0, 1, 0, 0, 4, 0, 0], np.int8)

        def rec(allele=0, seq_start=0, read_at=0, ops_at=0, n_ops=5):
            return np.array([(allele, seq_start, read_at, ops_at, n_ops, 0, 0, 0)], t1k_amd.PILEUP_ALN_DTYPE)

        def table():
            return ref.from_runs(*c.phase_get(), len(sa))
        assert c.phase_add(rec(), [[0, NO]], [1], text, ops, raw=True) == ERR_STATE and c.last_error().startswith("t1k_phase_add: ")   # add / get / stats / end before begin
        assert c.phase_get(raw=True) == ERR_STATE and c.phase_stats(raw=True) == ERR_STATE and c.phase_end(raw=True) == ERR_STATE
        for bad_a, bad_p in (([0, 0], [7, 1]), ([1, 0], [0, 1]), ([0, 0], [3, 3]), ([0], [8]), ([2], [0])):
            assert c.phase_begin(off, np.array(bad_a, np.uint32), np.array(bad_p, np.uint32), raw=True) == ERR_ARG
        many = np.zeros((1 << 28) + 1, np.uint32)                                                # (never touched: the count alone is refused)
        assert c.phase_begin(off, many, many, raw=True) == ERR_CAPACITY
        del many
        assert c.phase_get(raw=True) == ERR_STATE                                                # none of them opened a table
        c.phase_begin(off, sa, sp)
        assert table() == {}
        assert c.phase_begin(off, sa, sp, raw=True) == ERR_STATE                                 # a table is open
        good = np.concatenate([rec(n_ops=5), rec(seq_start=3, read_at=3, n_ops=5), rec(allele=1, read_at=5, n_ops=5)])
        gr, gu = [[0, 1], [2, NO]], [1, 0]
        assert c.phase_add(good, gr, gu, text, ops, raw=True) == 0
        before = table()
        assert ref.same(before, ref.restate(off, good, gr, gu, text, ops, sa, sp)[0]) and sum(int(v[0]) for v in before.values()) == 2
        stats = c.phase_stats()

        def refused(bad, book=(3, NO), code=ERR_ARG):
            assert c.phase_add(np.concatenate([good, bad]), gr + [list(book)], gu + [0], text, ops, raw=True) == code   # the sound bookings of the call emit nothing either
            assert c.last_error().startswith("t1k_phase_add: ")                                   # whoever refused it, host or device
            assert ref.same(table(), before) and c.phase_stats() == stats
        refused(rec(), book=(4, NO))                      # a record index equal to n
        refused(rec(), book=(3, 4))                       # ... as the mate
        refused(rec(), book=(3, 2))                       # mates on different alleles
        refused(rec(ops_at=3, n_ops=5))                   # op value 4
        refused(rec(allele=1, seq_start=1, n_ops=5))      # a walk one base past the allele (5 bases from position 1 of 5)
        refused(rec(seq_start=4, n_ops=5))                # ... of the first allele (the site bitmap continues into the second's)
        refused(rec(read_at=6, n_ops=5))                  # a walk past `text`
        refused(rec(allele=2))                            # an allele id equal to nAlleles
        refused(rec(ops_at=4, n_ops=5))                   # an edit string that leaves `ops`
        refused(rec(ops_at=3, n_ops=5), book=(0, NO))     # a bad record is refused even when no booking names it
        more = (rec(allele=1, read_at=5), [[0, 0]], [1])
        assert c.phase_add(*more, text, ops, raw=True) == 0                                      # and the table still takes sound calls
        both = ref.restate(off, np.concatenate([good, more[0]]), gr + [[3, 3]], gu + [1], text, ops, sa, sp)[0]
        assert ref.same(table(), both) and both[(2, 3, 1, 1)].tolist() == [2, 1]
        c.phase_end()
        assert c.phase_add(rec(), [[0, NO]], [1], text, ops, raw=True) == ERR_STATE
    finally:
        c.close()


# ---- the analyzer --------------------------------------------------------------------------------------------------------------------
def _run(cmd, env=None, ok=True):
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def _genotype(tmp, ref_fa, pfx, single=False):
    g = os.path.join(tmp, "g")
    reads = ["-u", pfx + "_1.fq"] if single else ["-1", pfx + "_1.fq", "-2", pfx + "_2.fq"]
    _run([GENO, "-f", ref_fa] + reads + ["--barcode", pfx + "_bc.fa", "-o", g])
    return g, (["-u", g + "_aligned.fa"] if single else ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"])


def _analyze(ref_fa, g, aligned, out, extra=(), env=None, ok=True, barcode=True):
    return _run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv"] + aligned + (["--barcode", g + "_aligned_bc.fa"] if barcode else []) + ["-o", out, "-t", "4"] + list(extra), env, ok)


def _read(path):
    return open(path, "rb").read()


def _vcf(path):
    """rows of _allele.vcf: (allele name, 0-based ref_pos, ref base, var base)"""
    return [(v[0], int(v[-2]), v[3], v[4]) for v in (l.split(" ") for l in open(path).read().split("\n") if l)]


def _var_of(path, idx):
    var_of = {}
    for name, pos, _, var in _vcf(path):
        var_of[(idx[name], pos)] = var_of[(idx[name], pos)] + "," + var if (idx[name], pos) in var_of else var
    return var_of


# ---- 4. analyzer = restatement on the CPU oracle's alignments; 6. sanity against --pileup --------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
def test_analyzer_equals_restatement_on_the_oracles_alignments(built, tmp_path, single):
    tmp = str(tmp_path)
    ref_fa, pfx = util.several_snps_sample(tmp, 29, genes=3, pairs=2500) if single else util.several_snps_sample(tmp, 3)
    g, aligned = _genotype(tmp, ref_fa, pfx, single)
    sel, out, names, _ = oracle_dump(tmp, ref_fa, g, aligned)
    ref_names, seqs, masks, _ = t1k_amd.load_reference_fasta(sel)
    assert ref_names == names
    r1 = [s for _, _, s in t1k_amd.read_fastx(aligned[1])]
    r2 = None if single else [s for _, _, s in t1k_amd.read_fastx(aligned[3])]
    ptr, asg, ops = parse_dump(out + "_fragdump.tsv", len(r1))
    assert len(asg) > 1000 and (np.diff(ptr.astype(np.int64)) > 1).any()
    lens = [len(s) for s in seqs]
    off = pileup_ref.offsets(lens).astype(np.int64)
    # about 40 sites of the file: both ends of every selected allele and, evenly spaced, groups of three positions 7 and 60 bases apart
    # (one read-end spans a group), a name that is not selected, one that does not exist, comments, a blank line and a duplicate
    other = next(n for n, _, _ in util.read_fa(ref_fa) if n not in names)
    groups = max(1, round(40 / len(seqs) / 3))
    file_sites = {(a, p) for a, s in enumerate(seqs) for p in (0, len(s) - 1)}
    file_sites |= {(a, (len(s) - 61) * (k + 1) // (groups + 1) + d) for a, s in enumerate(seqs) for k in range(groups) for d in (0, 7, 60)}
    lines = ["# allele\tpos", ""] + ["%s\t%d" % (names[a], p + 1) for a, p in sorted(file_sites, key=lambda x: (x[1], x[0]))]
    lines[5:5] = ["%s\t3" % other, "#" + names[0] + "\t1", "NOT*AN:ALLELE\t100000"]
    lines.append(lines[3])
    sites_file = os.path.join(tmp, "sites.tsv")
    open(sites_file, "w").write("\n".join(lines) + "\n")
    assert 30 <= len(file_sites) <= 70
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--phase", "--pileup", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"}, barcode=False)
    line = [l for l in r.stderr.split("\n") if l.startswith("phase: ")]
    assert len(line) == 1 and all(w in line[0] for w in (" sites", " records", " bookings", " keys emitted", " folds", " ms")), r.stderr[-2000:]
    print(line[0])
    assert [l for l in r.stderr.split("\n") if l.startswith("--sites: ") and " 2 lines name an allele that is not selected" in l], r.stderr[-2000:]
    var_of = _var_of(a + "_allele.vcf", {n: i for i, n in enumerate(names)})
    assert len(var_of) >= 1
    sites = sorted(file_sites | set(var_of))
    sa, sp = np.array([s[0] for s in sites], np.uint32), np.array([s[1] for s in sites], np.uint32)
    aln, text, book_rec, book_uniq = ref.analyzer_records(ptr, asg, r1, r2)
    cells, st = ref.restate(off, aln, book_rec, book_uniq, text, ops, sa, sp)
    print(vars(st))
    assert any(c[1] > 0 for c in cells.values()) and any(c[1] < c[0] for c in cells.values())
    want = ref.table_text(names, seqs, masks, sa, sp, var_of, cells).split("\n")
    got = open(a + "_allele_phase.tsv").read().split("\n")
    assert len(got) == len(want) > 20                       # (the floor only keeps the comparison from being empty)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    # the variant pass in several pieces, and with every alignment through the device: the same bytes
    for tag, env in (("piece", {"T1K_ANALYZER_PIECE": "600"}), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"})):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--phase", "--sites", sites_file], env=env, barcode=False)
        assert _read(o + "_allele_phase.tsv") == _read(a + "_allele_phase.tsv"), tag
    # against --pileup: a booking adds at most 1 to a site pair, and one of its records is in the depth of either site; single-end, a
    # booking is one record, so what it shows at s in state x is in the pileup's counter x there
    _, rows = ref.parse(a + "_allele_phase.tsv")
    pile = {(p[0], p[1]): p[4] for p in pileup_ref.parse(a + "_allele_pileup.tsv")[1]}
    col = dict(zip(ref.STATES, ("A", "C", "G", "T", "N", "del")))
    total, first = {}, {}
    for row in rows:
        total[row[:3]] = total.get(row[:3], 0) + row[11]
        first[(row[0], row[1], row[2], row[9])] = first.get((row[0], row[1], row[2], row[9]), 0) + row[11]
    for (name, p, q), n in total.items():
        assert n <= min(sum(pile[(name, x)][k] for k in col.values()) for x in (p, q)), (name, p, q)
    if single:
        for (name, p, q, x), n in first.items():
            assert n <= pile[(name, p)][col[x]], (name, p, q, x)


# ---- 5. ground truth: two unknown bases that are always carried together -------------------------------------------------------------
def test_bases_carried_together_are_seen_together(built, tmp_path):
    tmp = str(tmp_path)
    ref_fa, pfx = util.several_snps_sample(tmp, 6, genes=3, pairs=2500, sub=0)
    # the precondition: inside every gene all alleles of the database agree at both positions, so the carriers of a gene all show the
    # same two unknown bases there, and everything else shows the database's
    swap = {"A": "C", "C": "G", "G": "T", "T": "A"}
    by_gene = {}
    for name, _, sq in util.read_fa(ref_fa):
        by_gene.setdefault(name.split("*")[0], set()).add((sq[150], sq[152]))
    assert all(len(v) == 1 and set(next(iter(v))) <= set(swap) for v in by_gene.values()), by_gene
    g, aligned = _genotype(tmp, ref_fa, pfx)
    a = os.path.join(tmp, "a")
    _analyze(ref_fa, g, aligned, a, ["--phase"], barcode=False)
    called = {}
    for name, pos, ref_base, var in _vcf(a + "_allele.vcf"):
        called.setdefault(name, {})[pos] = (ref_base, var)
    both = [n for n, v in called.items() if 150 in v and 152 in v]
    assert both, called
    _, rows = ref.parse(a + "_allele_phase.tsv")
    for name in both:
        (ref1, var1), (ref2, var2) = called[name][150], called[name][152]
        assert (ref1, ref2) in by_gene[name.split("*")[0]] and (var1, var2) == (swap[ref1], swap[ref2])
        seen = {(r[9], r[10]): r[11] for r in rows if r[:3] == (name, 151, 153)}
        assert all(r[7] == var1 and r[8] == var2 for r in rows if r[:3] == (name, 151, 153))
        assert seen.get((var1, var2), 0) > 0, (name, seen)
        assert (var1, ref2) not in seen and (ref1, var2) not in seen, (name, seen)


# ---- 7. nothing else changes ---------------------------------------------------------------------------------------------------------
class Runs:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["homo", "het"])
def snp(request, built, tmp_path_factory):
    """the novel-SNP sample through this build's genotyper, then the analyzer six ways"""
    tmp = str(tmp_path_factory.mktemp("phase_snp"))
    s = Runs()
    s.tmp, s.het = tmp, request.param
    s.ref, pfx = util.novel_snp_sample(tmp, s.het)
    s.g, s.aligned = _genotype(tmp, s.ref, pfx)
    s.plain, s.phase, s.bp, s.both, s.phase0, s.nobc = (os.path.join(tmp, x) for x in ("plain", "phase", "bp", "both", "phase0", "nobc"))
    _analyze(s.ref, s.g, s.aligned, s.plain)
    _analyze(s.ref, s.g, s.aligned, s.phase, ["--phase"])
    _analyze(s.ref, s.g, s.aligned, s.bp, ["--barcodePileup"])
    _analyze(s.ref, s.g, s.aligned, s.both, ["--barcodePileup", "--phase"])
    _analyze(s.ref, s.g, s.aligned, s.phase0, ["--varMaxGroup", "0", "--phase"])
    _analyze(s.ref, s.g, s.aligned, s.nobc, ["--phase"], barcode=False)
    s.gold = os.path.join(util.GOLDEN, "analyzer_variants", "het" if s.het else "homo")
    return s


def test_nothing_else_changes(snp):
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(snp.phase + tail) == _read(snp.both + tail) == _read(snp.gold + tail) == _read(snp.plain + tail), tail
    assert _read(snp.nobc + "_allele.vcf") == _read(snp.plain + "_allele.vcf")
    # both flags together share the retained pieces: each file as with its flag alone
    assert _read(snp.both + "_barcode_pileup.tsv") == _read(snp.bp + "_barcode_pileup.tsv")
    assert _read(snp.both + "_allele_phase.tsv") == _read(snp.phase + "_allele_phase.tsv") == _read(snp.nobc + "_allele_phase.tsv")
    assert not os.path.exists(snp.plain + "_allele_phase.tsv") and not os.path.exists(snp.bp + "_allele_phase.tsv")
    assert sorted(os.path.basename(p) for p in glob.glob(snp.phase + "_*")) == ["phase_allele.vcf", "phase_allele_phase.tsv", "phase_barcode_expr.tsv"]
    assert sorted(os.path.basename(p) for p in glob.glob(snp.nobc + "_*")) == ["nobc_allele.vcf", "nobc_allele_phase.tsv"]
    # one called site makes no pair; no variant calling and no --sites: no site.  The header alone
    assert len(_vcf(snp.phase + "_allele.vcf")) >= 1
    assert _read(snp.phase0 + "_allele_phase.tsv").decode() == ref.HEADER + "\n" and _read(snp.phase0 + "_allele.vcf") == b""


def test_sites_without_variant_calling(snp):
    """--varMaxGroup 0 --phase --sites: the alignments are made although nothing is called -- the same counts, the var columns empty"""
    name, pos, _, _ = _vcf(snp.phase + "_allele.vcf")[0]
    f = os.path.join(snp.tmp, "two_sites.tsv")
    open(f, "w").write("%s\t%d\n%s\t%d\n" % (name, pos + 1, name, pos - 29))
    o, o0 = os.path.join(snp.tmp, "sites"), os.path.join(snp.tmp, "sites0")
    _analyze(snp.ref, snp.g, snp.aligned, o, ["--phase", "--sites", f], barcode=False)
    _analyze(snp.ref, snp.g, snp.aligned, o0, ["--varMaxGroup", "0", "--phase", "--sites", f], barcode=False)
    _, rows = ref.parse(o + "_allele_phase.tsv")
    _, rows0 = ref.parse(o0 + "_allele_phase.tsv")
    rows, rows0 = ([r for r in x if r[:3] == (name, pos - 29, pos + 1)] for x in (rows, rows0))
    assert _read(o0 + "_allele.vcf") == b"" and len(rows) >= 1 and sum(r[11] for r in rows) > 10
    assert all(r[7] == "." and r[8] != "." for r in rows)
    assert [r[:7] + r[9:] for r in rows0] == [r[:7] + r[9:] for r in rows] and all(r[7] == "." and r[8] == "." for r in rows0)


# ---- 8. the golden chain -------------------------------------------------------------------------------------------------------------
def test_golden_chain(built, tmp_path):
    tmp = str(tmp_path)
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    _run([GENO] + c.args() + ["-o", g])
    aligned = ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"]
    selected = [l.split()[0] for l in open(g + "_allele.tsv") if l.strip()]
    seq = {name: s for name, _, s in util.read_fa(c.ref)}
    assert len(selected) >= 4
    sites_file = os.path.join(tmp, "sites.tsv")
    file_sites = [(a, p) for a in selected for p in range(50, len(seq[a]) + 1, 50)]          # every 50th position, 1-based
    open(sites_file, "w").write("".join("%s\t%d\n" % s for s in file_sites))
    flag = os.path.join(tmp, "flag")
    r = _analyze(c.ref, g, aligned, flag, c.flags + ["--pileup", "--barcodePileup", "--phase", "--sites", sites_file], env={"T1K_DEBUG_PHASES": "1"})
    print("\n".join(l for l in r.stderr.split("\n") if l.startswith("phase: ")))
    header, rows = ref.parse(flag + "_allele_phase.tsv")
    assert header == ref.HEADER and len(rows) > 100 and len({r[0] for r in rows}) >= 2
    sites = set(file_sites) | {(v[0], v[1] + 1) for v in _vcf(flag + "_allele.vcf")}
    assert all((r[0], r[1]) in sites and (r[0], r[2]) in sites and r[1] < r[2] and 0 <= r[12] <= r[11] > 0 for r in rows)
    # line order: the alleles in the order of _allele_pileup.tsv, then pos1, pos2, obs1, obs2 in state order
    al_rank = {}
    for row in pileup_ref.parse(flag + "_allele_pileup.tsv")[1]:
        al_rank.setdefault(row[0], len(al_rank))
    order = [(al_rank[r[0]], r[1], r[2], ref.STATES.index(r[9]), ref.STATES.index(r[10])) for r in rows]
    assert order == sorted(order) and len(set(order)) == len(order)
    # ref columns as in _allele_pileup.tsv
    line = {(p[0], p[1]): p for p in pileup_ref.parse(flag + "_allele_pileup.tsv")[1]}
    assert all((r[3], r[5]) == line[(r[0], r[1])][2:4] and (r[4], r[6]) == line[(r[0], r[2])][2:4] for r in rows)
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
