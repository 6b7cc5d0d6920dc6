"""GPU tests of the diplotype table (t1k_diplo_batch, genotyper --diplotypes).  Every comparison is exact: the kernel's matrix
against the restatement tests/diplo_ref.py on the designed tables (diplo_cases: the wavefront and tile edges, segments that end at lane 63,
begin at lane 64 or cross a tile, a gene of one candidate, a gene nobody holds), under contention with sums beyond 2^54, for every piece
size, for an empty input; the refusals, none of which may touch the output; the diagonal against t1k_alt_batch; and the executable's file
against the restatement fed with the job's own read groups and the calls read from its files."""
import glob
import os
import subprocess

import numpy as np
import pytest

import alt_cases
import diplo_cases as cases
import diplo_ref as ref
import goldens
import util
import t1k_amd
import test_distributed_gloo as tdg

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
CODES = {"OK": 0, "ARG": -1, "CAPACITY": -3}


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def table():
    return cases.designed()


@pytest.fixture(scope="module")
def want(table):
    w = np.array(ref.matrix(*table.args()), dtype=np.uint64)
    w.setflags(write=False)
    return w


def run(ctx, c):
    got, ms = ctx.diplo_batch(*c.args())
    n = np.diff(c.cand_ptr.astype(np.int64))
    assert got.dtype == np.uint64 and got.shape == (int((n * n).sum()),) and ms >= 0
    return got


# ---- the kernel = the restatement ----------------------------------------------------------------------------------------------------
def test_designed_table(ctx, table, want):
    """groups of 1, 2, 63, 64, 65, 128, 129 and 257 ids over five genes; a segment that ends at lane 63 and one that begins at lane 64;
    segments across the 64-boundaries of a long group; all 70 candidates of a gene; a gene with one candidate; a gene that no group holds and
    one without candidates (test_diplo_cpu.test_designed_table_holds_the_cases checks that the table holds all of this)"""
    got = run(ctx, table)
    assert np.array_equal(got, want)
    cp = table.cand_ptr.tolist()
    assert int(got.max()) > 1 << 40 and not got[70 * 70 + 1:70 * 70 + 1 + 30 * 30].any() and int(got[70 * 70]) > 0 and cp[3] == cp[4]


def test_adjacent_segments(ctx):
    c = cases.adjacent_case()
    got = run(ctx, c)
    assert got.tolist() == ref.matrix(*c.args()) and got[:25].any() and got[25:].any()


@pytest.mark.parametrize("seed", range(4))
def test_random_tables(ctx, seed):
    c = cases.random_case(seed, n_genes=2 + seed, per=5 + 30 * seed, n_groups=50 + 40 * seed, max_size=8 + 40 * seed)
    assert run(ctx, c).tolist() == ref.matrix(*c.args())


def test_contention_and_wide_sums(ctx):
    """20 000 groups that hold one pair, q near 2^40: every add lands on the same three cells and the sums pass 2^54"""
    c = cases.hot_cell_case()
    total = sum(int(x) for x in c.q)
    assert total > 1 << 54
    assert run(ctx, c).tolist() == [0, 0, 0, 0, total, total, 0, 0, total]


@pytest.mark.parametrize("piece", [1, 64, 1000])
def test_piece_sizes_give_identical_matrices(ctx, table, want, monkeypatch, piece):
    """the library reads T1K_DIPLO_PIECE in every call.  1: a piece per group, every group longer than its piece; 64: groups longer than a
    piece beside pieces of several groups; 1000: several pieces of many groups"""
    monkeypatch.setenv("T1K_DIPLO_PIECE", str(piece))
    pieces = t1k_amd.diplo_pieces(table.group_ptr)
    sizes = np.diff(table.group_ptr.astype(np.int64))
    assert pieces >= 3 and (piece == 1000 or (sizes > piece).any())
    assert pieces == (len(sizes) if piece == 1 else pieces) and (piece == 1 or pieces < len(sizes))
    assert np.array_equal(run(ctx, table), want)


def test_no_groups(ctx):
    got, ms = ctx.diplo_batch(np.array([0], dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64), np.array([0, 2, 2, 5], dtype=np.uint32))
    assert got.shape == (13,) and not got.any()


@pytest.mark.parametrize("name", list(cases.refusals()))
def test_refusals_leave_the_output_untouched(ctx, name):
    code, (gp, ent, q, cp) = cases.refusals()[name]
    rc, got, _ = ctx.diplo_batch(gp, ent, q, cp, raw=True)
    assert rc == CODES[code], name
    if code == "OK":
        assert got.tolist() == ref.matrix(gp, ent, q, cp)
    else:
        assert len(got) and (got.view(np.uint8) == t1k_amd.DIPLO_FILL).all(), name


def test_diagonal_equals_the_totals_of_alt_batch(ctx, table, want):
    """the same groups read as alleles of t1k_alt_batch (nobody called): total[a] is cell (a, a)"""
    cp = table.cand_ptr.astype(np.int64)
    n = np.diff(cp)
    gene = np.repeat(np.arange(len(n)), n).astype(np.uint32)
    tabs, _ = ctx.alt_batch(table.group_ptr, table.ent, table.q, gene, len(n), np.full(len(gene), alt_cases.EMPTY, dtype=np.uint32))
    base = np.concatenate([[0], np.cumsum(n * n)])
    diag = np.array([int(base[x]) + (i - int(cp[x])) * (int(n[x]) + 1) for x in range(len(n)) for i in range(int(cp[x]), int(cp[x + 1]))])
    got = run(ctx, table)
    assert np.array_equal(got[diag], tabs[0]) and np.array_equal(got, want) and int(tabs[0].sum()) > 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _files(prefix):
    return {os.path.basename(p)[len(os.path.basename(prefix)):]: open(p, "rb").read() for p in glob.glob(prefix + "_*")}


def _major_of(name, majors, delim):
    hit = [m for m in majors if name == m or name.startswith(m + delim)]
    return max(hit, key=len) if hit else None


@pytest.mark.parametrize("name", ["hla_synth_2x150", "cyp_rna_2x100"])
def test_genotyper_writes_the_table(built, tmp_path, name):
    c = goldens.Case(name, str(tmp_path / "in"))
    out = {k: str(tmp_path / k) for k in ("plain", "diplo", "both")}
    extra = {"plain": [], "diplo": ["--diplotypes", "3"], "both": ["--alternatives", "3", "--diplotypes", "3"]}
    for k in out:
        r = subprocess.run([GENO] + c.args() + ["-o", out[k], "--outputReadAssignment"] + extra[k], stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b, both = (_files(out[k]) for k in ("plain", "diplo", "both"))
    assert "_diplotypes.tsv" not in a and set(b) == set(a) | {"_diplotypes.tsv"} and {"_genotype.tsv", "_allele.tsv", "_assign.tsv"} <= set(a)
    for k in a:
        assert a[k] == b[k], k                                   # every other output: byte for byte
    assert set(both) == set(b) | {"_alternatives.tsv"}
    for k in b:
        assert b[k] == both[k], k                                # --alternatives added: the same table, the same everything else
    text = b["_diplotypes.tsv"].decode()
    # the job's read groups, by the route the parity tests use
    cyp = "cyp" in name
    kw = dict(ref_seq_similarity=float(c.flags[c.flags.index("-s") + 1]) if "-s" in c.flags else 0.8, relax_intron_align=1 if "--relaxIntronAlign" in c.flags else 0)
    if cyp:
        kw.update(allele_digit_units=1, allele_delimiter=".")
    job = t1k_amd.Job(c.ref, diplotypes=1000, diplo_candidates=2, **kw)   # two candidates per gene: the called classes are forced in
    job.load_reads(c.r1, c.r2, c.bc)
    job.run()
    G, _, ptr, _, ent = tdg.parse_table(job.groups_serialize())
    gene, _ = job.allele_table()
    assert job.genotype_text().encode() == b["_genotype.tsv"]
    narrow = job.diplotypes_text()
    job.close()
    names = t1k_amd.load_reference_fasta(c.ref)[0]
    assert len(names) == len(gene)
    geno = [l.split("\t") for l in b["_genotype.tsv"].decode().splitlines()]
    gene_names = [f[0] for f in geno]
    # the calls: field k of the gene's line names the major alleles of slot k; the allele that stands for the slot is the one _allele.tsv lists
    listed = [l.split(" ")[0] for l in b["_allele.tsv"].decode().splitlines()]
    index = {n: i for i, n in enumerate(names)}
    called = [-1] * (2 * len(geno))
    for g, f in enumerate(geno):
        for k in (0, 1):
            field = f[2 + 3 * k]
            if field == ".":
                continue
            majors = field.split(",")
            mine = [n for n in listed if gene[index[n]] == g and _major_of(n, majors, "." if cyp else ":") is not None and index[n] not in called]
            assert mine, (f[0], k, "a call of quality 0 has no line in _allele.tsv: pick another case")
            called[2 * g + k] = index[mine[0]]
    assert max(called) >= 0
    q = np.array([ref.q_of(ent["w"][int(ptr[g]):int(ptr[g + 1])].max()) for g in range(G)], dtype=np.uint64)
    alleles = ent["allele"].astype(np.uint32)
    p = ref.plan(ptr, alleles, q, gene, called, 512)
    assert text == ref.text(p, ref.matrix(p.group_ptr, p.ent, p.q, p.cand_ptr), 3, gene_names, names)
    p2 = ref.plan(ptr, alleles, q, gene, called, 2)
    assert narrow == ref.text(p2, ref.matrix(p2.group_ptr, p2.ent, p2.q, p2.cand_ptr), 1000, gene_names, names)
    assert max(p.n_class) > 2 and max(np.diff(p2.cand_ptr)) == 2
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert rows and all(len(r) == 14 for r in rows) and {r[0] for r in rows if r[11] == "1"} == {geno[g][0] for g in range(len(geno)) if called[2 * g] >= 0}
    # explained of the called line from the read-assignment file: the fragments' allele sets are the groups; a group weighs what the job's table says
    frags = {}
    for line in b["_assign.tsv"].decode().splitlines():
        f = line.split("\t")
        frags.setdefault(f[0], set()).add(index[f[1]])
    sets = set(frozenset(s) for s in frags.values())
    weight = {frozenset(alleles[int(ptr[g]):int(ptr[g + 1])].tolist()): int(q[g]) for g in range(G)}
    assert sets == set(weight) and len(weight) == G
    for r in rows:
        if r[11] == "1":
            g = gene_names.index(r[0])
            mine = set(s for s in called[2 * g:2 * g + 2] if s >= 0)
            assert r[4] == ref.fmt(sum(w for s, w in weight.items() if s & mine)), r
            assert {index[r[2]], index[r[3]]} <= mine, r          # a class that holds a called allele is named by it


def test_two_ranks_write_the_same_table(built, tmp_path):
    """--gpus N: the rank that writes _genotype.tsv computes the table from the merged groups; here two ranks on one device"""
    c = goldens.Case("hla_synth_2x150", str(tmp_path / "in"))
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    for out, env in ((one, {}), (two, {"T1K_GPUS": "0,0"})):
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--diplotypes", "7"], stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = _files(one), _files(two)
    assert set(a) == set(b) and "_diplotypes.tsv" in a
    for k in a:
        assert a[k] == b[k], k
    assert len(a["_diplotypes.tsv"].decode().splitlines()) > 1
