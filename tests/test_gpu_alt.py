"""GPU tests of the alternatives table (t1k_alt_batch, genotyper --alternatives).  Every comparison is exact: the kernel's four
tables against the restatement tests/alt_ref.py on the designed table (alt_cases.designed: the wavefront and loop edges, every pattern of
called alleles, groups that run through several genes), at the bitset's word edges, under contention with sums beyond 2^54, for every
piece size, for an empty input; the refusals, none of which may touch the output; and the executable's file against the restatement fed
with the job's own read groups and the calls read from its files."""
import glob
import os
import subprocess

import numpy as np
import pytest

import alt_cases as cases
import alt_ref as ref
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
    w = np.array(ref.tables(*table.args()), dtype=np.uint64)
    w.setflags(write=False)
    return w


def run(ctx, c):
    got, ms = ctx.alt_batch(c.group_ptr, c.alleles, c.q, c.allele_gene, c.n_genes, c.slot_of)
    assert got.dtype == np.uint64 and got.shape == (4, len(c.allele_gene)) and ms >= 0
    return got


# ---- the kernel = the restatement ----------------------------------------------------------------------------------------------------
def test_designed_table(ctx, table, want):
    """groups of 1, 2, 63, 64, 65, 128, 129 and 257 entries; no called allele, only slot 0, only slot 1, both; a gene whose slot 1 is empty
    and a gene without a call; groups over two and three genes with different patterns; the called allele as the first and as the last
    entry of a 65-entry group (test_alt_cpu.test_designed_table_holds_the_cases checks that the table holds all of this)"""
    got = run(ctx, table)
    assert np.array_equal(got, want)
    assert int(got[0].max()) > 1 << 40 and int(got[3].sum()) > 0 and int(got[1].sum()) > 0 and int(got[2].sum()) > 0


@pytest.mark.parametrize("n_genes", [31, 32, 33, 150])
def test_bitset_word_edges(ctx, n_genes):
    """2 * nGenes = 62, 64, 66 and 300 (the number is even, so 65 slots cannot be had: 66 is the first size past the word, and its slots
    64 and 65 are called); the calls sit in the last two genes, i.e. in the last bits of the set"""
    c = cases.word_edge_case(n_genes)
    assert np.array_equal(run(ctx, c), np.array(ref.tables(*c.args()), dtype=np.uint64))


def test_contention_and_wide_sums(ctx):
    """20 000 one-entry groups on one allele, q near 2^40: every add lands on the same four cells and the sum passes 2^54"""
    n = 20000
    q = (1 << 40) - np.arange(n, dtype=np.uint64) * np.uint64(3)
    gp = np.arange(n + 1, dtype=np.uint64)
    al = np.full(n, 1, dtype=np.uint32)
    gene = np.zeros(3, dtype=np.uint32)
    slot = np.array([cases.EMPTY, 1, cases.EMPTY], dtype=np.uint32)
    got, _ = ctx.alt_batch(gp, al, q, gene, 1, slot)
    total = sum(int(x) for x in q)
    assert total > 1 << 54
    assert got.tolist() == [[0, total, 0], [0, 0, 0], [0, total, 0], [0, 0, 0]]
    slot = np.array([cases.EMPTY] * 3, dtype=np.uint32)      # ... and with no call at all everything is unexplained
    got, _ = ctx.alt_batch(gp, al, q, gene, 1, slot)
    assert got.tolist() == [[0, total, 0], [0, 0, 0], [0, 0, 0], [0, total, 0]]


@pytest.mark.parametrize("piece", [1, 64, 1000])
def test_piece_sizes_give_identical_tables(ctx, table, want, monkeypatch, piece):
    """the library reads T1K_ALT_PIECE in every call.  1: a piece per group, every group longer than its piece; 64: groups longer than a
    piece beside pieces of several groups; 1000: several pieces of many groups"""
    monkeypatch.setenv("T1K_ALT_PIECE", str(piece))
    pieces = t1k_amd.alt_pieces(table.group_ptr)
    sizes = np.diff(table.group_ptr.astype(np.int64))
    assert pieces >= 3 and (piece == 1000 or (sizes > piece).any())
    assert pieces == (len(sizes) if piece == 1 else pieces) and (piece == 1 or pieces < len(sizes))
    assert np.array_equal(run(ctx, table), want)


def test_no_groups(ctx):
    got, ms = ctx.alt_batch(np.array([0], dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64), np.array([0, 0, 1], dtype=np.uint32), 2,
                            np.array([0, cases.EMPTY, 3], dtype=np.uint32))
    assert got.shape == (4, 3) and not got.any()


@pytest.mark.parametrize("name", list(cases.refusals()))
def test_refusals_leave_the_output_untouched(ctx, name):
    code, (gp, al, q, gene, n_genes, slot) = cases.refusals()[name]
    rc, got, _ = ctx.alt_batch(gp, al, q, gene, n_genes, slot, raw=True)
    assert rc == CODES[code], name
    if code == "OK":
        assert got.tolist() == ref.tables(gp, al, q, gene, slot)
    else:
        assert (got.view(np.uint8) == t1k_amd.ALT_FILL).all(), name


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _files(prefix):
    return {os.path.basename(p)[len(os.path.basename(prefix)):]: open(p, "rb").read() for p in glob.glob(prefix + "_*")}


def _major_of(name, majors, delim):
    hit = [m for m in majors if name == m or name.startswith(m + delim)]
    return max(hit, key=len) if hit else None


@pytest.mark.parametrize("name", ["hla_synth_2x150", "cyp_rna_2x100"])
def test_genotyper_writes_the_table(built, tmp_path, name):
    c = goldens.Case(name, str(tmp_path / "in"))
    plain, flagged = str(tmp_path / "plain"), str(tmp_path / "alt")
    for out, extra in ((plain, []), (flagged, ["--alternatives", "3"])):
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--outputReadAssignment"] + extra, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = _files(plain), _files(flagged)
    assert "_alternatives.tsv" not in a and set(b) == set(a) | {"_alternatives.tsv"} and {"_genotype.tsv", "_allele.tsv", "_assign.tsv"} <= set(a)
    for k in a:
        assert a[k] == b[k], k                                   # every other output: byte for byte
    text = b["_alternatives.tsv"].decode()
    # the job's read groups, by the route the parity tests use, and the abundances behind alt_abundance
    cyp = "cyp" in name
    kw = dict(ref_seq_similarity=float(c.flags[c.flags.index("-s") + 1]) if "-s" in c.flags else 0.8, relax_intron_align=1 if "--relaxIntronAlign" in c.flags else 0)
    if cyp:
        kw.update(allele_digit_units=1, allele_delimiter=".")
    job = t1k_amd.Job(c.ref, alternatives=3, **kw)
    job.load_reads(c.r1, c.r2, c.bc)
    job.run()
    G, _, ptr, _, ent = tdg.parse_table(job.groups_serialize())
    gene, abundance = job.allele_table()
    assert job.genotype_text().encode() == b["_genotype.tsv"] and job.alternatives_text() == text
    job.close()
    names = t1k_amd.load_reference_fasta(c.ref)[0]
    assert len(names) == len(gene)
    geno = [l.split("\t") for l in b["_genotype.tsv"].decode().splitlines()]
    gene_names = [f[0] for f in geno]
    assert all(gene_names[gene[a]] == names[a].split("*")[0] for a in range(len(names)))
    # the calls: field k of the gene's line names the major alleles of slot k; the allele that stands for the slot is the one _allele.tsv lists
    listed = [l.split(" ")[0] for l in b["_allele.tsv"].decode().splitlines()]
    index = {n: i for i, n in enumerate(names)}
    slot_of = np.full(len(names), cases.EMPTY, dtype=np.uint32)
    n_called = 0
    for g, f in enumerate(geno):
        for k in (0, 1):
            field = f[2 + 3 * k]
            if field == ".":
                continue
            majors = field.split(",")
            mine = [n for n in listed if gene[index[n]] == g and _major_of(n, majors, "." if cyp else ":") is not None and slot_of[index[n]] == cases.EMPTY]
            assert mine, (f[0], k, "a call of quality 0 has no line in _allele.tsv: pick another case")
            slot_of[index[mine[0]]] = 2 * g + k
            n_called += 1
    assert n_called >= 1
    q = np.array([ref.q_of(ent["w"][int(ptr[g]):int(ptr[g + 1])].max()) for g in range(G)], dtype=np.uint64)
    alleles = ent["allele"].astype(np.uint32)
    tabs = ref.tables(ptr, alleles, q, gene, slot_of)
    assert text == ref.text(tabs, gene, slot_of, 3, gene_names, names, abundance)
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert len(rows) >= n_called and max(int(r[3]) for r in rows) <= 3 and {(r[0], r[2]) for r in rows} == {(geno[s >> 1][0], str(s & 1)) for s in slot_of.tolist() if s != cases.EMPTY}
    # total_called from the read-assignment file: the fragments' allele sets are the groups; a group weighs what the job's table says
    frags = {}
    for line in b["_assign.tsv"].decode().splitlines():
        f = line.split("\t")
        frags.setdefault(f[0], set()).add(index[f[1]])
    sets = {}
    for s in frags.values():
        sets[frozenset(s)] = sets.get(frozenset(s), 0) + 1
    weight = {frozenset(alleles[int(ptr[g]):int(ptr[g + 1])].tolist()): int(q[g]) for g in range(G)}
    assert set(sets) == set(weight) and len(weight) == G
    for s, n in sets.items():
        assert n * 1048 <= weight[s] <= n << 20, (n, weight[s])      # a fragment weighs 0.001 .. 1
    for r in rows:
        called = index[r[1]]
        assert r[5] == ref.fmt(sum(w for s, w in weight.items() if called in s)), r


def test_two_ranks_write_the_same_table(built, tmp_path):
    """--gpus N: the rank that writes _genotype.tsv computes the table from the merged groups; here two ranks on one device"""
    c = goldens.Case("hla_synth_2x150", str(tmp_path / "in"))
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    for out, env in ((one, {}), (two, {"T1K_GPUS": "0,0"})):
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--alternatives", "7"], stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = _files(one), _files(two)
    assert set(a) == set(b) and "_alternatives.tsv" in a
    for k in a:
        assert a[k] == b[k], k
    assert max(int(l.split("\t")[3]) for l in a["_alternatives.tsv"].decode().splitlines()[1:]) == 7
