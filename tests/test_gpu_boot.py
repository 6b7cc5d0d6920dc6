"""GPU tests of genotyper --bootstrap (t1k_boot.hip, host/bootstrap.cpp).  Every comparison is exact: the resampling kernel's
k as integers and c' bit for bit against the restatement tests/boot_ref.py (through its vectorised form, which test_boot_cpu.py holds to it);
one update of all replicates against em_ref.em_update_ref on every replicate's own c', under every mask; the job's matrix, file and debug
switches against each other and against the restatement's statistics; and the whole lockstep run of a job cut down to a size the
pure-Python EM can follow, SQUAREM and masking included.

The update table has 106 classes, not 40: a row's classes are distinct (em_ref.Table), so its row of 65 entries needs 65 classes that the
40 ordinary ones (sizes 0, 1, U - 1, U, U + 1, 2 U + 1 and 2 .. 40, two of abundance 0) cannot supply; 66 more appear in the prescribed rows only."""
import glob
import os
import subprocess
import time

import numpy as np
import pytest

import boot_cases as cases
import boot_ref as ref
import em_ref
import goldens
import util
import t1k_amd
import test_distributed_gloo as tdg

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
FIXTURES = ["hla_synth_2x150", "cyp_rna_2x100"]
FILL = 7.25


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


# ---- the resampling kernel ---------------------------------------------------------------------------------------------------------------
def one_class_per_group(ctx, count):
    G = len(count)
    ctx.em_setup(np.arange(G + 1, dtype=np.uint64), np.zeros(G, np.uint32), count, np.array([1000], np.int32))


@pytest.mark.parametrize("n_rep", cases.REPLICATES)
@pytest.mark.parametrize("G", cases.GROUPS)
def test_resampling_is_the_restatement(ctx, G, n_rep):
    """counts of n_g 1, 2, 3 (a lane draws alone), 63, 64, 65 and 1000 (around the size from which the lanes share the draws), fractional
    ones and halves (n_g by llrint); B + 1 around one and two blocks of lanes"""
    count, k, c = cases.resampled(G, n_rep)
    share = t1k_amd.boot_limits()[1]
    ns = [ref.n_of(v) for v in count.tolist()]
    assert G < 12 or (min(ns) < share - 1 and share - 1 in ns and share in ns and share + 1 in ns and max(ns) > 2 * share)
    one_class_per_group(ctx, count)
    ctx.boot_begin(n_rep - 1, cases.SEED)
    gk, gc = ctx.boot_counts()
    ne = ctx.boot_nonempty()
    ctx.boot_end()
    assert gk.shape == (n_rep, G) and np.array_equal(gk.astype(np.int64), k)
    assert em_ref.same_bits(gc, c), em_ref.first_difference(gc, c)
    assert np.array_equal(gk[0], ns) and em_ref.same_bits(gc[0], count)                       # replicate 0 is the data
    assert ne.tolist() == [ref.non_empty(row) for row in c]
    if G == 300:
        assert len({tuple(r) for r in gk.tolist()}) == n_rep                                  # no two replicates alike


@pytest.mark.parametrize("n_rep", [2, 129])
def test_identity_mode_hands_back_the_counts(ctx, n_rep):
    count, k, c = cases.resampled(300, n_rep, True)
    one_class_per_group(ctx, count)
    ctx.boot_begin(n_rep - 1, cases.SEED, identity=True)
    gk, gc = ctx.boot_counts()
    ctx.boot_end()
    assert np.array_equal(gk.astype(np.int64), k) and all(em_ref.same_bits(row, count) for row in gc) and em_ref.same_bits(gc, c)


def test_refusals(ctx):
    count = cases.counts_for(5)
    one_class_per_group(ctx, count)
    assert ctx.boot_begin(0, raw=True) != 0 and ctx.boot_begin(1001, raw=True) != 0
    one_class_per_group(ctx, np.array([1.0, float(1 << 28)]))
    assert ctx.boot_begin(3, raw=True) == -3 and "2^27" in ctx.last_error()
    fresh = t1k_amd.Context()
    assert fresh.boot_begin(3, raw=True) != 0 and "t1k_em_setup" in fresh.last_error()
    fresh.close()


# ---- one update of all replicates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", cases.REPLICATES)
def test_one_update_under_every_mask(ctx, n_rep):
    """n, x1 and diff of every active replicate: bit for bit em_update_ref on its c'; of every inactive one: the fill pattern"""
    U = t1k_amd.boot_limits()[0]
    t = cases.update_table(U)
    c, want = cases.update_want(U, n_rep)
    x = cases.update_x0(U, n_rep)
    ctx.em_setup(*t.args())
    ctx.boot_begin(n_rep - 1, cases.SEED)
    gk, gc = ctx.boot_counts()
    assert em_ref.same_bits(gc, c)
    masks = cases.masks(n_rep)
    assert ("block 0 inactive" in masks) == (n_rep > 64) and {"all", "only 0", "only the last"} <= set(masks) and (n_rep < 64 or "only 63" in masks) and (n_rep < 65 or "only 64" in masks)
    psum_zero = 0
    for name, active in masks.items():
        x1, n, diff = ctx.boot_update(active, x, fill=FILL)
        for r in range(n_rep):
            if active[r]:
                w = want[r]
                assert em_ref.same_bits(n[r], w[1]), (name, r, em_ref.first_difference(n[r], w[1]))
                assert em_ref.same_bits(x1[r], w[0]), (name, r, em_ref.first_difference(x1[r], w[0]))
                assert em_ref.same_bits(diff[r], w[2]), (name, r, diff[r], w[2])
                psum_zero += n[r][cases.ZERO_CLASSES[0]] == 0.0
            else:
                assert (n[r] == FILL).all() and (x1[r] == FILL).all() and diff[r] == FILL, (name, r)
    assert psum_zero > 0 and ctx.boot_times()["updates"] == len(masks)
    # the existing single EM on a replicate's counts gives the same doubles (what T1K_BOOTSTRAP_SERIAL=1 runs)
    r = n_rep - 1
    ctx.em_set_count(c[r])
    x1, n, diff = ctx.em_update(x[r])
    assert em_ref.same_bits(n, want[r][1]) and em_ref.same_bits(x1, want[r][0]) and em_ref.same_bits(diff, want[r][2])
    ctx.em_set_count(t.count)
    ctx.boot_end()


# ---- through the job ------------------------------------------------------------------------------------------------------------------------
def job_kw(c):
    kw = dict(ref_seq_similarity=float(c.flags[c.flags.index("-s") + 1]) if "-s" in c.flags else 0.8, relax_intron_align=1 if "--relaxIntronAlign" in c.flags else 0)
    if "cyp" in c.name:
        kw.update(allele_digit_units=1, allele_delimiter=".")
    return kw


class Run:
    """one job with a bootstrap: what the tests compare"""

    def __init__(self, c, B, seed=1, reads=None):
        job = t1k_amd.Job(c.ref, bootstrap=B, bootstrap_seed=seed, **job_kw(c))
        if reads is None:
            job.load_reads(c.r1, c.r2, c.bc)
        else:
            job.load_reads(*reads)
        job.run()
        self.matrix, self.rounds, self.valid = job.bootstrap_matrix()
        self.text = job.bootstrap_text()
        self.genotype = job.genotype_text()
        self.gene, self.abundance = job.allele_table()
        self.ec, self.weight, self.eff_len, self.series = job.em_alleles()
        self.series_names = job.series_names()
        self.groups = job.groups_serialize()
        self.em_rounds = job.counts()["em_iterations"]
        job.close()

    def restated_text(self):
        geno = [l.split("\t") for l in self.genotype.splitlines()]
        index = {n: i for i, n in enumerate(self.series_names)}
        called = [tuple([] if f[2 + 3 * k] == "." else [index[n] for n in f[2 + 3 * k].split(",")] for k in (0, 1)) for f in geno]
        rows = ref.table(self.matrix, self.valid, self.series, self.gene, called)
        return ref.text(rows, [f[0] for f in geno], self.series_names), called


_cache = {}


@pytest.fixture(scope="module")
def base(built, tmp_path_factory):
    def get(name):
        if name not in _cache:
            c = goldens.Case(name, str(tmp_path_factory.mktemp(name)))
            _cache[name] = (c, Run(c, 5))
        return _cache[name]
    return get


def _files(prefix):
    return {os.path.basename(p)[len(os.path.basename(prefix)):]: open(p, "rb").read() for p in glob.glob(prefix + "_*")}


@pytest.mark.parametrize("name", FIXTURES)
def test_the_flag_adds_one_file_and_changes_no_other(base, tmp_path, name):
    c, b = base(name)
    plain, flagged, all3 = str(tmp_path / "plain"), str(tmp_path / "boot"), str(tmp_path / "all")
    for out, extra in ((plain, []), (flagged, ["--bootstrap", "5"]), (all3, ["--bootstrap", "5", "--alternatives", "--diplotypes"])):
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--outputReadAssignment"] + extra, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    a, f, m = _files(plain), _files(flagged), _files(all3)
    assert "_bootstrap.tsv" not in a and set(f) == set(a) | {"_bootstrap.tsv"} and {"_genotype.tsv", "_allele.tsv", "_assign.tsv"} <= set(a)
    for k in a:
        assert a[k] == f[k] == m[k], k                                   # every other output: byte for byte
    assert f["_bootstrap.tsv"].decode() == b.text == m["_bootstrap.tsv"].decode() and set(m) == set(f) | {"_alternatives.tsv", "_diplotypes.tsv"}


@pytest.mark.parametrize("name", FIXTURES)
def test_matrix_and_table_of_the_job(base, name):
    c, b = base(name)
    assert b.matrix.shape == (6, len(b.gene)) and b.valid.all() and (b.rounds >= 2).all()
    assert em_ref.same_bits(b.matrix[0], b.abundance) and b.rounds[0] == b.em_rounds       # replicate 0 went through the new kernels
    text, called = b.restated_text()
    assert b.text == text
    assert any(s1 or s2 for s1, s2 in called) and len(text.splitlines()) > 1
    assert len({r.tobytes() for r in b.matrix}) == 6                                        # no two replicates alike


@pytest.mark.parametrize("name", FIXTURES)
def test_serial_path_gives_the_same_bits(base, monkeypatch, name):
    c, b = base(name)
    monkeypatch.setenv("T1K_BOOTSTRAP_SERIAL", "1")
    s = Run(c, 5)
    assert em_ref.same_bits(s.matrix, b.matrix) and np.array_equal(s.rounds, b.rounds) and np.array_equal(s.valid, b.valid) and s.text == b.text
    assert s.genotype == b.genotype and em_ref.same_bits(s.abundance, b.abundance)


@pytest.mark.parametrize("name", FIXTURES)
def test_identity_mode_repeats_the_data(base, monkeypatch, name):
    c, b = base(name)
    monkeypatch.setenv("T1K_BOOTSTRAP_IDENTITY", "1")
    s = Run(c, 65)
    assert s.matrix.shape[0] == 66 and all(em_ref.same_bits(row, b.matrix[0]) for row in s.matrix) and (s.rounds == b.rounds[0]).all() and s.valid.all()


@pytest.mark.parametrize("name", FIXTURES)
def test_a_replicate_depends_on_the_seed_and_its_index_only(base, name):
    c, b = base(name)
    few, many, other = Run(c, 3), Run(c, 70), Run(c, 3, seed=2)
    assert em_ref.same_bits(few.matrix, many.matrix[:4]) and em_ref.same_bits(few.matrix, b.matrix[:4]) and np.array_equal(few.rounds, many.rounds[:4])
    assert em_ref.same_bits(other.matrix[0], few.matrix[0]) and all(not em_ref.same_bits(other.matrix[r], few.matrix[r]) for r in (1, 2, 3))
    assert many.text == many.restated_text()[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_threads_and_ranks_write_the_same_file(base, tmp_path, name):
    c, b = base(name)
    outs = {}
    for tag, extra, env in (("t1", ["-t", "1"], {}), ("t4", ["-t", "4"], {}), ("two", [], {"T1K_GPUS": "0,0"})):
        out = str(tmp_path / tag)
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--bootstrap", "5"] + extra, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = _files(out)
    assert outs["t1"]["_bootstrap.tsv"].decode() == b.text
    for tag in ("t4", "two"):
        assert set(outs[tag]) == set(outs["t1"])
        for k in outs["t1"]:
            assert outs[tag][k] == outs["t1"][k], (tag, k)


def test_debug_line_and_serial_switch_of_the_executable(base, tmp_path):
    c, b = base("hla_synth_2x150")
    for tag, env in (("batched", {}), ("serial", {"T1K_BOOTSTRAP_SERIAL": "1"})):
        out = str(tmp_path / tag)
        r = subprocess.run([GENO] + c.args() + ["-o", out, "--bootstrap", "5"], stderr=subprocess.PIPE, text=True, env=dict(os.environ, T1K_DEBUG_PHASES="1", **env))
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stderr.splitlines() if l.startswith("[t1k job] bootstrap:")]
        assert len(line) == 1 and "5 replicates (5 valid)" in line[0] and " updates, kernel " in line[0] and " total " in line[0] and ("serial" in line[0]) == (tag == "serial"), r.stderr
        assert open(out + "_bootstrap.tsv").read() == b.text


# ---- the whole driver against the restatement -----------------------------------------------------------------------------------------------
def cut_reads(c, n, tmp):
    out = []
    for src in (c.r1, c.r2):
        dst = os.path.join(tmp, "cut_" + os.path.basename(src))
        with open(src) as f, open(dst, "w") as o:
            o.writelines(f.readlines()[:4 * n])
        out.append(dst)
    return out


def em_rows(groups, ec):
    """the rows of the E-step as quantify forms them from the read groups: the count is the largest weight of the row, the classes are
    the distinct classes of its alleles in first-appearance order"""
    G, _, ptr, _, ent = tdg.parse_table(groups)
    rows, count = [], []
    for g in range(G):
        e = ent[int(ptr[g]):int(ptr[g + 1])]
        count.append(float(e["w"].max()))
        seen = []
        for a in e["allele"].tolist():
            if ec[a] not in seen:
                seen.append(int(ec[a]))
        rows.append(seen)
    row_ptr = np.zeros(G + 1, np.uint64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    return (row_ptr, np.array([e for r in rows for e in r], np.uint32)), np.array(count, np.float64)


@pytest.mark.parametrize("name,fragments", [("cyp_rna_2x100", 300), ("hla_synth_2x150", 300)])
def test_lockstep_run_is_the_restatement(built, tmp_path, name, fragments):
    """the first 300 fragments of the fixture, B = 3: four pure-Python EMs of some tens of updates over at most a few hundred read groups
    and some 15 000 entries (a few tenths of a second; the time is printed); rounds, validity and every abundance bit for bit.  The cyp
    runs go past their 11th round, the first that is masked"""
    c = goldens.Case(name, str(tmp_path / "in"))
    b = Run(c, 3, seed=5, reads=cut_reads(c, fragments, str(tmp_path)))
    cl = ref.Classes(b.ec, b.eff_len, b.weight, b.series, b.gene)
    rows, count = em_rows(b.groups, b.ec)
    t0 = time.time()
    ab, rounds, valid = ref.bootstrap(rows, count, cl, 3, 5)
    print("%s: %d groups, %d entries, %d classes, rounds %s, restatement %.2f s" % (name, len(count), len(rows[1]), cl.E, rounds, time.time() - t0))
    assert len(count) >= 20 and cl.E >= 2 and ("cyp" not in name or min(rounds) > 11)
    assert rounds == b.rounds.tolist() and valid == b.valid.tolist()
    assert em_ref.same_bits(b.matrix, ab), em_ref.first_difference(b.matrix, ab)
    assert em_ref.same_bits(b.matrix[0], b.abundance) and b.text == b.restated_text()[0]


def test_empty_replicates_are_counted_out(built, tmp_path):
    """three fragments, B = 200: a replicate in which no group drew a read has nothing to estimate"""
    c = goldens.Case("hla_synth_2x150", str(tmp_path / "in"))
    b = Run(c, 200, reads=cut_reads(c, 3, str(tmp_path)))
    cl = ref.Classes(b.ec, b.eff_len, b.weight, b.series, b.gene)
    rows, count = em_rows(b.groups, b.ec)
    assert 1 <= len(count) <= 3
    ab, rounds, valid = ref.bootstrap(rows, count, cl, 200, 1)
    invalid = valid[1:].count(False)
    print("%d groups of counts %s: %d of 200 replicates invalid" % (len(count), count.tolist(), invalid))
    assert 1 <= invalid <= 100                                                  # the test's own precondition, under the restatement alone
    assert valid == b.valid.tolist() and rounds == b.rounds.tolist() and em_ref.same_bits(b.matrix, ab)
    lines = [l.split("\t") for l in b.text.splitlines()[1:]]
    assert lines and all(l[12] == str(200 - invalid) for l in lines) and b.text == b.restated_text()[0]
