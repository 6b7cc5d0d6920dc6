"""CPU tests of genotyper --bootstrap: the numbers of the resampling (thresholds, hash, draws, counts) in the restatement
tests/boot_ref.py, the host code of the product (the SQUAREM step functions with the masking rule, the called series, the statistics and the
text: t1k_amd/csrc/host/genotype.cpp built into tests/harness/boot_host_harness.cpp) against the restatement on tables written by hand, the
command line, the declarations and bindings, and the new kernels' resources as the compiler reports them."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import boot_cases as cases
import boot_ref as ref
import em_ref
import goldens
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
HOST = os.path.join(util.ROOT, "t1k_amd", "csrc", "host")
ISSUE_THRESHOLDS = """
5e2d58d8b3bcdf1a bc5ab1b16779be35 eb715e1dc1582dc2 fb23979734a252f1 ff1025f59174dc3d
ffd90f3ba4055e19 fffa8b71fc72c913 ffff540c0914b3c9 ffffed1f4aa8f120 fffffe216e641462
ffffffd4d85d3183 fffffffc6da262b4 ffffffffba12d178 fffffffffb07c64c ffffffffffab8ea5
fffffffffffabe22 ffffffffffffb11a fffffffffffffba1 ffffffffffffffc5 fffffffffffffffd
"""


# ---- the resampling ------------------------------------------------------------------------------------------------------------------
def test_thresholds_recomputed_with_decimals():
    want = [int(w, 16) for w in ISSUE_THRESHOLDS.split()]
    for digits in (80, 120, 200):
        got, t20 = ref.thresholds(digits)
        assert got == want and t20 == (1 << 64) - 1, digits
    assert len(want) == 20 and want == sorted(want) and ref.T == want
    src = open(os.path.join(CSRC, "t1k_boot.hip")).read()
    assert [int(w, 16) for w in re.findall(r"kBootT\d+ = 0x([0-9a-f]{16})ull", src)] == want        # the kernel's table, in order


def test_hash_check_values():
    assert ref.u(1, 1, 0, 0) == 0x2197de21cc1f2368 and ref.u(1, 2, 5, 7) == 0x7ff5d8a3f66b5aaa
    assert ref.mix(0) == 0xe220a8397b1dcdaf                                                          # (splitmix64's first output of state 0)


def test_draw_of_hand_picked_hashes():
    T = ref.T
    assert [ref.poisson(v) for v in (0, T[0] - 1, T[0], T[19], (1 << 64) - 1)] == [0, 0, 1, 20, 20]
    assert [ref.poisson(T[k]) for k in range(20)] == list(range(1, 21)) and [ref.poisson(T[k] - 1) for k in range(20)] == list(range(20))


def test_mean_of_the_draws():
    n = 200000
    k, _ = cases.resample_fast(np.array([float(n)]), 1, 1)
    mean = int(k[1, 0]) / n
    print("mean of %d draws: %.4f" % (n, mean))
    assert abs(mean - 1) < 0.02
    assert int(cases.resample_fast(np.array([2000.0]), 1, 1)[0][1, 0]) == sum(ref.poisson(ref.u(1, 1, 0, i)) for i in range(2000))   # (the same draws, one by one)


def test_replicate_counts_of_whole_and_fractional_weights():
    count = [1.0, 2.0, 0.5, 0.1, 2.5, 3.5]
    assert [ref.n_of(c) for c in count] == [1, 2, 1, 1, 2, 4]                                        # llrint: halves to the even integer
    k, c = ref.resample(count, 3, 7)
    assert k[0] == [1, 2, 1, 1, 2, 4] and c[0].tolist() == count
    for r in range(1, 4):
        assert k[r] == [ref.draws(7, r, g, n) for g, n in enumerate(k[0])]
        assert c[r].tolist() == [count[g] * float(k[r][g]) / float(k[0][g]) for g in range(6)]       # one multiplication, then one division
    assert c[1][3] == 0.1 * float(k[1][3]) and c[1][4] == 2.5 * float(k[1][4]) / 2.0 and c[1][5] == 3.5 * float(k[1][5]) / 4.0
    assert len({tuple(k[r]) for r in range(4)}) > 1
    ki, ci = ref.resample(count, 3, 7, identity=True)
    assert all(row == k[0] for row in ki) and all(row.tolist() == count for row in ci)


def test_vectorised_draws_are_the_restatement():
    count = cases.counts_for(24)
    k, c = ref.resample(count, 4, cases.SEED)
    kf, cf = cases.resample_fast(count, 4, cases.SEED)
    assert kf.tolist() == k and em_ref.same_bits(cf, c)
    assert set(count.tolist()) == set(cases.COUNTS)
    assert [ref.non_empty(row) for row in c] == [bool(np.any(row != 0)) for row in c]


# ---- the host code against the restatement -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("harness") / "boot_host_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(util.ROOT, "tests", "harness", "boot_host_harness.cpp"),
                    os.path.join(HOST, "refset.cpp"), os.path.join(HOST, "genotype.cpp"), "-lz", "-lpthread"], check=True)
    return exe


def _head(genes, series_names, series, gene, ec, eff, weight, frac=0.15):
    words = [float(frac).hex(), len(genes), len(series_names), len(series)] + list(genes) + list(series_names)
    for a in range(len(series)):
        words += [series[a], gene[a], ec[a], eff[a], weight[a]]
    return words


def _run(harness, tmp_path, words):
    p = str(tmp_path / "in.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    r = subprocess.run([harness, p], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cases_hold_the_situations():
    found = {}
    for name, c in cases.stat_cases().items():
        found[name] = c.situations()
    assert set().union(*found.values()) >= cases.SITUATIONS, found
    assert {"ties in rank", "a zero abundance", "an invalid replicate", "a series in both slots", "an uncalled series with top2 > 0"} <= found["main"]
    assert "V = 1" in found["one"] and "V = 0" in found["none"]


def test_table_worked_out_by_hand():
    rows = {(r[0], r[1]): r for r in cases.stat_cases()["main"].rows()}
    # G0*01 over the valid replicates 1, 2, 4, 5, 6: 8, 7, 2, 10, 4
    assert rows[(0, 0)][2:] == ("1", 8.0, 6.2, rows[(0, 0)][5], 2.0, 7.0, 10.0, 4, 4, 5, 5) and "%.6f" % rows[(0, 0)][5] == "3.193744"
    assert rows[(0, 1)][2] == "." and rows[(0, 1)][9:] == (1, 4, 4, 5)        # the tie of replicate 1 goes to G0*01, that of 6 to G0*02; 1 < 0.15 * 10 in replicate 5
    assert rows[(0, 2)][2] == "2" and rows[(0, 2)][9:] == (0, 2, 4, 5)        # 0 in replicate 1: neither ranked nor passed there
    assert rows[(1, 4)][2] == "1,2" and rows[(1, 3)][2] == "." and (2, 5) not in rows
    assert [k for k in rows] == [(0, 0), (0, 2), (0, 1), (1, 4), (1, 3)]      # slot 1, slot 2, then the rest
    text = cases.stat_cases()["main"].text()
    assert text.splitlines()[1] == "G0\tG0*01\t1\t8.000000\t6.200000\t3.193744\t2.000000\t7.000000\t10.000000\t4\t4\t5\t5"
    assert [ref.quantile_index(p, 5) for p in (5, 50, 95)] == [0, 2, 4] and [ref.quantile_index(p, 100) for p in (5, 50, 95)] == [4, 49, 94]
    assert [ref.quantile_index(p, 1) for p in (5, 50, 95)] == [0, 0, 0] and ref.quantile_index(95, 21) == 19
    one = {(r[0], r[1]): r for r in cases.stat_cases()["one"].rows()}
    assert one[(0, 0)][3:] == (8.0, 7.0, 0.0, 7.0, 7.0, 7.0, 1, 1, 1, 1)
    none = cases.stat_cases()["none"].rows()
    assert [(r[0], r[1]) for r in none] == [(0, 0), (0, 2), (1, 4)] and all(r[4:] == (0.0,) * 5 + (0, 0, 0, 0) for r in none)


@pytest.mark.parametrize("name", ["main", "one", "none"])
def test_host_table_is_the_restatement(harness, tmp_path, name):
    c = cases.stat_cases()[name]
    A = len(c.series)
    words = _head(cases.GENES, cases.SERIES, c.series, c.gene, [-1] * A, [1000] * A, [1] * A) + ["text", c.B]
    for sel in c.selected:
        words += [len(sel)] + [v for s in sel for v in s]
    words += [int(v) for v in c.valid] + [float(v).hex() for v in c.matrix.ravel().tolist()]
    got = _run(harness, tmp_path, words)
    assert got == c.text()
    assert got.startswith(ref.HEADER) and all(len(l.split("\t")) == 13 for l in got.splitlines())


def test_squarem_steps_are_the_restatement(harness, tmp_path):
    """the step functions quantify and both bootstrap drivers share, with the masking rule that writes into the run's own arrays, around
    a plain EM update: rounds, ecReadCount and the abundances bit for bit those of boot_ref.quantify; the run must pass a masked round"""
    t, cl = cases.small_em()
    for r, count in enumerate((t.count, t.count * np.array([(3 * g) % 4 for g in range(t.G)], np.float64) / 2.0)):
        n, rounds = ref.quantify((t.row_ptr, t.ec_idx), count, cl)
        assert rounds > 12 or r, rounds                                       # (the round of t = 10 is masked)
        masked = ref.masked_x0(cl, n)
        # the lengths go in per allele: every member of a class gets its class's length
        words = _head(["A", "B", "C"], ["s%d" % i for i in range(cl.n_series)], cl.series, cl.gene, cl.ec,
                      [int(cl.ec_len[e]) if e >= 0 else 1000 for e in cl.ec], cl.weight) + ["em", t.G]
        words += [int(v) for v in t.row_ptr] + [int(v) for v in t.ec_idx] + [float(v).hex() for v in count.tolist()]
        out = _run(harness, tmp_path, words).split()
        assert int(out[0]) == rounds
        got = np.array([float.fromhex(w) for w in out[1:]])
        assert em_ref.same_bits(got[:cl.E], n), em_ref.first_difference(got[:cl.E], n)
        assert em_ref.same_bits(got[cl.E:], ref.abundances(cl, n)[0])
        if r == 0:
            assert (masked == 0).any() and (masked > 0).any(), "the masking rule removes nothing here: pick another table"


# ---- the command line, the build -----------------------------------------------------------------------------------------------------
def test_usage_names_the_options(built):
    r = subprocess.run([GENO], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--bootstrap [INT]" in r.stderr and "prefix_bootstrap.tsv" in r.stderr and "--bootstrapSeed INT" in r.stderr


@pytest.mark.parametrize("value", ["0", "x", "1001", "-3", "5x"])
def test_bad_counts_are_usage_errors_that_write_nothing(built, tmp_path, value):
    c = goldens.Case("cyp_rna_2x100", str(tmp_path / "in"))
    out = str(tmp_path / "o")
    arg = ["--bootstrap=" + value] if value.startswith("-") else ["--bootstrap", value]
    r = subprocess.run([GENO] + c.args() + ["-o", out] + arg, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "--bootstrap takes an integer from 1 to 1000" in r.stderr and "./genotyper [OPTIONS]" in r.stderr
    assert glob.glob(out + "*") == []


@pytest.mark.parametrize("value", ["x", "-1", "18446744073709551616", "7 "])
def test_bad_seeds_are_usage_errors_that_write_nothing(built, tmp_path, value):
    c = goldens.Case("cyp_rna_2x100", str(tmp_path / "in"))
    out = str(tmp_path / "o")
    r = subprocess.run([GENO] + c.args() + ["-o", out, "--bootstrap", "3", "--bootstrapSeed=" + value], stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "--bootstrapSeed takes an unsigned 64-bit integer" in r.stderr and glob.glob(out + "*") == []


def test_abundance_file_with_bootstrap_is_a_usage_error_that_writes_nothing(built, tmp_path):
    c = goldens.Case("cyp_rna_2x100", str(tmp_path / "in"))
    out = str(tmp_path / "o")
    ab = str(tmp_path / "ab.tsv")
    open(ab, "w").write("x\t1\t1\t1\n")
    for args in (["-a", ab, "--bootstrap"], ["--bootstrap", "5", "-a", ab]):
        r = subprocess.run([GENO] + c.args() + ["-o", out] + args, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and "--bootstrap resamples the EM, which -a skips" in r.stderr and "./genotyper [OPTIONS]" in r.stderr
        assert glob.glob(out + "*") == []


def test_boot_symbols_declared_exported_and_bound(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    assert re.search(r"^int t1k_boot_begin\(t1k_ctx \*ctx, uint32_t nReplicates[^,]*, uint64_t seed, int identity\);", header, flags=re.M)
    assert re.search(r"^int t1k_boot_update\(t1k_ctx \*ctx, const uint8_t \*active, const double \*x0, double \*x1, double \*\w+, double \*diff\);", header, flags=re.M)
    # the two fields stand in front of --alternatives' (the last three fields of the structure are pinned by test_diplo_cpu.py)
    assert re.search(r"int32_t batch_fragments;.*\n\s*uint64_t bootstrap_seed;.*\n\s*int32_t bootstrap;.*\n\s*int32_t alternatives;", header)
    for name in ("t1k_boot_begin", "t1k_boot_counts", "t1k_boot_update", "t1k_boot_end", "t1k_boot_limits", "t1k_boot_nonempty", "t1k_boot_stride", "t1k_em_set_count",
                 "t1k_job_bootstrap_text", "t1k_job_bootstrap_matrix", "t1k_job_em_alleles", "t1k_job_series_names"):
        assert name in header and hasattr(L, name), name
    for name in ("boot_begin", "boot_counts", "boot_update", "boot_end", "boot_nonempty", "em_set_count"):
        assert hasattr(t1k_amd.Context, name), name
    assert hasattr(t1k_amd.Job, "bootstrap_text") and hasattr(t1k_amd.Job, "bootstrap_matrix")
    U, share, lanes = t1k_amd.boot_limits()
    assert U >= 2 and lanes == 64 and 3 < share <= 1000                                                    # (the resampling counts lie on both sides of it)
    assert [t1k_amd.boot_stride(b) for b in (1, 62, 63, 64, 127, 128, 1000)] == [64, 64, 64, 128, 128, 192, 1024]


def test_job_parameters_binding_has_the_size_of_the_structure(built):
    """t1k_job_params_default clears sizeof(t1k_job_params) bytes: the binding's structure must be exactly as long; no bootstrap, seed 1"""
    n = C.sizeof(t1k_amd.JobParams)
    buf = (C.c_uint8 * (n + 64))(*([0xEE] * (n + 64)))
    f = t1k_amd.lib().t1k_job_params_default
    keep, f.argtypes = f.argtypes, [C.c_void_p]
    try:
        f(C.addressof(buf))
    finally:
        f.argtypes = keep
    p = t1k_amd.JobParams.from_buffer(buf)
    assert bytes(buf[n:]) == b"\xee" * 64 and p.bootstrap == 0 and p.bootstrap_seed == 1 and p.diplo_candidates == 512 and p.filter_frac == 0.15
    assert t1k_amd.JobParams.bootstrap_seed.offset == t1k_amd.JobParams.batch_fragments.offset + 4 and t1k_amd.JobParams.bootstrap_seed.offset % 8 == 0
    assert t1k_amd.JobParams.bootstrap.offset + 4 == t1k_amd.JobParams.alternatives.offset and t1k_amd.JobParams.diplo_candidates.offset + 4 == n


def test_boot_kernels_use_no_scratch(tmp_path):
    """t1k_boot.hip compiled for gfx950 with the Makefile's flags: the compiler's resource remarks of the three kernels show no scratch
    memory and no LDS, and the class pass, which keeps 2 U operands and U contributions in registers, stays under 128 VGPRs"""
    hipcc, flags = hipcc_and_flags()
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "t1k_boot.o"), "t1k_boot.hip"], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", r.stdout)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        fig = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", b)}
        seen[name] = fig
    for kernel in ("k_boot_resample", "k_boot_rows", "k_boot_cols"):
        mine = [n for n in seen if kernel in n]
        assert len(mine) == 1, (kernel, sorted(seen))
        fig = seen[mine[0]]
        print(kernel, fig)
        assert fig["ScratchSize"] == 0 and fig["LDS Size"] == 0 and 0 < fig["VGPRs"] <= 128, (kernel, fig)
