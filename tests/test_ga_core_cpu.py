"""CPU test of the one-word gap-alignment sweeps (tests/harness/ga_core_cmp.cpp): the text of the alignment routines is taken from
t1k_amd/csrc/t1k_dev.h as it is, compiled for the host with the device intrinsics shimmed, linked into a stand-alone program under the
address and undefined-behaviour sanitizers, and the one-word routines (t1k_ga_matches_equal_w, t1k_ga_band_w<4>) are compared with the int32
routines that stay as their fallback (t1k_ga_matches_equal, t1k_ga_band<4, false>): match count and score, equal lengths and length
differences of -4 .. +4, lengths from 2 to both sides of the one-word bound (AlignAlgo.hpp:215-421)."""
import gzip
import os
import subprocess

import pytest

import util

BEGIN = "// accessor for one sequence operand of the alignment routines"
END = "// Exact fast path for equal lengths"
CASES, SEED = 120000, 11
# what the generator gives for (CASES, SEED), rounded down: the comparison must not pass on inputs that never leave the diagonal, never
# reach the bound, or never differ in length.  (offdiag counts equal-length pairs only: the optimum's score exceeds the ungapped score.)
FLOOR = {"offdiag": 30000, "beyond": 7000, "unequal": 70000, "inrange": 110000}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ga_core"))
    dev = open(os.path.join(util.ROOT, "t1k_amd", "csrc", "t1k_dev.h")).read()
    a, b = dev.index(BEGIN), dev.index(END)
    harness = open(os.path.join(util.ROOT, "tests", "harness", "ga_core_cmp.cpp")).read()
    src = os.path.join(tmp, "ga_core_cmp_full.cpp")
    open(src, "w").write(harness.replace("@@ROUTINE@@", dev[a:b]))
    out = os.path.join(tmp, "ga_core_cmp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
    return out


def test_one_word_sweeps_equal_the_int32_sweeps_on_random_pairs(exe):
    r = subprocess.run([exe, "random", str(CASES), str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok cases"), (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1, 2)}
    print(got)
    assert got["cases"] == CASES
    for key, floor in FLOOR.items():
        assert got[key] >= floor, (key, got)


def test_one_word_sweeps_on_the_reference_vectors(exe, tmp_path):
    """the committed outputs of the reference's own GlobalAlignment with |length difference| <= 4: both routines must give the number of MATCH
    columns of its traceback"""
    path = str(tmp_path / "vectors.tsv")
    n = 0
    with gzip.open(os.path.join(util.GOLDEN, "ga_vectors.tsv.gz"), "rt") as f, open(path, "w") as out:
        for line in f:
            t, p, score, ops = line.rstrip("\n").split("\t")
            if abs(len(t) - len(p)) > 4 or not t or not p or (len(t) == len(p) and len(t) < 2):
                continue   # the band routines take 1 .. (2 .. when equal) bases a side
            out.write("%s\t%s\t%d\n" % (t, p, ops.count("0")))
            n += 1
    assert n > 600
    r = subprocess.run([exe, "vectors", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok vectors %d" % n, (r.stdout[-2000:], r.stderr[-2000:])
