"""CPU test of the selection's emit rule on an unsorted list (t1k_amd/csrc/t1k_select_rule.h, which k_select's CUT instantiations call):
tests/harness/select_emit_san.cpp, a stand-alone host program built with the address and undefined-behaviour sanitizers, decides random
lists by the rule (latch by min-reduction and exact settlement of its ties, `good` by max-reduction, emit predicate) and by the positional
rule of the sorted selection, and checks the cut's bitmap prefix -> position mapping at word boundaries.  The lists include equal keys up
to the candidate number, no latch, the latch first, no emitted candidate before the latch, and KEEPCLIP candidates behind the latch."""
import os
import shutil
import subprocess

import pytest

import util


def test_emit_rule_and_bitmap_positions_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(util.ROOT, "tests", "harness", "select_emit_san.cpp")
    exe = str(tmp_path / "select_emit_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(util.ROOT, "t1k_amd", "csrc"), "-o", exe, src], check=True)
    for seed in ("1", "2"):
        r = subprocess.run([exe, "100000", seed], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
        lists, no_latch, latch_first, good_none, keep_behind, latch_tie, full_tie, bitmaps = [int(x) for x in r.stdout.replace(":", " ").split() if x.isdigit()]
        assert lists == 100000
        # every kind of list the rule has a branch for was really decided
        assert no_latch > 5000 and latch_first > 5000 and good_none > 5000 and keep_behind > 5000, r.stdout
        assert latch_tie > 5000 and full_tie > 1000, r.stdout   # candidates of the latch's class and allele; equal up to the candidate number
        assert bitmaps == 14 * 6
