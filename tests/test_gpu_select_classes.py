"""GPU tests of the selection by size class: k_select_classes sorts the read-ends of a range into three lists by candidate count
(1 .. 1000, 1001 .. 2048, beyond) and publishes the empty lists, every k_select launch takes its own list, and the two launches whose
lists can be cut decide what is emitted on the list as it lies (the latch by a min-reduction, `good` by a max-reduction:
t1k_amd/csrc/t1k_select_rule.h) and sort only once, in the cut.  References are built by hand as in tests/test_gpu_select_tail.py
(whose helpers are used here); every list is compared in order and field by field with the oracle's and with the same reads through a
context in eager mode, and every case asserts from the oracle's lists that the edge it is named for is hit before anything runs on the GPU.

What the alleles do to the read's overlap (150-base window, -s 0.8), as the oracle shows it in the controls below:
  failing      80 clean bases, then every other base wrong: a candidate whose extension fails -- the latch
  every(s)     60 clean bases, then every s-th base wrong (s = 3 .. 10): a shorter seed than the failing allele's, similarity 0.8 .. 0.94
  clip         the allele ends 70 bases into the window: a 70-base seed, clipped overlap with full credit (KEEPCLIP)
  sep          an N in the middle of the seed: a candidate that is never tried"""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_select_tail as tail
import util
from test_gpu_select_tail import W0, W1

pytestmark = pytest.mark.gpu


def every(root, step, start=60):
    return tail.swap(root, list(range(W0 + start, W1, step)))


def sep(root):
    return root[:W0 + 75] + "N" + root[W0 + 76:]


def oracle_list(tmp_path, name, alleles, read):
    (o, s), = tail.oracle_lists(tail.write_fasta(str(tmp_path / name), alleles), [read])
    return o, s


def check_ranges(fa, reads, orc, ranges, pairs=None):
    """tail.check for ranges that need not follow each other: every list of every range against the oracle's list of its read-end and
    against eager coverage; the deferred context's statistics per range"""
    got, stats, rows = tail.gpu_lists(fa, reads, True, ranges, pairs)
    eager, estats, erows = tail.gpu_lists(fa, reads, False, ranges, pairs)
    which = [first + j for first, count in ranges for j in range(count)]
    assert len(got) == len(which) == len(eager)
    for k, i in enumerate(which):
        o, s = orc[i]
        assert tail.same_as_oracle(o, s, got[k]), ("deferred", k, i, len(o), len(got[k]))
        assert tail.same_as_oracle(o, s, eager[k]), ("eager", k, i, len(o), len(eager[k]))
    for a, b in zip(stats, estats):
        assert a["extended"] == b["extended"] and a["near_best"] == b["near_best"] and a["candidates"] == b["candidates"], (a, b)
    if pairs:
        assert len(rows) == len(erows)
        for x, y in zip(rows, erows):
            assert np.array_equal(x, y)
    return stats


def test_size_edges(built, tmp_path):
    """1000 candidates (the launch without the cut's code), 1001 candidates with exactly 1000 emitted (the deciding launch, not cut: the list
    is sorted after the decision) and with 1001 emitted (cut), 2048 and 2049 candidates (the 256- and the 1024-thread shape), in one range
    and one range each"""
    rng = np.random.default_rng(212)

    def with_sep(root, i):
        return (tail.sign(sep(root), i), "sep") if i == 600 else tail.usual(root, i)
    genes = [tail.gene(rng, 1000), tail.gene(rng, 1001, with_sep), tail.gene(rng, 1001), tail.gene(rng, 2048), tail.gene(rng, 2049)]
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), [a for _, al, _ in genes for a in al])
    reads = [root[W0:W1] for root, _, _ in genes]
    orc = tail.oracle_lists(fa, reads)
    far = [kinds.count("far") for _, _, kinds in genes]
    assert min(far) >= 30
    assert len(orc[0][0]) == 1000 and int((orc[0][1] < 0.9).sum()) == far[0]            # 1000 emitted: nothing is cut
    assert len(orc[1][0]) == 1000 and int((orc[1][1] < 0.9).sum()) == far[1]            # 1001 candidates, the separator one is not emitted: not cut
    assert 600 + 1000 not in set(orc[1][0][:, 0].tolist())
    assert len(orc[2][0]) == 1001 - far[2] and orc[2][1].min() == 0.9                   # 1001 emitted: cut
    assert len(orc[3][0]) == 2048 - far[3] and len(orc[4][0]) == 2049 - far[4]
    tail.check(fa, reads, orc)
    stats = tail.check(fa, reads, orc, ranges=[(i, 1) for i in range(5)])
    assert [st["candidates"] for st in stats] == [1000, 1001, 1001, 2048, 2049]
    assert [st["extended"] for st in stats] == [1000, 1000, 1001, 2048, 2049]


def test_more_than_8192_candidates_around_an_empty_read_end(built, tmp_path):
    """8700 candidates (keys in HBM scratch: the reductions, the emit words and the bitonic network on them) on both strands, a read-end
    without candidates between the two (the reference of the selection tail's largest case)"""
    rng = np.random.default_rng(103)
    root, al, kinds = tail.gene(rng, 8700)
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1], tail.rand_seq(rng, 150), tail.revcomp(root[W0:W1])]
    orc = tail.oracle_lists(fa, reads)
    assert [len(o) for o, _ in orc] == [8700 - kinds.count("far"), 0, 8700 - kinds.count("far")] and len(orc[0][0]) > 8192
    stats = tail.check(fa, reads, orc, pairs=[(0, 2), (1, 1)])
    assert stats[0]["candidates"] == 2 * 8700


def test_more_than_256_classes_in_the_cut(built, tmp_path):
    """the cut's sort of a list decided in candidate order: more than 256 classes, the bitonic network in LDS"""
    rng = np.random.default_rng(204)
    root = tail.rand_seq(rng, 300)
    made, seen = [], set()
    for i in range(1500):
        a, k = tail.clipped(root, i)
        if a not in seen:
            seen.add(a)
            made.append((a, k))
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), [a for a, _ in made])
    reads = [root[W0:W1]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    far = [k for _, k in made].count("far")
    assert far >= 20 and 1000 < len(o) == len(made) - far and len(tail.classes(o)) > 256
    tail.check(fa, reads, orc)


STEPS = (3, 4, 5, 6, 7, 8, 10)   # every(s): similarity 0.8, 0.847, 0.88, 0.9, 0.913, 0.92, 0.94


def controls(tmp_path, root):
    """what the kinds of alleles do, on small references"""
    read = root[W0:W1]
    short = [tail.sign(every(root, st), i + 1) for i, st in enumerate(STEPS)]
    fail = tail.sign(tail.failing(root), 0)
    # the failing allele is in front of every every(s): with nothing emitted before it all of them are tried ...
    o, s = oracle_list(tmp_path, "c1.fa", [fail] + short, read)
    assert sorted(o[:, 0].tolist()) == list(range(1, 8)) and s.min() == 0.8 and s.max() == 0.94
    # ... and with a perfect allele before it none of them is
    o, _ = oracle_list(tmp_path, "c2.fa", [fail] + short + [tail.sign(root, 9)], read)
    assert o[:, 0].tolist() == [8]
    o, _ = oracle_list(tmp_path, "c3.fa", short + [tail.sign(root, 9)], read)
    assert len(o) == 8
    # the clipped allele is tried behind the latch although its seed is the shorter one, the separator allele never
    o, _ = oracle_list(tmp_path, "c4.fa", [fail, short[1], tail.sign(root, 9), tail.sign(root[:W0 + 70], 10), tail.sign(sep(root), 11)], read)
    assert sorted(o[:, 0].tolist()) == [2, 3] and int(o[o[:, 0] == 3][0, 8]) == 80


def test_latch_first(built, tmp_path):
    """the failing allele is the first candidate of the selection's order (it has the longest seed of the list): nothing is emitted before
    the latch, `good` stays -1 and every other candidate is tried; 1200 are emitted and the cut removes the ones at 0.8 (best 0.94)"""
    rng = np.random.default_rng(205)
    root = tail.rand_seq(rng, 300)
    controls(tmp_path, root)
    al = [tail.sign(tail.failing(root), i) if i == 500 else tail.sign(every(root, STEPS[i % 7]), i) for i in range(1201)]
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    gone = [i for i in range(1201) if i != 500 and STEPS[i % 7] == 3]
    assert len(o) == 1200 - len(gone) > 1000 and not set(o[:, 0].tolist()) & set(gone + [500]) and s.max() == 0.94 and s.min() > 0.84
    stats = tail.check(fa, reads, orc)
    assert stats[0]["candidates"] == 1201 and stats[0]["extended"] == 1200


def test_nothing_emitted_before_the_latch(built, tmp_path):
    """as above with separator alleles, which have the longest seeds of all, in front of the latch: the latch is not the first candidate,
    and still nothing is emitted before it"""
    rng = np.random.default_rng(206)
    root = tail.rand_seq(rng, 300)
    al = [tail.sign(tail.failing(root), i) if i == 500 else tail.sign(sep(root), i) if i % 40 == 3 else tail.sign(every(root, STEPS[i % 7]), i) for i in range(1300)]
    seps = [i for i in range(1300) if i % 40 == 3 and i != 500]
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    gone = [i for i in range(1300) if i != 500 and i not in seps and STEPS[i % 7] == 3]
    emitted = 1300 - 1 - len(seps)
    assert emitted > 1000 and len(o) == emitted - len(gone) and not set(o[:, 0].tolist()) & set(gone + seps + [500])
    stats = tail.check(fa, reads, orc)
    assert stats[0]["candidates"] == 1300 and stats[0]["extended"] == emitted


def behind_mix(root, i):
    """the usual mix with a failing allele, alleles of a shorter seed that the latch keeps from being tried, clipped alleles of a still
    shorter seed that are tried all the same (KEEPCLIP), separator alleles, and alleles the cut removes that lie before the latch (18 .. 23
    mismatches behind 104 clean bases)"""
    m = i % 25
    if i == 333:
        return tail.sign(tail.failing(root), i), "fail"
    if m in (0, 14):
        return tail.sign(sep(root), i), "sep"
    if m in (9, 16):
        return tail.sign(every(root, 4), i), "late"
    if m == 21:
        return tail.sign(root[:W0 + 70 - i % 6], i), "clip"
    if m == 7:
        return tail.sign(tail.mism(root, 18 + (i // 25) % 6, at=104), i), "far"
    return tail.usual(root, i)


def test_keepclip_behind_the_latch_and_separators_between(built, tmp_path):
    """candidates behind the latch with a seed match count below `good`: the ones that need clipping at a seed similarity of at least 0.95
    are emitted, the others are not; separator candidates lie between emitted ones in the candidate order"""
    rng = np.random.default_rng(207)
    root, al, kinds = tail.gene(rng, 1700, behind_mix)
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    in_list = set(o[:, 0].tolist())
    of = lambda kind: [i for i, k in enumerate(kinds) if k == kind]
    assert len(of("clip")) > 50 and in_list >= set(of("clip")) and int((o[:, 8] > 0).sum()) == len(of("clip"))   # tried behind the latch
    assert len(of("late")) > 100 and not in_list & set(of("late"))                                                # not tried
    assert not in_list & set(of("sep") + of("fail")) and sum(1 for i in of("sep") if min(in_list) < i < max(in_list)) > 100
    assert len(of("far")) > 50 and not in_list & set(of("far")) and len(o) > 1000                                  # emitted, and cut
    stats = tail.check(fa, reads, orc)
    assert stats[0]["candidates"] == 1700 and stats[0]["extended"] >= len(o) + len(of("far"))


def test_no_failed_extension(built, tmp_path):
    """no latch: every candidate without a separator is emitted (1400 candidates, separator alleles in between), and the list is cut"""
    rng = np.random.default_rng(208)

    def mix(root, i):
        return (tail.sign(sep(root), i), "sep") if i % 25 in (0, 14) else tail.usual(root, i)
    root, al, kinds = tail.gene(rng, 1400, mix)
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    emitted = 1400 - kinds.count("sep")
    assert emitted > 1000 and len(o) == emitted - kinds.count("far") and s.min() == 0.9
    stats = tail.check(fa, reads, orc)
    assert stats[0]["candidates"] == 1400 and stats[0]["extended"] == emitted


@pytest.mark.parametrize("fail_first", [True, False])
def test_tie_with_the_latch(built, tmp_path, fail_first):
    """two candidates on one allele in one seed class (80 clean bases each), one of which fails its extension: which of them comes first
    on the allele decides whether the other lies before the latch.  Perfect alleles sit in front (`good` is their seed match count), so
    behind the latch the passing copy is not tried, before it it is emitted: the two orders give different lists"""
    rng = np.random.default_rng(209)
    root, al, kinds = tail.gene(rng, 1300)
    junk = tail.rand_seq(rng, 40)
    bad, ok = tail.mism(root, 35, at=80), tail.swap(root, list(range(W0 + 80, W1, 6)))
    both = {}
    for first in (True, False):
        a, b = (bad, ok) if first else (ok, bad)
        mine = list(al)
        mine[400] = a[:W1] + junk + b[W0:]
        both[first] = tail.oracle_lists(tail.write_fasta(str(tmp_path / ("ref%d.fa" % first)), mine), [root[W0:W1]])
    (of, sf), (op, sp) = both[True][0], both[False][0]
    assert 400 not in set(of[:, 0].tolist()) and int((op[:, 0] == 400).sum()) == 1 and len(op) == len(of) + 1 > 1000
    assert np.array_equal(op[op[:, 0] != 400], of) and float(sp[op[:, 0] == 400][0]) >= 0.9   # (the passing copy survives the cut)
    stats = tail.check(str(tmp_path / ("ref%d.fa" % fail_first)), [root[W0:W1]], both[fail_first])
    assert stats[0]["candidates"] == 1301


def test_class_lists_over_ranges(built, tmp_path):
    """ranges in which a class is empty, a range of read-ends without candidates only, read-ends without candidates between the others, a
    second, smaller range after a larger one on the same context (the class lists still hold the larger range's read-ends), and mate
    pairing from the lists of all of them (the empty ones' published tables are read there)"""
    rng = np.random.default_rng(210)
    big, mid, small = tail.gene(rng, 2100), tail.gene(rng, 1100), tail.gene(rng, 60)
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), big[1] + mid[1] + small[1])
    rb, rm, rs = big[0][W0:W1], mid[0][W0:W1], small[0][W0:W1]
    none = lambda: tail.rand_seq(rng, 150)
    reads = [rb, none(), rm, rs, none(), tail.revcomp(rb), rs, tail.revcomp(rm), none(), none(), tail.revcomp(rs), none(), rm, none()]
    orc = tail.oracle_lists(fa, reads)
    fb, fm = big[2].count("far"), mid[2].count("far")
    B, M, S = 2100 - fb, 1100 - fm, 60
    assert [len(o) for o, _ in orc] == [B, 0, M, S, 0, B, S, M, 0, 0, S, 0, M, 0] and fb > 30 and fm > 30
    pairs = [(0, 5), (2, 7), (3, 6), (1, 4), (8, 10), (12, 13), (9, 11)]
    # all three classes and the empty ones in one range; then the same read-ends again in smaller ranges: the long lists alone, the empty
    # ones alone (8 .. 9), the short lists with empty ones in between (8 .. 11), a middle list between empty ones
    stats = check_ranges(fa, reads, orc, [(0, 14), (5, 1), (8, 2), (8, 4), (11, 3), (0, 14)], pairs)
    assert [st["candidates"] for st in stats] == [2 * 2100 + 3 * 1100 + 3 * 60, 2100, 0, 60, 1100, 2 * 2100 + 3 * 1100 + 3 * 60]
    check_ranges(fa, reads, orc, [(0, 7), (7, 7)], pairs)


def test_long_reads_through_the_large_shape(built, tmp_path):
    """1000-base read-ends (the wide key fields) with 2100 candidates: the 1024-thread shape's decision and cut; 110 .. 166 mismatches go"""
    rng = np.random.default_rng(211)
    root = tail.rand_seq(rng, 1100)
    al, kinds = [], []
    for i in range(2100):
        m = i % 25
        k, kind = (110 + 8 * (i // 25 % 8), "far") if m == 7 else (100, "bound") if m == 11 else (i % 4, "near")
        al.append(tail.sign(tail.swap(root, [50 + 300 + 3 * j for j in range(k)]), i))
        kinds.append(kind)
    fa = tail.write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[50:1050], root[900:1050]]
    orc = tail.oracle_lists(fa, reads)
    o, s = orc[0]
    assert len(o) == 2100 - kinds.count("far") and s[0] == 1.0 and s.min() == 0.9 and int(o[:, 2].max()) == 999
    assert len(orc[1][0]) == 2100
    stats = tail.check(fa, reads, orc)
    assert stats[0]["candidates"] == 2 * 2100


def test_through_the_job_with_read_ends_of_earlier_windows(built, tmp_path):
    """the executable on a sample whose lists are cut, small windows, and the first 300 pairs once more at the end of the files: their
    read-ends are linked to an earlier window's (skipped in the range: k_select_classes must leave their table entries alone).  Every
    output file is the same with deferred and with eager coverage"""
    geno = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
    ref = str(tmp_path / "ref.fa")
    util.synth_ref("ref-rna", ref, genes=2, scale=0.2, seed=43)
    pfx = str(tmp_path / "r")
    util.synth_reads(ref, pfx, pairs=1500, len=150, seed=9, sub=0.004)
    for end in ("_1.fq", "_2.fq"):
        lines = open(pfx + end).read().split("\n")
        with open(pfx + end, "a") as f:
            f.write("\n".join(lines[:4 * 300]) + "\n")
    args = ["-f", ref, "-1", pfx + "_1.fq", "-2", pfx + "_2.fq", "-s", "0.8"]
    small = {"T1K_FIRST_WINDOW": "256", "T1K_WINDOW": "512", "T1K_BATCH": "96", "T1K_PAIR_BATCH": "256", "T1K_PIPELINES": "1"}
    out = {}
    for tag, env in (("deferred", dict(small, T1K_DEBUG_PHASES="1", T1K_DEBUG_TASKS="1")), ("eager", dict(small, T1K_COVERAGE="eager"))):
        out[tag] = str(tmp_path / tag)
        r = subprocess.run([geno] + args + ["-o", out[tag]], stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (tag, r.stderr[-500:])
        if tag == "deferred":
            linked = [int(x) for x in re.findall(r"(\d+) read-ends linked to earlier windows", r.stderr)]
            assert sum(linked) > 0, linked
            acc = re.findall(r"packed selection: cand \d+ emitted (\d+) kept (\d+)", r.stderr)
            assert sum(int(e) for e, _ in acc) > sum(int(k) for _, k in acc) > 0, acc[:5]
    for suf in ("_genotype.tsv", "_allele.tsv", "_aligned_1.fa", "_aligned_2.fa"):
        assert open(out["deferred"] + suf, "rb").read() == open(out["eager"] + suf, "rb").read(), suf
