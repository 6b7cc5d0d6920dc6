"""GPU tests of the selection tail at its edges: with deferred coverage (and no --relaxIntronAlign) k_select cuts the lists of more than
1000 emitted overlaps itself and writes the kept records to the overlap store in the packed form; with eager coverage the unfused
sequence (k_select, full alignments, k_truncate, k_pack_overlaps, k_publish_lists) runs.  Every case builds a small reference by hand --
alleles of a few hundred bases derived from one root sequence per gene, a read that is a window of the root, so that the read-end
overlaps every allele of the gene and the list length follows the allele count -- and compares every read-end's list, in order and field
by field, with the oracle's (util.Oracle.assign_read) and with the same reads through a context left in eager mode.  Before any GPU run
each case asserts from the oracle's lists that the edge it is named for is really hit.

What an allele does to the read's overlap (150-base window, -s 0.8), as the oracle shows it:
  k mismatches in the window      matchCnt 300 - 2 k, similarity (150 - k) / 150: k <= 15 stays within 0.1 of a perfect allele (k = 15 is
                                  exactly 0.9: kept, the comparison is strict), 16 <= k <= 30 passes -s and is cut from a list of more than
                                  1000, k > 30 fails its extension
  an N inside the seed            no overlap (separator in the seed)
  allele starts / ends inside     clipped overlap with full credit: matchCnt and span sum as for the full window, shorter read span
  the window twice                two overlaps on one allele
The last case but one runs the long-read (XL) key widths: 1000-base reads, a list that is cut."""
import os
import subprocess

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

ROT = {"A": "C", "C": "G", "G": "T", "T": "A"}
W0, W1 = 70, 220   # the read's window in a 300-base root
SIM = 0.8


def rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def swap(s, positions):
    s = list(s)
    for p in positions:
        s[p] = ROT[s[p]]
    return "".join(s)


def sign(s, i, at=4):
    """allele number i written into the bases in front of the window: alleles of one kind stay distinct sequences"""
    s = list(s)
    k = 0
    while i:
        for _ in range(i & 3):
            s[at + 2 * k] = ROT[s[at + 2 * k]]
        i >>= 2
        k += 1
    return "".join(s)


def mism(root, k, at=60):
    """k mismatches inside the window, on every other base from window offset `at`"""
    return swap(root, [W0 + at + 2 * j for j in range(k)])


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def usual(root, i):
    """the allele mix of most cases, by allele number: 1 in 25 cut from a long list (16 .. 25 mismatches), 1 in 25 exactly at the cut's
    bound (15: kept), 1 in 25 just above it (14), the others 0 .. 3 mismatches (four classes, interleaved in allele order)"""
    m = i % 25
    if m == 7:
        return sign(mism(root, 16 + (i // 25) % 10), i), "far"
    if m == 11:
        return sign(mism(root, 15), i), "bound"
    if m == 19:
        return sign(mism(root, 14), i), "near"
    return sign(mism(root, i % 4), i), "near"


def gene(rng, n, make=usual):
    root = rand_seq(rng, 300)
    made = [make(root, i) for i in range(n)]
    return root, [a for a, _ in made], [k for _, k in made]


def write_fasta(path, alleles):
    assert len(set(alleles)) == len(alleles)
    with open(path, "w") as f:
        for i, a in enumerate(alleles):
            f.write(">G%d*01:%02d:%02d\n%s\n" % (i // 9000, i // 90 % 100, i % 90 + 1, a))
    return path


def oracle_lists(fa, reads):
    orc = util.Oracle(fa, similarity=SIM)
    return [orc.assign_read(r) for r in reads]


def classes(o):
    """the distinct (match count, span sum with clips, read span) of a list: what the cut's order sorts by before the allele"""
    return set(zip(o[:, 6].tolist(), (o[:, 2] - o[:, 1] + 1 + o[:, 4] - o[:, 3] + 1 + 2 * o[:, 7] + 2 * o[:, 8]).tolist(), (o[:, 2] - o[:, 1]).tolist()))


FIELDS = ("seq_idx", "read_start", "read_end", "seq_start", "seq_end", "strand", "match_cnt", "left_clip", "right_clip", "relaxed_match_cnt")


def same_as_oracle(o, s, g):
    return len(o) == len(g) and all(np.array_equal(o[:, k], g[f]) for k, f in enumerate(FIELDS)) and np.array_equal(s, g["similarity"])


def gpu_lists(fa, reads, deferred, ranges=None, pairs=None):
    """the lists of every read-end (one array per read-end) from a bare context, the statistics of every range and, with `pairs`
    ((end1, end2) read-end numbers), the rows mate pairing makes of the lists the read set holds after the last range"""
    import t1k_amd
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(fa)
    ctx = t1k_amd.Context(ref_seq_similarity=SIM)
    try:
        ctx.set_coverage_mode(deferred)
        ctx.ref_upload(seqs, masks)
        ctx.reads_upload(reads)
        lists, stats = [], []
        for first, count in ranges or [(0, len(reads))]:
            ctx._check(t1k_amd.lib().t1k_assign_range(ctx.h, first, count), "t1k_assign_range")
            counts, ovl = ctx.overlaps()
            assert int(counts[:count].sum()) == len(ovl)
            pos = 0
            for i in range(count):
                lists.append(ovl[pos:pos + counts[i]].copy())
                pos += counts[i]
            stats.append(ctx.stats())
        rows = None
        if pairs:
            ctx.pair([a for a, _ in pairs], [b for _, b in pairs], [0] * len(pairs))
            rows = ctx.rows()
        return lists, stats, rows
    finally:
        ctx.close()


def check(fa, reads, orc, ranges=None, pairs=None):
    """deferred coverage (the packed selection) against the oracle and against eager coverage (the unfused sequence); returns the
    deferred context's statistics per range"""
    got, stats, rows = gpu_lists(fa, reads, True, ranges, pairs)
    eager, estats, erows = gpu_lists(fa, reads, False, ranges, pairs)
    assert len(got) == len(reads) == len(eager)
    for i, (o, s) in enumerate(orc):
        assert same_as_oracle(o, s, got[i]), ("deferred", i, len(o), len(got[i]))
        assert same_as_oracle(o, s, eager[i]), ("eager", i, len(o), len(eager[i]))
        assert np.array_equal(got[i], eager[i]), i
    for a, b in zip(stats, estats):  # the statistics keep their meaning: overlaps emitted (before the cut) and near-best among them
        assert a["extended"] == b["extended"] and a["near_best"] == b["near_best"] and a["candidates"] == b["candidates"], (a, b)
    if pairs:
        for x, y in zip(rows, erows):
            assert np.array_equal(x, y)
    return stats


def test_cut_threshold(built, tmp_path):
    """emitted lists of exactly 999, 1000, 1001 and 1002 records (one gene each, one read-end each): nothing is cut up to 1000; from 1001 on
    the alleles more than 0.1 below the best go, the ones exactly 0.1 below stay"""
    rng = np.random.default_rng(101)
    sizes = (999, 1000, 1001, 1002)
    genes = [gene(rng, n) for n in sizes]
    fa = write_fasta(str(tmp_path / "ref.fa"), [a for _, al, _ in genes for a in al])
    reads = [root[W0:W1] for root, _, _ in genes]
    orc = oracle_lists(fa, reads)
    for (root, al, kinds), (o, s), n in zip(genes, orc, sizes):
        far, bound = kinds.count("far"), kinds.count("bound")
        assert far >= 30 and bound >= 30
        assert s[0] == 1.0 and int((s == 0.9).sum()) == bound          # exactly 0.1 below the best: kept in every list
        if n <= 1000:
            assert len(o) == n and int((s < 0.9).sum()) == far         # everything emitted, nothing cut
        else:
            assert len(o) == n - far < n and s.min() == 0.9            # the cut list is shorter than the emitted one
    stats = check(fa, reads, orc)
    assert stats[0]["extended"] == sum(sizes)


def test_shape_boundary(built, tmp_path):
    """candidate lists of 2048 (the 256-thread shape's last) and 2049 (the 1024-thread shape's first), both cut"""
    rng = np.random.default_rng(102)
    sizes = (2048, 2049)
    genes = [gene(rng, n) for n in sizes]
    fa = write_fasta(str(tmp_path / "ref.fa"), [a for _, al, _ in genes for a in al])
    reads = [root[W0:W1] for root, _, _ in genes]
    orc = oracle_lists(fa, reads)
    for (root, al, kinds), (o, s), n in zip(genes, orc, sizes):
        assert 1000 < len(o) == n - kinds.count("far") < n   # every allele but the cut ones is in the list: n candidates, all emitted
    stats = check(fa, reads, orc, ranges=[(0, 1), (1, 1)])
    assert [st["candidates"] for st in stats] == list(sizes) and [st["extended"] for st in stats] == list(sizes)


def test_more_than_8192_candidates(built, tmp_path):
    """read-ends with 8700 candidates: the keys of both orderings live in HBM scratch (bitonic network)"""
    rng = np.random.default_rng(103)
    root, al, kinds = gene(rng, 8700)
    fa = write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1], revcomp(root[W0:W1])]
    orc = oracle_lists(fa, reads)
    for o, s in orc:
        assert 8192 < len(o) == 8700 - kinds.count("far") < 8700
    assert orc[0][0][0, 5] == 1 and orc[1][0][0, 5] == -1  # both strands
    stats = check(fa, reads, orc)
    assert stats[0]["candidates"] == 2 * 8700


def clipped(root, i):
    """alleles that start and end inside the window (clipped overlaps with full credit: the read span varies with a + b) with 0 .. 3
    mismatches: more than 256 classes; every 25th a full allele of the usual mix's cut / bound kinds"""
    if i == 0:
        return sign(root, i), "near"
    if i % 25 == 7:
        return sign(mism(root, 16 + i % 10), i), "far"
    t, v = i % 300, i // 300
    k, both = t % 4, t // 4              # 4 match counts x 75 read spans; v: another split of a + b, other places for the mismatches
    a = 1 + (both // 2 + v) % (both + 1)
    b = both + 2 - a
    s = swap(root, [W0 + a + 20 + 2 * ((5 * j + v) % 12) for j in range(k)])
    return s[W0 + a:W1 - b], "clip"


def test_more_than_256_classes(built, tmp_path):
    """a list of more than 1000 emitted records with more than 256 distinct (match count, span sum, read span): the class ranks do not
    fit the counting pass, the bitonic network orders the keys in LDS"""
    rng = np.random.default_rng(104)
    root = rand_seq(rng, 300)
    made, seen = [], set()
    for i in range(1500):
        a, k = clipped(root, i)
        if a not in seen:
            seen.add(a)
            made.append((a, k))
    fa = write_fasta(str(tmp_path / "ref.fa"), [a for a, _ in made])
    reads = [root[W0:W1]]
    orc = oracle_lists(fa, reads)
    o, s = orc[0]
    far = [k for _, k in made].count("far")
    assert far >= 20 and 1000 < len(o) == len(made) - far
    assert len(classes(o)) > 256, len(classes(o))
    assert int((o[:, 7] > 0).sum()) > 500 and int((o[:, 8] > 0).sum()) > 500   # clips on either side
    check(fa, reads, orc)


def test_ties(built, tmp_path):
    """two overlaps on one allele with equal class in a list that is cut: alleles that hold the window twice (the overlaps tie in read
    start and read end, the allele position decides) and alleles that hold its two ends, each cut off by an N (equal read span, the
    read start decides)"""
    rng = np.random.default_rng(105)
    root, al, kinds = gene(rng, 1100)
    junk = rand_seq(rng, 40)
    twice = {200: root[:W1] + junk + root[W0:], 611: mism(root, 2)[:W1] + junk + mism(root, 2)[W0:]}
    ends = {333: root[W0 + 12:W1 + 20] + "N" + root[W0 - 20:W1 - 12], 902: root[W0 + 30:W1 + 20] + "N" + root[W0 - 20:W1 - 30]}
    for i, a in list(twice.items()) + list(ends.items()):
        al[i], kinds[i] = a, "double"
    fa = write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    orc = oracle_lists(fa, reads)
    o, s = orc[0]
    assert 1000 < len(o) == 1100 + 4 - kinds.count("far")   # emitted 1104 > 1000, and cut
    for i in list(twice) + list(ends):
        mine = o[o[:, 0] == i]
        assert len(mine) == 2 and len(classes(mine)) == 1, (i, mine)
        lead_tie = mine[0, 1] == mine[1, 1] and mine[0, 2] == mine[1, 2]
        assert lead_tie == (i in twice), (i, mine)
    check(fa, reads, orc)


def failing(root):
    return mism(root, 35, at=80)


def latched(root):
    return swap(root, [W0 + 60 + 4 * j for j in range(22)])


def gapped(root, i):
    """the usual mix with, in between, candidates that are not emitted: an N in the middle of the seed, extensions that fail (35 mismatches
    behind 80 clean bases) and alleles of a shorter seed (60 clean bases, then every fourth base wrong: 0.85, enough for -s) that the latch
    left by a failed extension keeps from being tried; the alleles a cut removes carry their 18 .. 23 mismatches behind 104 clean bases,
    a longer seed than the failing alleles': they are tried before the latch"""
    m = i % 25
    if m in (0, 14):
        return sign(root[:W0 + 75] + "N" + root[W0 + 76:], i), "sep"
    if m in (5, 21):
        return sign(failing(root), i), "fail"
    if m in (9, 16, 23):
        return sign(latched(root), i), "late"
    if m == 7:
        return sign(mism(root, 18 + (i // 25) % 6, at=104), i), "far"
    return usual(root, i)


@pytest.mark.parametrize("n,above", [(1420, True), (1350, False)])
def test_not_everything_emitted(built, tmp_path, n, above):
    """more than 1000 candidates of which the separator rule, failed extensions and the latch rule remove some before and between the
    emitted ones -- the compaction by candidate number is not the identity -- with just more and just fewer than 1000 emitted"""
    rng = np.random.default_rng(106)
    root, al, kinds = gene(rng, n, gapped)
    fa = write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[W0:W1]]
    # what the latch does, on a control: behind the failed extension the allele of the shorter seed is not tried (without the failing
    # allele it is), the alleles of 18 .. 23 mismatches at the window's end are, and their similarity says which of them a cut removes
    ctl = [sign(root, 1), sign(failing(root), 2), sign(latched(root), 3)] + [sign(mism(root, k, at=104), k) for k in range(18, 24)]
    (o3, s3), = oracle_lists(write_fasta(str(tmp_path / "ctl3.fa"), ctl), reads)
    (o2, _), = oracle_lists(write_fasta(str(tmp_path / "ctl2.fa"), ctl[:1] + ctl[2:]), reads)
    assert sorted(o3[:, 0].tolist()) == [0] + list(range(3, 9)) and sorted(o2[:, 0].tolist()) == list(range(8))
    cut_k = set(int(a) - 3 + 18 for a, x in zip(o3[:, 0], s3) if a >= 3 and x < s3.max() - 0.1)
    orc = oracle_lists(fa, reads)
    o, s = orc[0]
    gone = [i for i, k in enumerate(kinds) if k in ("sep", "fail", "late")]
    cut = [i for i, k in enumerate(kinds) if k == "far" and 18 + (i // 25) % 6 in cut_k]
    emitted = n - len(gone)
    in_list = set(o[:, 0].tolist())
    assert len(gone) > 350 and not in_list & set(gone) and min(gone) < min(in_list) and sum(1 for i in gone if min(in_list) < i < max(in_list)) > 350
    if above:
        assert 1000 < emitted <= 1040 and len(cut) > 10 and len(o) == emitted - len(cut) and not in_list & set(cut)
    else:
        assert 960 <= emitted < 1000 and len(cut) > 10 and len(o) == emitted and in_list >= set(cut)
    stats = check(fa, reads, orc)
    assert stats[0]["extended"] == emitted and stats[0]["candidates"] > 1000


def test_mixed_ranges(built, tmp_path):
    """read-ends without candidates, with short lists and with cut lists in one range, and two ranges in a row on one context: the second
    range's records go behind the first range's kept ones (mate pairing across the two ranges reads both)"""
    rng = np.random.default_rng(107)
    big, small = gene(rng, 1100), gene(rng, 60)
    fa = write_fasta(str(tmp_path / "ref.fa"), big[1] + small[1])
    rb, rs = big[0][W0:W1], small[0][W0:W1]
    reads = [rb, rand_seq(rng, 150), rs, revcomp(rs), revcomp(rb), rand_seq(rng, 150), big[0][W0 + 20:W1 + 20]]
    orc = oracle_lists(fa, reads)
    sizes = [len(o) for o, _ in orc]
    far = big[2].count("far")
    assert sizes == [1100 - far, 0, 60, 60, 1100 - far, 0, 1100 - far] and far > 30
    check(fa, reads, orc, ranges=[(0, 3), (3, 4)], pairs=[(0, 4), (2, 3), (1, 5), (0, 6)])
    check(fa, reads, orc, ranges=[(0, 7)])


def test_long_reads(built, tmp_path):
    """1000-base read-ends (beyond the fast windows' read length: key fields as wide as the read needs) with a list of 1060 overlaps that
    is cut: 110 .. 166 mismatches go, 100 (exactly 0.9) stay; a 150-base read-end of the same window keeps the narrow fields"""
    rng = np.random.default_rng(108)
    root = rand_seq(rng, 1100)
    al, kinds = [], []
    for i in range(1060):
        m = i % 25
        k, kind = (110 + 8 * (i // 25 % 8), "far") if m == 7 else (100, "bound") if m == 11 else (i % 4, "near")
        al.append(sign(swap(root, [50 + 300 + 3 * j for j in range(k)]), i))
        kinds.append(kind)
    fa = write_fasta(str(tmp_path / "ref.fa"), al)
    reads = [root[50:1050], revcomp(root[50:1050]), root[900:1050]]
    orc = oracle_lists(fa, reads)
    far, bound = kinds.count("far"), kinds.count("bound")
    for o, s in orc[:2]:
        assert far > 30 and 1000 < len(o) == 1060 - far and s[0] == 1.0 and s.min() == 0.9 and int((s == 0.9).sum()) == bound
        assert int(o[:, 2].max()) == 999 and int(o[:, 6].max()) == 2000
    assert len(orc[2][0]) == 1060   # (every allele is perfect there: nothing to cut)
    stats = check(fa, reads, orc)
    assert stats[0]["extended"] == 3 * 1060


def test_through_the_job(built, tmp_path):
    """the executable on a sample whose lists are cut (two genes of 1200 alleles each, about 10 % apart: a read's overlaps on the other
    gene lie around 0.1 below its own), small ranges and windows: every output file is the same with deferred and with eager coverage"""
    geno = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
    ref = str(tmp_path / "ref.fa")
    util.synth_ref("ref-rna", ref, genes=2, scale=0.2, seed=41)
    pfx = str(tmp_path / "r")
    util.synth_reads(ref, pfx, pairs=2000, len=150, seed=8, sub=0.004)
    args = ["-f", ref, "-1", pfx + "_1.fq", "-2", pfx + "_2.fq", "-s", "0.8"]
    small = {"T1K_FIRST_WINDOW": "256", "T1K_WINDOW": "1024", "T1K_BATCH": "96", "T1K_PAIR_BATCH": "256", "T1K_PIPELINES": "1"}
    out = {}
    for tag, env in (("deferred", dict(small, T1K_DEBUG_PHASES="1")), ("eager", dict(small, T1K_COVERAGE="eager"))):
        out[tag] = str(tmp_path / tag)
        r = subprocess.run([geno] + args + ["-o", out[tag]], stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (tag, r.stderr[-500:])
        if tag == "deferred":  # the ranges' own account: overlaps emitted and kept
            import re
            acc = re.findall(r"packed selection: cand \d+ emitted (\d+) kept (\d+)", r.stderr)
            assert len(acc) > 10 and sum(int(e) for e, _ in acc) > sum(int(k) for _, k in acc) > 0, acc[:5]
    for suf in ("_genotype.tsv", "_allele.tsv", "_aligned_1.fa", "_aligned_2.fa"):
        assert open(out["deferred"] + suf, "rb").read() == open(out["eager"] + suf, "rb").read(), suf
    assert os.path.getsize(out["deferred"] + "_aligned_1.fa") > 100000
