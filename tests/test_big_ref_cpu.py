"""The designed references of tests/big_ref_cases.py hit the edges they are named for -- proved without a GPU, from the oracle's index
(orc_kmer_postings: the posting lists KmerIndex's insert rule makes, as oracle_core.cpp:buildIndex restates it) and from the oracle's
overlap lists.  Which code the device runs is a function of the number of sequences A, the lengths of the posting lists a read uses
and the read's length, so these conditions stand in for a route report of the GPU tests in tests/test_gpu_big_ref.py."""
import ctypes as C
import time

import numpy as np
import pytest

import big_ref_cases as B
import util

SIM = 0.9


def postings(orc, kmer, cap=20000):
    out = np.zeros(cap, dtype=np.int32)
    orc.L.orc_kmer_postings.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
    n = orc.L.orc_kmer_postings(orc.h, kmer.encode(), out.ctypes.data, cap)
    assert 0 <= n <= cap, (kmer, n)
    return out[:n]


def kmers(s):
    return [s[i:i + B.K] for i in range(len(s) - B.K + 1)]


class Loaded:
    def __init__(self, A, tmp):
        self.case = B.make_case(A)
        self.fa = B.write_fasta(str(tmp / ("ref%d.fa" % A)), self.case)
        self.orc = util.Oracle(self.fa, similarity=SIM)
        self.reads = B.designed_reads(self.case)
        self.lists = {label: self.orc.assign_read(read) for label, read in self.reads}
        self.read = dict(self.reads)


@pytest.fixture(scope="module")
def loaded(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bigref")
    return {A: Loaded(A, tmp) for A in B.CASES}


def holding(loaded, name):
    got = [l for l in loaded.values() if name in l.case["families"]]
    assert got, name
    return got


def test_regimes_by_size():
    """the size-keyed branches each case is on, restated from the code: seeding chunks of 512 alleles, 64-bit directory mask words, the
    two all-allele bitmaps inside the accumulators while 2 * ceil(A / 32) <= 512 * AW (AW = 7 up to 160 bases, 13 up to 320), allele bits"""
    want = {32768: (64, 1, True, True, 15), 32769: (65, 2, True, True, 16), 33300: (66, 2, True, True, 16), 57344: (112, 2, True, True, 16),
            57345: (113, 2, False, True, 16), 66200: (130, 3, False, True, 17), 106496: (208, 4, False, True, 17),
            106497: (209, 4, False, False, 17), 131072: (256, 4, False, False, 17)}
    assert set(want) == set(B.CASES)
    for A, w in want.items():
        chunks = (A + B.CHUNK - 1) // B.CHUNK
        words = 2 * ((A + 31) // 32)
        bits = max(1, int(A - 1).bit_length())
        assert (chunks, (chunks + 63) // 64, words <= 512 * 7, words <= 512 * 13, bits) == w, A
    assert (131073 + B.CHUNK - 1) // B.CHUNK == 257   # the refused size: one chunk more than the 256 the hot-chunk words hold


def test_sequences_distinct_and_in_place(loaded):
    """nothing collapses on loading, so every family lies at the allele indices of the plan"""
    for A, l in loaded.items():
        seqs = l.case["seqs"]
        assert len(seqs) == A == len(set(seqs)) == l.orc.n_alleles
        for name, (first, m, L) in l.case["families"].items():
            assert first + m <= A and all(len(s) == L for s in seqs[first:first + m])
            o, _ = l.lists[name + "/fwd"]
            assert name in ("low", "paralog") or (first <= o[:, 0].min() and o[:, 0].max() < first + m)   # (those two: test_paralog)
    assert sorted(loaded[33300].case["families"]) == ["last_partial", "long320", "low", "small64", "straddle64", "xlong"]
    assert set(loaded[66200].case["families"]) >= {"paralog", "tie1200", "tie2100", "small128"}
    assert set(loaded[131072].case["families"]) >= {"small255", "last_full", "long320_top"} and "last_partial" in loaded[106497].case["families"]
    assert "last_full" in loaded[32768].case["families"] and "last_partial" in loaded[32769].case["families"]


def test_straddle64(loaded):
    """the first and the last k-mer of the read (always used: the skipping of long lists starts behind the first) have lists longer
    than T1K_DIR_MINLEN with postings below and from allele 32 768 on: chunks 63 and 64 of one directory row.  In the 32 769 case the
    last family does the same with a single allele in chunk 64"""
    for l in holding(loaded, "straddle64") + [loaded[32769]]:
        name = "straddle64" if "straddle64" in l.case["families"] else "last_partial"
        for label in (name + "/fwd", name + "/rc"):
            own = l.read[label] if label.endswith("/fwd") else B.revcomp(l.read[label])   # the strand that lies in the reference
            for km in (kmers(own)[0], kmers(own)[-1]):
                p = postings(l.orc, km)
                assert len(p) > B.DIR_MINLEN and p.min() < 32768 <= p.max() and np.all(np.diff(p) >= 0), (l.case["A"], label, len(p))
                assert p.min() // B.CHUNK == 63 and p.max() // B.CHUNK == 64
    assert loaded[32769].case["families"]["last_partial"][0] + 300 == 32769


@pytest.mark.parametrize("name,chunk", [("small64", 64), ("small128", 128), ("small255", 255)])
def test_small_high(loaded, name, chunk):
    """every k-mer of the read, on either strand, has a list of at most T1K_DIR_MINLEN postings (no directory row: the chunk is found by
    the third sighting alone), an allele of the family collects three postings and more, and the family lies in the chunk whose bit is
    in word 2, 4 and 7 of the hot-chunk words"""
    for l in holding(loaded, name):
        first, m, L = l.case["families"][name]
        assert first // B.CHUNK == chunk == (first + m - 1) // B.CHUNK and m <= B.DIR_MINLEN
        for label in ("fwd", "rc", "sub", "del"):
            read = l.read[name + "/" + label]
            per_allele = {}
            for strand in (read, B.revcomp(read)):
                for km in kmers(strand):
                    p = postings(l.orc, km)
                    assert len(p) <= B.DIR_MINLEN, (label, km, len(p))
                    for a in p.tolist():
                        per_allele[(strand is read, a)] = per_allele.get((strand is read, a), 0) + 1
            assert set(a for _, a in per_allele) <= set(range(first, first + m))
            assert max(per_allele.values()) >= 3 and len(l.lists[name + "/" + label][0]) == m


def test_paralog(loaded):
    """a read of the low family overlaps that family and its copy beyond 65 536: alleles with bit 16 clear and set in one list"""
    for l in holding(loaded, "paralog"):
        (lo, m, _), (hi, _, _) = l.case["families"]["low"], l.case["families"]["paralog"]
        assert lo + m < 1000 and hi >= 65536
        for label in ("low/fwd", "low/rc", "paralog/fwd", "paralog/sub", "low/del"):
            o, s = l.lists[label]
            al = o[:, 0]
            assert int((al < 65536).sum()) == m == int((al >= 65536).sum()), label
            assert 0.9 <= s.min() < 0.93 and s.max() > 0.97


def test_ties(loaded):
    """all members of a tie family are in the list with equal match count, spans and similarity, so the allele alone orders them:
    ascending, for tie1200 across 65 536 (1 200 candidates: the 1001 .. 2048 size class; 2 100: the class beyond)"""
    for name, n in (("tie1200", 1200), ("tie2100", 2100)):
        for l in holding(loaded, name):
            first, m, _ = l.case["families"][name]
            assert m == n
            for label in ("fwd", "rc", "sub", "del"):
                o, s = l.lists[name + "/" + label]
                assert len(o) == n and o[:, 0].tolist() == list(range(first, first + n)), (name, label, len(o))
                assert len(set(map(tuple, o[:, 1:10].tolist()))) == 1 and len(set(s.tolist())) == 1
    first = loaded[66200].case["families"]["tie1200"][0]
    assert first < 65536 < first + 1200 - 1


def test_candidate_counts_stay_below_the_sort_capacity(loaded):
    """a read-end with 16 384 candidates or more is refused (ERR_SORTCAP): the cases must test the sort, not the refusal.  The distinct
    alleles among the postings of all k-mers of a read, both strands, bound its candidates from above"""
    worst = 0
    for l in loaded.values():
        for label, read in l.reads:
            if label.startswith("bg/"):
                continue
            n = 0
            for strand in (read, B.revcomp(read)):
                ks = set(kmers(strand))
                n += len(set(np.concatenate([postings(l.orc, km) for km in ks] or [np.zeros(0, np.int32)]).tolist()))
            worst = max(worst, n)
            assert n < 16384, (l.case["A"], label, n)
    assert worst >= 2100


def test_every_designed_read_has_a_list(loaded):
    for l in loaded.values():
        for label, _ in l.reads:
            o, _ = l.lists[label]
            assert (len(o) == 0) == label.startswith("none/"), (l.case["A"], label, len(o))
        labels = [label for label, _ in l.reads]
        assert len(set(labels)) == len(labels) and sum(1 for x in labels if x.startswith("bg/")) == 40
        if l.case["A"] > 33000:
            assert sum(1 for x in labels if x.startswith("bg/") and int(x[3:]) >= 32768) >= 20


def test_read_lengths_choose_the_kernels(loaded):
    """short reads (<= 150 bases: the narrow seeding kernel when a batch holds only them), long320 reads of 200 .. 320 bases (the wide
    one), xlong reads of about 400 (k_seed_long)"""
    for l in loaded.values():
        lens = {label: len(r) for label, r in l.reads}
        for label, n in lens.items():
            fam = label.split("/")[0]
            if fam.startswith("long320"):
                assert 200 <= n <= 320, (label, n)
            elif fam == "xlong":
                assert 320 < n <= 400
            else:
                assert n <= 150
        assert len(B.short_reads(l.reads)) + len(B.long_reads(l.reads)) + sum(1 for x in lens if x.startswith("xlong/")) == len(l.reads)
    assert sorted(len(r) for x, r in loaded[131072].reads if x.startswith("long320_top/")) == [200, 260, 320, 320]


def test_pair_mates(loaded):
    """the pairing test's mates: both lists of the first fragment hold the low family and its paralog (an allele span above 65 000),
    both lists of the second all of tie1200"""
    l = loaded[66200]
    (la, a1, a2), (lb, b1, b2) = B.pair_mates(l.case)
    for r in (a1, a2):
        al = l.orc.assign_read(r)[0][:, 0]
        assert al.min() < 1000 and al.max() >= 65536 and len(al) == 600, (la, len(al))
    first = l.case["families"]["tie1200"][0]
    for r in (b1, b2):
        assert l.orc.assign_read(r)[0][:, 0].tolist() == list(range(first, first + 1200)), lb


def test_the_largest_case_is_made_and_loaded_quickly(tmp_path):
    """generating, writing and loading the 131 072 case: 1.7 s measured (0.25 s generating, 0.1 s writing, 1.3 s loading); under 10 s"""
    t0 = time.time()
    case = B.make_case(131072)
    orc = util.Oracle(B.write_fasta(str(tmp_path / "ref.fa"), case), similarity=SIM)
    dt = time.time() - t0
    assert orc.n_alleles == 131072 and dt < 10, dt
