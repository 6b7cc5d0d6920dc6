"""The index of the reference, stated three times and compared on the CPU (no GPU): tests/refindex_ref.py (plain Python), the reference's
own KmerIndex::BuildIndexFromRead / Search (oracle/_ref/index_harness, where it is built) and the oracle's index (orc_kmer_postings) -- on
the designed cases of tests/refindex_cases.py.  And the proof that every designed case meets the edge it is named for, and that the
cases tell every wrong rule of refindex_ref.MUTATIONS from the right one: tests/test_gpu_refindex.py then holds the kernels to the
same cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refindex_cases as rc
import refindex_ref as rr
import util


def test_constants_come_from_the_header():
    c = rr.constants()
    assert c["T1K_DIR_MINLEN"] > 0 and c["T1K_SEED_CHUNK"] > 0 and c["T1K_SEED_CHUNK"] % 64 == 0 and c["T1K_NO_DIR"] == 0xFFFFFFFF


def test_codes_and_prefixes():
    """the device's order: first base in the lowest bits; the canonical prefix is read off the smaller code's text"""
    assert rr.encode("CA") == 1 and rr.encode("AC") == 4 and rr.decode(rr.encode("GATTACA"), 7) == "GATTACA"
    assert rr.revcomp("AACG") == "CGTT"
    k = 5
    for t in ("ACGTA", "TTTTT", "CCCCC", "GATTA"):
        c, r = rr.encode(t), rr.encode(rr.revcomp(t))
        assert rr.canonical_prefix(c, k) == min(c, r) % (1 << (2 * (k - 2)))  # (the kernel's form of the same thing)


def inserted(case, a):
    return [w[3] for w in rr.windows(case.seqs[a], case.k, case.n_code)]


def occurrences(case, text):
    return [(a, i) for a, s in enumerate(case.seqs) for i in range(len(s) - case.k + 1) if s[i:i + case.k] == text]


def chunk_counts(ix, code):
    return [sum(1 for a, _ in ix.list_of(code) if a // ix.CHUNK == c) for c in range(ix.stride - 1)]


def test_every_case_states_its_edge():
    kinds = set()
    for c in rc.all_cases():
        k, ix, m = c.k, c.ref(), c.meta
        kinds.add(c.kind)
        assert c.what
        if c.kind == "rule_all_a":
            assert c.seqs[0][:k + 2] == "A" * (k + 2) and inserted(c, 0)[:3] == [False, True, False], c.name
            assert ix.list_of(0) == [(0, 1)], c.name
        elif c.kind == "rule_homopolymer":
            for a, b in enumerate("ACGT"):
                assert len(c.seqs[a]) > 2 * k and set(c.seqs[a]) == {b}
                assert inserted(c, a) == ([False, True] if b == "A" else [True, True]) + [False] * (len(c.seqs[a]) - k - 1), c.name
            for a, b in enumerate("ACGT"):  # inside an allele: once
                s = c.seqs[4 + a]
                run = [i for i in range(len(s) - k + 1) if s[i:i + k] == b * k]
                assert len(run) > k and [inserted(c, 4 + a)[i] for i in run] == [True] + [False] * (len(run) - 1), c.name
        elif c.kind == "rule_tandem":
            for a, s in enumerate(c.seqs):
                assert all(inserted(c, a)) and len(ix.seen) < sum(len(s) - k + 1 for s in c.seqs), c.name
            assert any(len(l) > 3 and len({a for a, _ in l}) == 1 for l in ix.lists.values())
        elif c.kind == "rule_first_window":
            assert m["pal"] == m["pal"][::-1] and set(m["pal"]) == {"A", "C"}
            for a in range(5):
                assert c.seqs[a][:k] != "A" * k and inserted(c, a)[0], c.name
            assert {rr.encode(c.seqs[0][:k]), rr.encode(c.seqs[1][:k])} == {1, 1 << (2 * (k - 1))}
            assert inserted(c, 5) == [False] and inserted(c, 6) == [False, True]
        elif c.kind == "n_positions":
            assert [s.index("N") for s in c.seqs[:4]] == m["at"] and [s.count("N") for s in c.seqs] == [1, 1, 1, 1, 2, 2, 2]
            for a, s in enumerate(c.seqs):
                ws = rr.windows(s, k, c.n_code)
                assert all(w[2] == ("N" not in s[w[0]:w[0] + k]) for w in ws) and any(w[2] for w in ws) and any(not w[2] for w in ws), c.name
            assert ix.alleleHasN.all() and len(ix.sepPos) == 10
        elif c.kind == "n_then_same":
            o = m["n_at"] + 1
            for a, same in ((0, True), (1, False)):
                w = rr.windows(c.seqs[a], k, c.n_code)
                assert w[o][2] and not w[o - 1][2] and (w[o][1] == w[o - 1][1]) == same and w[o][3] == (not same), c.name
            for a in (2, 3):  # N at offset 0: the first valid window ends at i == k
                w = rr.windows(c.seqs[a], k, c.n_code)
                assert not w[0][2] and w[1][2] and w[1][3], c.name
            w = rr.windows(c.seqs[4], k, c.n_code)
            assert w[-1][2] and not w[-1][3] and w[-2][2] and not w[-2][3] and not w[-3][2], c.name  # (two Ns: no posting behind them at all)
        elif c.kind == "order_multi":
            l1, l2, l3 = (ix.list_of(rr.encode(m[x])) for x in ("m1", "m2", "m3"))
            assert [l1, l2, l3] == [occurrences(c, m[x]) for x in ("m1", "m2", "m3")], c.name
            assert [a for a, _ in l1] == [0, 0, 0, 1, 2] and [a for a, _ in l2] == [0, 1, 2, 2] and [a for a, _ in l3] == [0, 1, 2], c.name
            assert sorted(l1, key=lambda p: (p[1], p[0])) != l1
            assert rr.encode(m["m1"]) in ix.multi and rr.encode(m["m2"]) in ix.multi and rr.encode(m["m3"]) not in ix.multi
        elif c.kind == "lengths":
            assert set(m["lens"]) <= {len(s) for s in c.seqs} and m["lens"] == [0, 1, k - 1, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65, 96]
            for a, s in enumerate(c.seqs):
                words = (int(ix.alleleOff[a + 1]) if a + 1 < len(c.seqs) else ix.totalBases - 64) - int(ix.alleleOff[a])
                assert words == (len(s) // 32 + 1) * 32, c.name
            assert sorted(p for l in ix.lists.values() for p in l) == [(a, o) for a, s in enumerate(c.seqs) for o in range(len(s) - k + 1)]  # (random text: every window)
            assert any(len(s) % 32 == 0 and len(s) and len(c.seqs[a + 1]) >= k for a, s in enumerate(c.seqs[:-1]))
            assert ix.exon.any()
        elif c.kind == "other_letters":
            assert not c.vs_reference and all(len(set(s) - set("ACGT")) == 1 and "N" not in s for s in c.seqs)
            assert ix.alleleHasN.all() and len(ix.sepPos) == len(c.seqs)
            w = rr.windows(c.seqs[-1], k, c.n_code)
            assert w[7][2] and not w[7][3] and w[7][1] == w[6][1]
        elif c.kind == "straddle":
            assert all(inserted(c, 0)) and len(c.seqs[0]) - k + 1 >= 64  # every in-word start, every split
            bit = lambda a, p: (int(ix.posted[(int(ix.alleleOff[a]) + p) >> 5]) >> (2 * (p & 31))) & 1
            assert [(bit(a, 31), bit(a, 32)) for a in (0, 1, 2)] == [(1, 1), (1, 0), (0, 1)], c.name
            nb = lambda a, p: (int(ix.nmask[(int(ix.alleleOff[a]) + p) >> 5]) >> (2 * (p & 31))) & 1
            assert nb(2, 31) and nb(3, 32) and nb(4, 63) and nb(4, 64) and nb(5, 31) and nb(5, 32)
            assert c.slices == (k == 15)
        elif c.kind == "haspre":
            enc = rr.encode
            assert enc(rr.revcomp(m["rc_one"])) < enc(m["rc_one"]) and rr.canonical_prefix(enc(m["rc_one"]), k) in ix.pre
            assert rr.canonical_prefix(enc(m["rc_one"]), k) == enc(rr.revcomp(m["rc_one"])[:k - 2])
            assert m["t1"][:k - 2] == m["t2"][:k - 2] and rr.canonical_prefix(enc(m["t1"]), k) == rr.canonical_prefix(enc(m["t2"]), k) == enc(m["t1"][:k - 2])
            assert enc(m["t1"]) in ix.lists and enc(m["t2"]) in ix.lists
            assert enc(m["absent"]) not in ix.lists and enc(rr.revcomp(m["absent"])) not in ix.lists and rr.canonical_prefix(enc(m["absent"]), k) not in ix.pre
        elif c.kind == "dir_32_33":
            assert len(ix.list_of(rr.encode(m["m32"]))) == 32 == ix.MINLEN and len(ix.list_of(rr.encode(m["m33"]))) == 33
            assert ix.rowCodes == [rr.encode(m["m33"])] and ix.dir_idx(rr.encode(m["m32"])) == ix.NO_DIR
        elif c.kind.startswith("dir_A"):
            A, ca, cb = m["A"], rr.encode(m["ma"]), rr.encode(m["mb"])
            assert len(c.seqs) == A and sorted(ix.rowCodes) == sorted([ca, cb]) and ix.stride == (A + 511) // 512 + 1
            assert [a for a, _ in ix.list_of(ca)] == m["la"] and [a for a, _ in ix.list_of(cb)] == m["lb"]
            want = {511: [33], 512: [33], 513: [32, 1], 1025: [32, 0, 1]}[A]
            assert chunk_counts(ix, ca) == want, c.name
            row = ix.kDir[ix.rowOf[ca] * ix.stride:(ix.rowOf[ca] + 1) * ix.stride].tolist()
            assert row == [0] + list(np.cumsum(want)), c.name
            assert int(ix.kDirMask[ix.rowOf[ca]]) == sum(1 << i for i, n in enumerate(want) if n) and int(ix.kDirMask[ix.rowOf[cb]]) == 1
        elif c.kind == "dir_last_chunk":
            code = rr.encode(m["ml"])
            assert ix.rowCodes == [code] and chunk_counts(ix, code) == [0, 40] and ix.kDir.tolist() == [0, 0, 40] and ix.kDirMask.tolist() == [2]
        elif c.kind == "dir_two_mask_words":
            code = rr.encode(m["m"])
            assert len(c.seqs) == 64 * 512 + 1 == m["A"] and all(len(s) == k + 1 for s in c.seqs[:-1])
            assert ix.maskWords == 2 and ix.stride == 66 and ix.rowCodes == [code] and ix.list_of(code) == [(m["A"] - 1, 12 * i) for i in range(33)]
            assert ix.kDirMask.tolist() == [0, 1] and ix.kDir.tolist() == [0] * 65 + [33]
        elif c.kind.startswith("transpose_A"):
            A = m["A"]
            assert len(c.seqs) == A and len({len(s) for s in c.seqs}) > 5 and ix.hasT and len(ix.blockT) == (A + 63) // 64
            if A >= 64:
                assert len(c.seqs[63]) == max(len(s) for s in c.seqs[:64])
            for a, s in enumerate(c.seqs):  # the column of allele a: its words, then zeros to the block's end
                b = a >> 6
                end = int(ix.blockT[b + 1]) if b + 1 < len(ix.blockT) else len(ix.basesT) - 512
                col = ix.basesT[int(ix.blockT[b]) + (a & 63):end:64]
                nw = (len(s) + 31) // 32
                assert np.array_equal(col[:nw], ix.bases[int(ix.alleleOff[a]) // 32:int(ix.alleleOff[a]) // 32 + nw]) and not col[nw:].any() and len(col) >= nw + 2, (c.name, a)
            if A % 64:
                end = len(ix.basesT) - 512
                assert all(not ix.basesT[int(ix.blockT[-1]) + j:end:64].any() for j in range(A % 64, 64)), c.name
            assert not ix.basesT[-512:].any()
        elif c.kind == "transpose_off":
            on = rc.get("transpose_A65_k11_n3").ref()
            assert not ix.hasT and len(ix.basesT) == 0 and c.seqs == rc.get("transpose_A65_k11_n3").seqs
            assert all(np.array_equal(v, on.small()[n]) for n, v in ix.small().items() if n not in ("basesT", "blockT"))
        else:
            raise AssertionError("a case of a kind without a proof: " + c.kind)
    assert len(kinds) == 23, sorted(kinds)
    ks = {(c.k, c.n_code) for c in rc.all_cases() if c.vs_reference}
    assert ks == set(rc.RULE_WORLDS) and any(c.k == 15 and c.slices for c in rc.all_cases())


# the designed case that tells each wrong rule from the right one
CAUGHT_BY = {
    "no_i_eq_k": "rule_all_a_k11_n3",
    "prev_if_valid": "n_then_same_k11_n3",
    "first_vs_nothing": "rule_all_a_k11_n3",
    "sort_offset_first": "order_multi_k11_n3",
    "dir_bound_le": "dir_A1025_k11_n3",
    "mask_no_guard": "dir_A513_k11_n3",
    "multi_first_two": "order_multi_k11_n3",
    "n_ignored_last_base": "n_positions_k11_n3",
}


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_every_wrong_rule_is_caught(mutation):
    assert set(CAUGHT_BY) == set(rr.MUTATIONS)
    c = rc.get(CAUGHT_BY[mutation])
    good, bad = c.ref().fingerprint(), c.ref(mutation).fingerprint()
    differ = [n for n in good if good[n] != bad[n]]
    assert differ, "%s is not caught by %s" % (mutation, c.name)
    if mutation in ("no_i_eq_k", "prev_if_valid", "first_vs_nothing", "n_ignored_last_base"):
        assert "lists" in differ and "posted" in differ
    elif mutation == "sort_offset_first":
        assert "kPost" in differ and "posted" not in differ
    elif mutation == "dir_bound_le":
        assert differ == ["kDir", "kDirMask"] or differ == ["kDir"]
    elif mutation == "mask_no_guard":
        assert differ == ["kDirMask"]
    elif mutation == "multi_first_two":
        assert differ == ["multi"]


def test_rule_mutations_are_caught_in_every_world():
    """the rule, N and order cases do their work at every k and N code they exist for"""
    for k, n in rc.RULE_WORLDS:
        for mutation, name in CAUGHT_BY.items():
            if name.endswith("_k11_n3") and not name.startswith("dir_"):
                c = rc.get(name[:-len("_k11_n3")] + "_k%d_n%d" % (k, n))
                assert c.ref().fingerprint() != c.ref(mutation).fingerprint(), (mutation, c.name)


@pytest.fixture(scope="module")
def index_harness(built):
    """oracle/_ref/index_harness is younger than the other reference-built checkers: a tree whose oracle/_ref was built before it existed
    passes `built` without it, so the build (which makes oracle/_ref again where the reference's sources lie and a binary is missing) is
    asked for here"""
    if not os.path.exists(util.REF_INDEX):
        import __graft_entry__
        __graft_entry__.build()
    return util.REF_INDEX


def probe_texts(c, extra=6):
    """the text of every code that occurs in a window of the case, valid or not, and a handful of absent ones"""
    ix = c.ref()
    codes = sorted(ix.seen)
    n, x = 1 << (2 * c.k), 12345
    while extra:
        x = (x * 1103515245 + 12345) % n
        if x not in ix.seen:
            codes.append(x)
            extra -= 1
    return codes, [rr.decode(code, c.k) for code in codes]


@pytest.mark.parametrize("k,n_code", rc.RULE_WORLDS)
def test_restatement_equals_the_reference(index_harness, tmp_path, k, n_code):
    """KmerIndex::BuildIndexFromRead + Search of the reference itself: every list, posting for posting, in list order"""
    util.need(util.REF_INDEX)  # (decided when the test runs, after the fixtures had their chance to build oracle/_ref)
    cases = [c for c in rc.all_cases() if c.vs_reference and (c.k, c.n_code) == (k, n_code)]
    assert {c.group for c in cases} == {"rule", "n", "order"} and len(cases) == 7
    for c in cases:
        codes, texts = probe_texts(c)
        sf, kf = str(tmp_path / (c.name + ".seqs")), str(tmp_path / (c.name + ".kmers"))
        open(sf, "w").write("".join(s + "\n" for s in c.seqs))
        open(kf, "w").write("".join(t + "\n" for t in texts))
        p = subprocess.run([util.REF_INDEX, sf, kf, str(k)] + (["0"] if n_code == 0 else []), stdout=subprocess.PIPE, text=True, check=True)
        lines = p.stdout.split("\n")[:-1]
        assert len(lines) == len(codes)
        n_lists = 0
        for code, text, line in zip(codes, texts, lines):
            got = [tuple(int(x) for x in f.split(":")) for f in line.split()]
            assert got == c.ref().list_of(code), "%s: the list of %s" % (c.name, text)
            n_lists += bool(got)
        assert n_lists == len(c.ref().lists) > 0


@pytest.mark.parametrize("k,n_code", [(9, 0), (11, 0), (12, 0), (11, 3)])
def test_restatement_agrees_with_the_oracle(built, tmp_path, k, n_code):
    """the oracle's index (orc_kmer_postings): list lengths and the alleles in list order.  N coded as A: the extractors' loader at any k;
    N coded as T: the genotyper's, which exists at k = 11"""
    for c in [c for c in rc.all_cases() if c.vs_reference and (c.k, c.n_code) == (k, n_code)]:
        fa = str(tmp_path / (c.name + ".fa"))
        open(fa, "w").write("".join(">G*01:%02d\n%s\n" % (a + 1, s) for a, s in enumerate(c.seqs)))
        orc = util.Oracle(fa) if n_code == 3 else util.ExtractOracle(fa, k=k, hit_len_required=k)
        orc.L.orc_kmer_postings.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
        if n_code == 3:
            assert orc.n_alleles == len(c.seqs), c.name
        codes, texts = probe_texts(c)
        buf = np.zeros(4096, np.int32)
        for code, text in zip(codes, texts):
            n = orc.L.orc_kmer_postings(orc.h, text.encode(), buf.ctypes.data, len(buf))
            want = c.ref().list_of(code)
            assert n == len(want) and buf[:n].tolist() == [a for a, _ in want], "%s: the list of %s" % (c.name, text)
        orc.L.orc_destroy(orc.h)
        orc.h = None
