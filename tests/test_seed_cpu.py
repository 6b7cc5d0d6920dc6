"""The look-up rule of seeding, stated three times and compared on the CPU (no GPU): tests/seed_ref.py (plain Python), Oracle::seedHits
(orc_seed_used) and the reference's own SeqSet::GetHitsFromRead (oracle/_ref/seed_harness, where it is built) -- on the designed cases
of tests/seed_cases.py and on seeded random reads.  And the proof that every designed case meets the edge it is named for, from the
list lengths of the oracle's index and the restatement's trace: tests/test_gpu_seed.py then holds the kernels to the same cases."""
import subprocess

import pytest

import seed_cases as sc
import seed_ref
import util

WORLDS = [(11, 3), (9, 0), (12, 0), (15, 0)]  # the genotyper's k and N; the extractors' N at k/2 + 1 = 5, 7, 8
_kept = {}


@pytest.fixture(scope="module")
def expect(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("seed"))

    def get(k, n_code):
        if (k, n_code) not in _kept:
            _kept[(k, n_code)] = sc.Expect(sc.World(k, n_code), d)
        return _kept[(k, n_code)]
    return get


def big(size):
    return size is not None and size >= seed_ref.BIG


def windows(read, k):
    return [read[p:p + k] for p in range(len(read) - k + 1)]


@pytest.mark.parametrize("k,n_code", WORLDS)
def test_list_lengths_are_the_construction(expect, k, n_code):
    """99 + the prefixes that hold the k-mer: 439 ... 101, 100, 99 along R1 (and along revcomp(R1)); exactly 99 over the variant's site;
    nothing big behind a root's end"""
    e = expect(k, n_code)
    w = e.w
    for root in (w.R1, seed_ref.revcomp(w.R1)):
        for p in range(sc.ROOT_LEN - k + 1):
            assert e.list_len(root[p:p + k]) == sc.COPIES + sum(1 for n in range(sc.PREFIX_MIN, sc.ROOT_LEN) if n >= p + k), p
    assert [e.list_len(w.R1[p:p + k]) for p in (w.T - 1, w.T, w.T + 1)] == [101, 100, 99]
    at = w.VAR_SITE - w.VAR_A
    for p in range(len(w.var_core) - k + 1):
        want99 = p <= at < p + k
        assert (e.list_len(w.var_core[p:p + k]) == 99) == want99 and (want99 or e.list_len(w.var_core[p:p + k]) >= 198), p
    for p in range(w.REP_END, w.T + 1):
        assert e.list_len(w.R2[p:p + k]) >= 100
    for s, en, d in w.spans2:
        assert all(e.list_len(x) >= 100 for x in windows(w.R2[s:en], k))
    for s, en, d in w.spans0:
        assert all(0 < e.list_len(x) < 100 for x in windows(w.B0[s:en], k))
    for tag in ("R1", "R2"):
        c = w.copy[tag]
        assert all(0 < e.list_len(c[p:p + k]) < 100 for p in range(w.T + 1, len(c) - k + 1))


def interruption(tr, first, last, kind):
    """positions first .. last of a strand's trace are all `kind` and the positions around them big; -> skipCnt on arrival"""
    assert all(t[0] == kind for t in tr[first:last + 1]), (kind, tr[first - 1:last + 2])
    assert big(tr[first - 1][1]) and big(tr[last + 1][1])
    return tr[first][2]


@pytest.mark.parametrize("k,n_code", WORLDS)
def test_every_case_hits_its_edge(expect, k, n_code):
    e = expect(k, n_code)
    w = e.w
    W, W1 = w.W, w.W1
    seen = {}

    def note(kind, v):
        seen.setdefault(kind, set()).add(v)

    required = ("threshold_interior", "threshold_replay", "threshold_first", "threshold_last", "ends", "broken_sub", "broken_n", "broken_sub2", "broken_99", "repeat", "n_homopolymer",
                "replay_segment", "scan", "long", "tiny")
    for kind in required:
        assert w.by_kind(kind), "no case of kind " + kind
    suppressed_after_skips = 0
    for c in w.cases:
        r = e.of(c.read)
        tr0, tr1 = r["trace"]
        m = c.meta
        if c.kind == "threshold_interior":
            at = m["at"]
            assert [t[1] for t in tr0[at - 1:at + 2]] == [101, 100, 99] and 0 < at < len(tr0) - 2, c.name
            assert tr0[at][2] == m["skip"] and tr0[at][0] == ("skip" if m["skip"] < W else "use") and tr0[at + 1][0] == "use", c.name
            note(c.kind, m["skip"])
        elif c.kind == "threshold_replay":
            at = m["at"]
            assert r["replay"] and [t[1] for t in tr0[at - 1:at + 2]] == [101, 100, 99] and 0 < at < len(tr0) - 2, c.name
            assert tr0[at][0] == ("skip" if tr0[at][2] < W else "use") and tr0[at + 1][0] == "use", c.name
            note(c.kind, tr0[at][2])
        elif c.kind == "threshold_first":
            assert tr0[0] == ("use", m["size"], 0), c.name
            note(c.kind, m["size"])
        elif c.kind == "threshold_last":
            assert tr0[-1][:2] == ("use", m["size"]) and all(big(t[1]) for t in tr0[:-1]), c.name
            note(c.kind, m["size"])
        elif c.kind == "ends":
            assert len(tr0) == m["nk"] == len(c.read) - k + 1 and all(big(t[1]) for t in tr0) and not r["replay"], c.name
            assert tr0[0][0] == "use" and tr0[-1][0] == "use"
            if "r2" not in c.name:  # big on both strands: the strand boundary interrupts the run
                assert all(big(t[1]) for t in tr1) and tr1[0][0] == "use" and tr1[-1][0] == "use", c.name
                note("strand_boundary", (m["nk"] - 1) % W1)
            else:
                assert all(t[1] == 0 for t in tr1), c.name
            note(c.kind, (m["nk"] - 1) % W1)
            note("ends_nk", m["nk"])
        elif c.kind in ("broken_sub", "broken_n"):
            x = m["x"]
            assert not r["replay"] or c.kind == "broken_n", c.name
            note(c.kind, interruption(tr0, x - k + 1, x, "empty"))
            assert ("N" in c.read) == (c.kind == "broken_n")
        elif c.kind == "broken_sub2":
            x, d = m["x"], m["d"]
            assert not r["replay"], c.name
            if d <= k:  # one empty stretch of k + d positions
                note((c.kind, d), interruption(tr0, x - k + 1, x + d, "empty"))
            else:       # two of k, d - k big positions between them
                note((c.kind, d), interruption(tr0, x - k + 1, x, "empty"))
                assert all(big(t[1]) for t in tr0[x + 1:x + d - k + 1]), c.name
                interruption(tr0, x + d - k + 1, x + d, "empty")
        elif c.kind == "broken_99":
            x = m["x"]
            assert all(t[1] == 99 for t in tr0[x - k + 1:x + 1]) and not r["replay"], c.name
            note(c.kind, interruption(tr0, x - k + 1, x, "use"))
        elif c.kind == "repeat":
            d = m["d"]
            assert r["replay"] == m["replay"] == (d <= W1), c.name
            for s in (c.read, seed_ref.revcomp(c.read)):
                ws = windows(s, k)
                dist = [j - i for i in range(len(ws)) for j in range(i + 1, min(len(ws), i + W1 + 3)) if ws[i] == ws[j]]
                assert dist and min(dist) == d, (c.name, dist)
            sizes = [t[1] for t in tr0 + tr1 if t[1] is not None]
            if m["where"] == "big":
                run = tr1 if c.name.endswith("_rc") else tr0
                assert all(t[0] == "same" or big(t[1]) for t in run[1:-1]), c.name
            else:
                assert max(sizes) < seed_ref.BIG and max(sizes) > 0, c.name
            note((c.kind, m["where"]), d)
            for tr, s in ((tr0, c.read), (tr1, seed_ref.revcomp(c.read))):  # a look-up suppressed by a k-mer further back than the one before
                ws = windows(s, k)
                suppressed_after_skips += sum(1 for p in range(1, len(tr)) if tr[p][0] == "same" and ws[p] != ws[p - 1] and tr[p - 1][0] == "skip")
        elif c.kind == "n_homopolymer":
            ws = windows(c.read, k)
            same_n = [p for p in range(len(ws)) if "N" in ws[p] and tr0[p][0] == "same"]
            assert c.read.count("N") == 1
            if m["where"] == "same" and not c.name.endswith("_before"):  # (before the run: the N is the window's first base only at the run's start)
                assert same_n, c.name
            if m["where"] == "other":
                assert not same_n, c.name
            note(c.kind, (m["where"], bool(same_n)))
        elif c.kind == "replay_segment":
            assert r["replay"] and len(tr0) == m["nk"], c.name
            if "both" in c.name:
                assert any(t[0] == "skip" for t in tr0) and any(t[0] == "skip" for t in tr1), c.name
            note(c.kind, m["nk"])
        elif c.kind == "scan":
            assert len(c.read) == 320 and not r["replay"] and len(tr0) == m["nk"], c.name
            comb = tr0 + tr1
            if "last_empty" in m:
                q = m["last_empty"]
                assert comb[q][0] == "empty" and comb[q + 1][0] != "empty" and big(comb[q + 1][1]), c.name
                assert sum(1 for t in comb if t[0] == "empty") == 2 * k
                note(c.kind, q)
            else:
                assert all(big(t[1]) for t in comb), c.name
                for edge in (191, 383, 575):  # the runs cross the wavefronts' edges, the last other position two wavefronts back
                    if edge + 1 < len(comb) - 1:
                        note("scan_edge", edge)
        elif c.kind == "long":
            assert len(c.read) > 320 and len(c.read) <= 450 and r["postings"] > 0, c.name
        elif c.kind == "tiny":
            assert len(c.read) <= k
        else:
            raise AssertionError("a case of a kind without a proof: " + c.kind)
    every = set(range(W1))
    assert seen["threshold_interior"] == every and seen["threshold_replay"] == every
    assert seen["threshold_first"] == seen["threshold_last"] == {101, 100, 99}
    assert seen["ends"] == every and seen["strand_boundary"] == every
    assert set(range(1, 15)) <= seen["ends_nk"] and set(range(150 - k + 1, 162 - k + 1)) <= seen["ends_nk"]
    for kind in ("broken_sub", "broken_n", "broken_99"):
        assert seen[kind] == every, kind
    ds = set(key[1] for key in seen if isinstance(key, tuple) and key[0] == "broken_sub2")
    assert len(ds) >= 5 and all(seen[("broken_sub2", d)] == every for d in ds)
    want_d = {1, 2, 3, 5, W1, W1 + 1}
    assert seen[("repeat", "big")] == want_d and seen[("repeat", "small")] == want_d
    assert suppressed_after_skips >= 1
    assert ("same", True) in seen["n_homopolymer"] and ("other", False) in seen["n_homopolymer"]
    assert seen["replay_segment"] == {63, 64, 65, 128, 129}
    if k == 11:
        assert seen["scan_edge"] == {191, 383, 575} and {190, 191, 192, 193, 383, 384, 385, 575, 576, 577} <= seen["scan"]
    shapes = dict(w.shapes())
    assert max(len(c.read) for c in shapes["nw5"]) <= 160 < max(len(c.read) for c in shapes["nw10"]) <= 320 < max(len(c.read) for c in shapes["xlong"]) <= 450
    for cs in shapes.values():
        assert any(len(c.read) < k for c in cs) and any(len(c.read) == k for c in cs)
        assert 0 < min(i for i, c in enumerate(cs) if c.kind == "tiny") and cs[-1].kind != "tiny"  # between the others


def check_against_oracle(e, reads):
    for r in reads:
        want = e.of(r)
        used, lookups, postings = e.orc.seed_used(r)
        assert used == e.flat(r), r
        assert (lookups, postings) == (want["lookups"], want["postings"]), r


@pytest.mark.parametrize("k,n_code", WORLDS)
def test_restatement_equals_the_oracle(expect, k, n_code):
    e = expect(k, n_code)
    reads = [c.read for c in e.w.cases] + e.w.random_reads(2000, 11)
    assert sum(1 for r in reads if "N" in r) > 300 and sum(1 for r in reads if e.of(r)["replay"]) > 300
    check_against_oracle(e, reads)


@pytest.mark.parametrize("k,n_code", WORLDS[:3])
def test_restatement_equals_the_reference(expect, k, n_code):
    """the reference's own GetHitsFromRead on its own index of the same file: the hit count (the sum of the used lists' lengths) and the
    distinct (strand, offset) pairs in order"""
    util.need(util.REF_SEED)
    e = expect(k, n_code)
    reads = [c.read for c in e.w.cases] + e.w.random_reads(2000, 11)
    p = subprocess.run([util.REF_SEED, e.fasta, str(k)] + (["0"] if n_code == 0 else []), input="\n".join(reads) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(reads)
    for r, line in zip(reads, lines):
        f = line.split()
        assert int(f[0]) == e.of(r)["postings"], r
        assert [tuple(int(x) for x in s.split(":")) for s in f[1:]] == [(s, o) for s, o, _ in e.flat(r)], r


def test_postings_fingerprint_the_used_positions(expect):
    """in the strictly decreasing stretch every list length is another, so the used set moved by one position sums to another number:
    `postings` alone tells a phase error of the (k/2 + 1) pattern"""
    e = expect(11, 3)
    n = 0
    for c in e.w.cases:
        if c.kind not in ("threshold_interior", "ends", "broken_sub", "broken_n", "broken_sub2", "scan") or "r2" in c.name:
            continue
        r = e.of(c.read)
        for by in (1, -1):
            s = seed_ref.shifted_postings(r, by)
            if s is not None:
                assert s != r["postings"], (c.name, by)
                n += 1
    assert n >= 100
