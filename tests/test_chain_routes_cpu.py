"""The designed inputs of tests/chain_routes_cases.py are what they claim to be (no GPU): the preconditions that make the plain count of
equal k-mer pairs a group's hit count hold, the count is the one the case names, the predicates of the chain stage put the target
group where the case says, and the oracle gives the target read an overlap (so that equality with the oracle on the GPU is not
vacuous)."""
import os

import pytest

import chain_routes_cases as cc
import util

CASES = cc.all_cases()


@pytest.fixture(scope="module")
def oracle_counts(built, tmp_path_factory):
    """overlaps the oracle gives each case's read, computed once"""
    d = tmp_path_factory.mktemp("routes")
    out = {}
    for c in CASES:
        fa = cc.write_fasta(c, os.path.join(str(d), c.name + ".fa"))
        orc = util.Oracle(fa, similarity=0.8)
        out[c.name] = len(orc.assign_read(c.read)[0])
    return out


def test_registry_is_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for nw in (5, 10):
        for stem in ("closed_form", "gap_walk_finish", "gap_walk_retry", "simple_n3", "simple_n96", "simple_n97", "three_diag_n32", "three_diag_n33", "near_count_30",
                     "near_count_31", "text_start", "text_end", "scratch_lane", "scratch_wave", "gap_job", "short_repeat", "tandem_le32", "tandem_gt32", "tandem_le512", "tandem_gt512",
                     "tandem_le4096", "tandem_gt4096") + tuple("indel_%s%d" % (k, d) for k in "DI" for d in (1, 4, 5, 10, 11)):
            assert "%s_nw%d" % (stem, nw) in names
    # (16384 is within reach of the long class only: see chain_routes_cases.TANDEM)
    assert "tandem_le16384_nw10" in names and "tandem_gt16384_nw10" in names and "many_diagonals_nw5" in names


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_is_what_it_claims(c, oracle_counts):
    longest, repeat = cc.preconditions(c.alleles, [c.read])
    p = cc.predict(c.read, c.alleles, c.target, c.nw)
    print("%s: read of %d bases, n %d (near %s far %s), longest posting list %d, nearest repeat %d, oracle overlaps %d"
          % (c.name, len(c.read), p["n"], p.get("near"), p.get("far"), longest, repeat, oracle_counts[c.name]))
    assert len(c.alleles) <= 6 and max(len(s) for s in c.alleles) <= (4700 if c.threshold and c.threshold[0] == 4096 else 3100)  # (27 copies of a 160-mer)
    assert (len(c.read) <= 160) == (c.nw == 5) and len(c.read) <= 320
    if c.n is None:  # the short-repeat read: n is not predicted, the sequential replay of seeding is what it is for
        assert repeat <= 6 and c.route is None
    else:
        assert longest < 100 and repeat > 6
        assert p["n"] == c.n
        if c.single:
            assert not p["multi"]
        else:
            # multi-diagonal whichever diagonal seeding takes as the reference; the claim is the outcome for the fullest one
            assert p["multi"] and p["always_multi"] and p["near_done"] == c.near_done and p["simple"] == c.simple
            if c.route == "capacity":
                assert c.n > cc.BIG_CAP
            elif c.route == "candidate_cap":
                assert p["route"] == "wave_large" and len(set(a - b for a, b in cc.hit_pairs(c.read, c.alleles[c.target]))) > 32
            elif c.scratch:
                assert c.route == "big_by_scratch" and p["route"] in ("general_lane", "wave_small") and c.n <= cc.WAVE_CAP
            else:
                assert p["route"] == c.route
        if c.threshold:
            thr, side = c.threshold
            # (the search found T and T + 1 for every pair; the issue's bound is the copy count)
            assert (c.n <= thr) == (side == "le") and abs(c.n - thr) <= c.copies
            assert c.n == (thr if side == "le" else thr + 1)
        if c.route and c.route not in ("capacity", "candidate_cap"):
            # the claim must not depend on which diagonal seeding makes the reference one (the first hit to arrive decides); only the
            # two-diagonal chains of more than 96 hits cannot be built that way, and there the claim is one of two outcomes
            claim = (p["route"] if c.scratch else c.route, c.near_done, c.simple)
            if c.asymmetric:
                assert claim in p["admissible"] and len(p["admissible"]) == 2
            else:
                assert p["admissible"] == {claim}
    assert (oracle_counts[c.name] == 0) == c.expect_none
