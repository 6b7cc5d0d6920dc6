"""Every route out of t1k_run_chain, on the designed inputs of tests/chain_routes_cases.py: the overlap lists and the per-base coverage
against the oracle, and the route report (Context.route_report) against what the case's construction predicts -- which kernel chained
the target group, whether k_near_hits wrote its hit list, whether it was marked a two-diagonal chain, and its hit count.

Run as a program (`python tests/test_gpu_chain_routes.py OUT.npz DIR`) it assigns every case once and stores the lists and reports:
test_without_simple_chains starts it as a fresh child with T1K_NO_SIMPLE_CHAIN=1, which the library reads once per process."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_routes_cases as cc  # noqa: E402
import util  # noqa: E402
import t1k_amd  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cc.all_cases()
RUNS = [c for c in CASES if c.route not in ("capacity", "candidate_cap") and not c.heavy]
TOTALS = ("groups", "fast", "slow", "jobs", "retry", "finish", "general", "wave", "genjobs", "big", "eq", "band", "wide", "extjobs", "extretry")
FIELDS = ("seq_idx", "read_start", "read_end", "seq_start", "seq_end", "strand", "match_cnt", "left_clip", "right_clip", "relaxed_match_cnt")


def long_read(c):
    """a read beyond 320 bases (the range becomes an xlong one: k_seed_long seeds it, k_near_hits does not run)"""
    return c.alleles[0][10:10 + 340]


def assign(c, fasta, reads):
    """(counts, overlaps, coverage, totals, records) of one t1k_assign_batch over `reads` with the route report on"""
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(fasta)
    assert list(seqs) == list(c.alleles)
    ctx = t1k_amd.Context(ref_seq_similarity=0.8)
    try:
        ctx.route_report_enable()
        ctx.ref_upload(seqs, masks)
        ctx.reads_upload(reads)
        ctx.assign()
        counts, ovl = ctx.overlaps()
        cov = ctx.coverage()
        totals, recs = ctx.route_report()
    finally:
        ctx.close()
    return counts, ovl, cov, totals, recs


def oracle_lists(c, fasta, reads):
    orc = util.Oracle(fasta, similarity=0.8)
    lists = [orc.assign_read(r) for r in reads]
    cov = np.concatenate([orc.coverage(a, len(s)) for a, s in enumerate(c.alleles)])
    return lists, cov


def same_lists(lists, counts, ovl, what):
    """the fields gpu_assign_check.compare compares"""
    pos = 0
    for i, (o, s) in enumerate(lists):
        g = ovl[pos:pos + counts[i]]
        pos += counts[i]
        assert len(o) == len(g), "%s read %d: oracle %d overlaps, GPU %d" % (what, i, len(o), len(g))
        for k, f in enumerate(FIELDS):
            assert np.array_equal(o[:, k], g[f]), "%s read %d: %s differs: oracle %s GPU %s" % (what, i, f, o[:, k][:8], g[f][:8])
        assert np.array_equal(s, g["similarity"]), "%s read %d: similarity differs" % (what, i)


def target_of(c, recs, read_end=0):
    return recs[(recs["read_end"] == read_end) & (recs["strand"] == 0) & (recs["allele"] == c.target)]


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    """every case assigned once, alone and with a long read behind it, and the oracle's answer to both: computed once, read by all tests"""
    d = str(tmp_path_factory.mktemp("routes"))
    w = {}
    for c in RUNS:
        fa = cc.write_fasta(c, os.path.join(d, c.name + ".fa"))
        t0 = time.time()
        w[c.name] = dict(fasta=fa, gpu=assign(c, fa, [c.read]), orc=oracle_lists(c, fa, [c.read]), gpu_long=assign(c, fa, [c.read, long_read(c)]),
                         orc_long=oracle_lists(c, fa, [c.read, long_read(c)]))
        print("%s: %.2f s" % (c.name, time.time() - t0))
    return w


@pytest.mark.parametrize("c", RUNS, ids=[c.name for c in RUNS])
def test_lists_and_coverage_equal_the_oracle(world, c):
    counts, ovl, cov, _, _ = world[c.name]["gpu"]
    lists, ocov = world[c.name]["orc"]
    assert (len(lists[0][0]) == 0) == c.expect_none  # (equality with an empty list only where the case says so)
    same_lists(lists, counts, ovl, c.name)
    assert np.array_equal(ocov, cov), "%s: coverage differs at %s" % (c.name, np.nonzero(ocov != cov)[0][:8])


@pytest.mark.parametrize("c", RUNS, ids=[c.name for c in RUNS])
def test_route_of_the_target_group(world, c):
    _, _, _, totals, recs = world[c.name]["gpu"]
    t = target_of(c, recs)
    print("%s: totals %s; target %s" % (c.name, {k: totals[k] for k in TOTALS}, t))
    assert totals["ranges"] == 1 and totals["ranges_nw%d" % c.nw] == 1 and totals["ranges_xlong"] == 0
    assert totals["general"] == len(recs) and np.all(recs["nw"] == c.nw) and np.all(recs["xlong"] == 0)
    if c.single:  # one diagonal: not a multi-diagonal group, and the list the case names is not empty
        assert len(t) == 0 and totals[c.single] >= 1
        return
    if c.n is None:  # the short-repeat read: only the oracle comparison applies
        return
    assert len(t) == 1
    t = t[0]
    got = (t1k_amd.ROUTE_NAMES[t["route"]], bool(t["near_done"]), bool(t["simple"]))
    claim = (c.route, c.near_done, c.simple)
    print("claimed %s, reported %s" % (claim, got))
    if c.asymmetric:
        # more than 96 hits in a two-diagonal chain put more than 30 on one diagonal: if seeding's first hit (the reference diagonal) is on the
        # other one the near count saturates and k_gather_general writes the list.  Either outcome is right here;
        # test_every_route_is_reached asks that the claimed one occurred
        adm = cc.predict(c.read, c.alleles, c.target, c.nw)["admissible"]
        if c.scratch:
            adm = set(("big_by_scratch", nd, s) for _, nd, s in adm)
        assert claim in adm and got in adm
    else:
        assert got == claim
    if c.route == "big_by_size":
        assert t["n"] == 0xFFFFFFFF and c.n > cc.WAVE_CAP  # (k_gather_general hands the group on without keeping its count)
    else:
        assert t["n"] == c.n
    if c.route in ("big_by_size", "big_by_scratch"):
        assert totals["big"] >= 1
    if c.route in ("wave_small", "wave_large") or (c.scratch and c.n > 96):
        assert totals["wave"] >= 1


@pytest.mark.parametrize("c", RUNS, ids=[c.name for c in RUNS])
def test_long_read_in_the_range(world, c):
    """with a read beyond 320 bases in the range k_near_hits does not run: the same lists from k_gather_general's hit lists"""
    counts, ovl, cov, totals, recs = world[c.name]["gpu_long"]
    lists, ocov = world[c.name]["orc_long"]
    same_lists(lists, counts, ovl, c.name + " + long read")
    assert np.array_equal(ocov, cov)
    c0, o0 = world[c.name]["gpu"][:2]
    assert counts[0] == c0[0] and np.array_equal(ovl[:counts[0]], o0)  # the short read's list, record for record
    assert totals["ranges_xlong"] == 1 and np.all(recs["xlong"] == 1)
    assert not recs["near_done"].any() and not recs["simple"].any()
    if c.route and c.n is not None:
        t = target_of(c, recs)
        assert len(t) == 1
        want = "big_by_scratch" if c.scratch else "big_by_size" if c.n > cc.WAVE_CAP else "general_lane" if c.n <= 32 else "wave_small" if c.n <= 512 else "wave_large"
        assert t1k_amd.ROUTE_NAMES[t[0]["route"]] == want
        assert t[0]["n"] == (0xFFFFFFFF if c.n > cc.WAVE_CAP else c.n)


def test_without_simple_chains(world, tmp_path):
    """T1K_NO_SIMPLE_CHAIN=1 (read once per process: a fresh child): the two-diagonal chains go through the general path, the lists stay"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, T1K_NO_SIMPLE_CHAIN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(out)
    n_groups = 0
    for c in RUNS:
        counts, ovl, cov, recs = (z["%s/%s" % (c.name, k)] for k in ("counts", "ovl", "cov", "recs"))
        lists, ocov = world[c.name]["orc"]
        same_lists(lists, counts, ovl, c.name + " without simple chains")
        assert np.array_equal(ocov, cov)
        assert not recs["simple"].any()
        n_groups += len(recs)
        if c.route and c.n is not None and c.simple:  # same hit list, now by hit count alone
            t = target_of(c, recs)
            assert len(t) == 1 and t[0]["n"] == c.n
            assert c.asymmetric or bool(t[0]["near_done"]) == c.near_done  # (asymmetric: either, see test_route_of_the_target_group)
            want = "big_by_scratch" if c.scratch else "general_lane" if c.n <= 32 else "wave_small"
            assert t1k_amd.ROUTE_NAMES[t[0]["route"]] == want
    assert n_groups > 0


def test_group_at_the_big_cap(built, tmp_path):
    """exactly 16384 hits in one diagonal run (a 10-mer repeat: every diagonal within the radius of the next): the most k_chain_big takes, its
    scratch arrays full to the last word.  Its one lane sorts and filters the run in one piece, which takes seconds -- the size is the
    point, so the case is assigned once, here"""
    (c,) = [c for c in CASES if c.heavy]
    assert c.n == cc.BIG_CAP
    fa = cc.write_fasta(c, str(tmp_path / "cap.fa"))
    lists, ocov = oracle_lists(c, fa, [c.read])
    assert len(lists[0][0]) > 0
    t0 = time.time()
    counts, ovl, cov, totals, recs = assign(c, fa, [c.read])
    print("%.2f s; totals %s" % (time.time() - t0, {k: totals[k] for k in TOTALS}))
    same_lists(lists, counts, ovl, c.name)
    assert np.array_equal(ocov, cov)
    (t,) = target_of(c, recs)
    assert t1k_amd.ROUTE_NAMES[t["route"]] == "big_by_size" and t["n"] == 0xFFFFFFFF and not t["near_done"] and totals["big"] >= 1


def test_group_beyond_the_big_cap(built, tmp_path):
    """more than 16384 hits in one group: T1K_ERR_CAPACITY "group too large", and the call gives up (t1k_assign_range runs a range again only
    for an arena it can grow, and this flag names none; t1k_assign_batch splits nothing), no range is counted, no overlap is returned"""
    (c,) = [c for c in CASES if c.route == "capacity"]
    assert c.n > cc.BIG_CAP
    fa = cc.write_fasta(c, str(tmp_path / "big.fa"))
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(fa)
    ctx = t1k_amd.Context(ref_seq_similarity=0.8)
    ctx.route_report_enable()
    ctx.ref_upload(seqs, masks)
    ctx.reads_upload([c.read])
    t0 = time.time()
    with pytest.raises(t1k_amd.T1kError) as e:
        ctx.assign()
    dt = time.time() - t0
    print("refused after %.2f s: %s" % (dt, e.value))
    assert "(-3)" in str(e.value) and "group too large" in str(e.value)
    totals, recs = ctx.route_report()
    assert totals["ranges"] == 0 and len(recs) == 0  # the pass was not kept
    assert dt < 30  # (one pass of a single read: well under a second; a retry loop that did not end would not come back at all)
    counts, ovl = ctx.overlaps()
    assert counts.sum() == 0 and len(ovl) == 0
    assert ctx.stats()["batches"] == 0
    ctx.close()
    assert ctx.h is None


@pytest.mark.xfail(strict=True, raises=t1k_amd.T1kError, reason="a group may yield at most 32 candidates (k_chain_wave, k_chain_big): 41 diagonals are refused with 'group too large'")
def test_many_diagonals(built, tmp_path):
    """4096 hits on 41 diagonals of a 12-mer repeat (chain_routes_cases.c_many_diagonals): the oracle gives the read overlaps, the library
    refuses the range with T1K_ERR_CAPACITY "group too large" because every diagonal is a candidate and a group keeps 32.  Strict: the
    day the candidates of a group are no longer capped, this must pass as it stands"""
    (c,) = [c for c in CASES if c.route == "candidate_cap"]
    fa = cc.write_fasta(c, str(tmp_path / "many.fa"))
    lists, ocov = oracle_lists(c, fa, [c.read])
    assert len(lists[0][0]) > 0
    try:
        counts, ovl, cov, totals, recs = assign(c, fa, [c.read])
    except t1k_amd.T1kError as e:  # the expected failure is this refusal and no other
        assert "(-3)" in str(e) and "group too large" in str(e), e
        raise
    same_lists(lists, counts, ovl, c.name)
    assert np.array_equal(ocov, cov)


def test_every_route_is_reached(world):
    """the sum of the cases' reports: every list, every alignment queue, every route and both flags of k_near_hits, for both instantiations"""
    for nw in (5, 10):
        tot = {k: 0 for k in TOTALS}
        routes = {r: 0 for r in t1k_amd.ROUTE_NAMES}
        flags = dict(near_done=0, simple=0, gathered=0, near_done_not_simple=0)
        for c in RUNS:
            if c.nw != nw:
                continue
            _, _, _, totals, recs = world[c.name]["gpu"]
            for k in TOTALS:
                tot[k] += totals[k]
            for r in recs:
                routes[t1k_amd.ROUTE_NAMES[r["route"]]] += 1
                flags["near_done"] += int(r["near_done"]); flags["simple"] += int(r["simple"]); flags["gathered"] += int(not r["near_done"])
                flags["near_done_not_simple"] += int(r["near_done"] and not r["simple"])
        print("NW = %d: totals %s routes %s flags %s" % (nw, tot, routes, flags))
        if nw == 5:  # (a read of at most 160 bases has too few offsets for 16384 hits, but 4097 it reaches)
            assert routes["big_by_size"] >= 1
        for stem in ("simple_n96", "simple_n97", "scratch_wave"):  # the cases that may take either of two outcomes took the one they claim
            (c,) = [c for c in RUNS if c.name == "%s_nw%d" % (stem, nw)]
            (t,) = target_of(c, world[c.name]["gpu"][4])
            assert (t1k_amd.ROUTE_NAMES[t["route"]], bool(t["near_done"]), bool(t["simple"])) == (c.route, c.near_done, c.simple), c.name
        zero = [k for k, v in list(tot.items()) + list(routes.items()) + list(flags.items()) if v == 0]
        assert not zero, "NW = %d never reached: %s" % (nw, zero)


def main(out, d):
    z = {}
    for c in RUNS:
        counts, ovl, cov, totals, recs = assign(c, cc.write_fasta(c, os.path.join(d, c.name + ".fa")), [c.read])
        z.update({"%s/counts" % c.name: counts, "%s/ovl" % c.name: ovl, "%s/cov" % c.name: cov, "%s/recs" % c.name: recs})
    np.savez(out, **z)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
