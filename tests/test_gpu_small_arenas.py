"""GPU tests (pytest -m gpu) of t1k_assign_range's grow-and-run-again path on small inputs.  T1K_TEST_SMALL_ARENAS lowers the floors and the
per-read-end starting figure of the working capacities (never the limits of t1k_params), so that a few hundred read-ends overflow their
first group, candidate and overlap arenas and the driver has to grow each to the demand the device counted.  The result must be what the
oracle computes: every overlap list field for field (similarity bits included) and the per-base coverage.  The switch is read once per
process and the capacities are reported on stderr (T1K_DEBUG_PHASES), so the assignment runs in a child process: this file run as a script.
Without the switch, a group_cap LIMIT too small for the input still ends in T1K_ERR_CAPACITY (the caller splits the range)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import util  # noqa: E402
import t1k_amd  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ["seq_idx", "read_start", "read_end", "seq_start", "seq_end", "strand", "match_cnt", "left_clip", "right_clip", "relaxed_match_cnt"]
# two inputs of tests/gpu_assign_check.py: CYP2D6 rna (300 pairs of 100 bp, -s 0.8) and the indel-rich synthetic HLA reads (150 pairs of
# 150 bp, -s 0.9: groups with several diagonals, the "rare" lists, the general job list)
CASES = ["cyp2d6_rna", "synthetic_hla_indels"]
# what t1k_assign_range starts from under the switch: max(floor, per read-end x read-ends)
START = {"groups": lambda n: max(1024, 2 * n), "candidates": lambda n: max(128, 2 * n * 5 // 12), "overlaps": lambda n: max(128, 2 * n // 3)}


def case_input(name, tmp):
    if name == "cyp2d6_rna":
        fa = util.gunzip_to(util.CYP_RNA, os.path.join(tmp, "cyp_rna.fa"))
        util.synth_reads(fa, os.path.join(tmp, "c1"), pairs=300, len=100, seed=11, sub=0.005)
        pfx, sim = os.path.join(tmp, "c1"), 0.8
    else:
        fa = os.path.join(tmp, "hla.fa")
        util.synth_ref("ref-rna", fa, genes=4, scale=0.05)
        util.synth_reads(fa, os.path.join(tmp, "h3"), pairs=150, len=150, seed=9, sub=0.004, indel=0.006)
        pfx, sim = os.path.join(tmp, "h3"), 0.9
    reads = [s for _, _, s in t1k_amd.read_fastx(pfx + "_1.fq")] + [s for _, _, s in t1k_amd.read_fastx(pfx + "_2.fq")]
    return fa, reads, sim


def child(name, tmp):
    """assign() of one case through the C ABI; the lists and the coverage go to <tmp>/out.npz"""
    fa, reads, sim = case_input(name, tmp)
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(fa)
    ctx = t1k_amd.Context(ref_seq_similarity=sim)
    ctx.ref_upload(seqs, masks)
    ctx.reads_upload(reads)
    ctx.assign()  # (raises unless T1K_OK)
    counts, ovl = ctx.overlaps()
    np.savez(os.path.join(tmp, "out.npz"), counts=counts, ovl=ovl, cov=ctx.coverage())
    ctx.close()


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    """every case once: the child's lists, coverage and stderr, and the oracle's lists and coverage for the same input"""
    out = {}
    for name in CASES:
        tmp = str(tmp_path_factory.mktemp(name))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, tmp], stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, T1K_TEST_SMALL_ARENAS="1", T1K_DEBUG_PHASES="1"))
        assert r.returncode == 0, (name, r.stderr[-2000:])
        fa, reads, sim = case_input(name, tmp)
        _, seqs, _, _ = t1k_amd.load_reference_fasta(fa)
        orc = util.Oracle(fa, similarity=sim, relax=False)
        lists = [orc.assign_read(x) for x in reads]
        cov = np.concatenate([orc.coverage(a, len(s)) for a, s in enumerate(seqs)])
        caps = [dict(groups=int(g), candidates=int(c), overlaps=int(o)) for g, c, o in
                re.findall(r"again with capacities: groups (\d+) lists \d+ / \d+ jobs \d+ / \d+ candidates (\d+) overlaps (\d+)", r.stderr)]
        print("%s: %d read-ends, capacities of the run-agains: %s" % (name, len(reads), caps))
        out[name] = dict(n=len(reads), got=np.load(os.path.join(tmp, "out.npz")), lists=lists, cov=cov, caps=caps)
    return out


def grown_alone(run, what):
    """run-agains in which capacity `what` grew and the capacities ahead of it in the pipeline did not (it was the arena that overflowed)"""
    order = ["groups", "candidates", "overlaps"]
    ahead = order[:order.index(what)]
    prev = {k: START[k](run["n"]) for k in order}
    hits = 0
    for caps in run["caps"]:
        if caps[what] > prev[what] and all(caps[k] == prev[k] for k in ahead):
            hits += 1
        prev = caps
    return hits


@pytest.mark.parametrize("name", CASES)
def test_overflowing_first_capacities_give_the_oracles_lists_and_coverage(runs, name):
    run = runs[name]
    assert run["caps"], "no range ran again: the switch did not make the first capacities overflow"
    assert len(run["caps"]) <= 10  # (the driver gives up after attempt 10)
    counts, ovl = run["got"]["counts"], run["got"]["ovl"]
    assert len(counts) == run["n"] and int(counts.sum()) == len(ovl)
    pos = 0
    for i, (o, s) in enumerate(run["lists"]):
        g = ovl[pos:pos + counts[i]]
        pos += counts[i]
        assert len(o) == len(g), "read-end %d: oracle %d overlaps, GPU %d" % (i, len(o), len(g))
        for k, f in enumerate(FIELDS):
            assert np.array_equal(o[:, k], g[f]), "read-end %d: %s differs: oracle %s GPU %s" % (i, f, o[:, k][:8], g[f][:8])
        assert np.array_equal(s, g["similarity"]), "read-end %d: similarity differs" % i
    assert np.array_equal(run["cov"], run["got"]["cov"])


@pytest.mark.parametrize("what", ["groups", "candidates", "overlaps"])
def test_each_arena_triggers_a_run_again_of_its_own(runs, what):
    """over the two inputs, the group bit, the candidate bit and the overlap bit of the error word each make a range run again"""
    assert sum(grown_alone(runs[name], what) for name in CASES) >= 1, {name: runs[name]["caps"] for name in CASES}


def test_group_cap_limit_too_small_is_a_capacity_error(built, tmp_path):
    """at the limits nothing grows: T1K_ERR_CAPACITY (-3) naming the limit, and the caller splits the range"""
    fa, reads, sim = case_input("cyp2d6_rna", str(tmp_path))
    _, seqs, masks, _ = t1k_amd.load_reference_fasta(fa)
    ctx = t1k_amd.Context(ref_seq_similarity=sim, group_cap=2048)
    ctx.ref_upload(seqs, masks)
    ctx.reads_upload(reads)
    with pytest.raises(t1k_amd.T1kError) as e:
        ctx.assign()
    assert "(-3)" in str(e.value) and "group_cap" in str(e.value), str(e.value)
    ctx.close()


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
