"""CPU test (no GPU): the two host statements of Genotyper::CoalesceReadAssignments (Genotyper.hpp:841-908) agree -- the Python
restatement tests/coalesce_ref.py, which is the expectation of test_gpu_coalesce.py, and Genotyper::coalesce of the job layer
(t1k_job_coalesce_rows), which test_gpu_parity.py holds the GPU against on real samples.  The rows are those of the GPU file's
generators, paired by the oracle: run lengths on every batch edge of the two fold kernels, one run above 4096 fragments, patterns of
1, 63, 64, 65, 128 and 129 alleles.  The conditions under which a wrong fold order or a lost row changes bits are asserted here too, so
that the seeds of the generators are guarded without a GPU."""
import numpy as np

import t1k_amd
import util
import coalesce_ref as cr
import test_distributed_gloo as tdg
import test_gpu_pair as tp


def test_restatement_equals_host_coalescing(built, tmp_path):
    B, L, T = t1k_amd.coalesce_limits()
    fasta = str(tmp_path / "ref.fa")
    alen = tp.make_reference(fasta)
    orc = util.Oracle(fasta, similarity=0.8, relax=False, max_assign=0)
    long_run = max(L, 4096) + 1
    cases = [("a", cr.case_a(B, L)), ("a below 2 B + 2, as the GPU file's child process folds it", cr.case_a(B, 2 * B + 2)),
             ("a with the exchange test's extra run", cr.case_a(B, L, extra=(12 * B + 7,))), ("b", cr.case_b(B, T)), ("d", cr.case_d(B, T)), ("one long run", cr.case_c(B, L, T, runs=[long_run]))]
    slots, runs = set(), set()
    for name, fr in cases:
        counts, rec, has_n = fr.lists()
        ovl = cr.overlap_lists(rec, alen)
        rc, rows = cr.rows_by_oracle(orc, counts, ovl, has_n)
        assert int((rc > 0).sum()) == sum(fr.runs) and (rc == 0).sum() >= len(rc) // 6, name   # every generated row survives; the empty ones are there
        want = cr.coalesce_ref(rc, rows)
        assert sorted(want[3].tolist()) == sorted(fr.runs), name
        host = t1k_amd.Job(fasta, device=-1)
        host.coalesce_rows(rows, rc)
        g, assigned, ptr, first, ent = tdg.parse_table(host.groups_serialize())
        host.close()
        assert g == len(fr.runs) and assigned == sum(fr.runs), name
        diff = cr.same_table(want, (ptr, ent, first))
        assert diff is None, "%s: %s of group %d, slot %d (run %d)" % ((name,) + diff + (want[3][diff[1]],))
        assert np.array_equal(first, np.sort(first))  # numbered by first appearance
        for gi, n in enumerate(fr.runs):
            fs = fr.fragments_of(gi)
            assert np.any(np.diff(fs) > 1) or n < 2, "%s: the run of group %d is contiguous in fragment order" % (name, gi)
            if n >= 3:  # (a run of one has no order, a run of two adds two floats: commutative)
                assert cr.order_conditions(rc, rows, fs) == (True, True, True), "%s: group %d (run %d) does not show a wrong fold order" % (name, gi, n)
            slots.add(len(fr.patterns[gi]))
            runs.add(n)
    assert {1, 64, 65, 129} <= slots and max(runs) > 4096


def test_another_order_another_table(built, tmp_path):
    """the restatement's own `order` argument (the sensitivity conditions rest on it): case b folded backwards is another table, folded in
    the default order it is the same one; and the committed salts are what the search gives when it starts from them"""
    B, L, T = t1k_amd.coalesce_limits()
    fasta = str(tmp_path / "ref.fa")
    alen = tp.make_reference(fasta)
    orc = util.Oracle(fasta, similarity=0.8, relax=False, max_assign=0)

    def rows_of(fr):
        counts, rec, has_n = fr.lists()
        return cr.rows_by_oracle(orc, counts, cr.overlap_lists(rec, alen), has_n)
    rc, rows = rows_of(cr.case_b(B, T))
    forward = cr.coalesce_ref(rc, rows)
    assert cr.same_table(forward, cr.coalesce_ref(rc, rows, order=range(len(rc)))) is None
    assert cr.same_table(forward, cr.coalesce_ref(rc, rows, order=range(len(rc) - 1, -1, -1))) is not None
    small = [b for b in cr.salt_builders(B, max(L, 4096), T) if b[0] != "c"]   # (case c's 36 000 fragments are folded in the test above)
    assert cr.search_salts(small, rows_of, start=cr.SALTS) == cr.SALTS
