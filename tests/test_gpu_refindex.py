"""The reference index as t1k_ref_upload's kernels build it, array by array, against its plain restatement (tests/refindex_ref.py, pinned to
the reference's own KmerIndex and to the oracle by tests/test_refindex_cpu.py) on the designed cases of tests/refindex_cases.py.  The index
is read through the reference view (Context.ref_geometry / ref_array: t1k_ref_view_*); every comparison is integer equality, and a
difference is reported with the array's name, the first index and the case (tests/gpu_refindex_check.py)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_refindex_check as chk  # noqa: E402
import refindex_cases as rc  # noqa: E402
import refindex_ref as rr  # noqa: E402
import t1k_amd  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = [("rule+n+order", k, n) for k, n in rc.RULE_WORLDS] + [(g,) + rc.GENO for g in ("lengths", "n", "straddle", "haspre", "dir", "transpose")] + [("straddle", 15, 0)]


def cases_of(group, k, n_code):
    if group == "rule+n+order":
        return [c for c in rc.all_cases() if c.vs_reference and (c.k, c.n_code) == (k, n_code)]
    return [c for c in rc.by_group(group, k, n_code) if not c.vs_reference and c.transpose]


def test_every_case_is_run():
    ran = {c.name for g, k, n in GROUPS for c in cases_of(g, k, n)}
    assert ran | {"transpose_off_k11_n3"} == {c.name for c in rc.all_cases()}


@pytest.mark.parametrize("group,k,n_code", GROUPS)
def test_index_equals_the_restatement(built, group, k, n_code):
    """1. every array of every case, each on a context of its own world; the cases of a group one after the other on one context.  (Letters
    outside ACGTN, case other_letters: the device's documented behaviour -- N -- is what is pinned; the reference itself codes them as T.)"""
    cases = cases_of(group, k, n_code)
    assert cases
    ctx = t1k_amd.Context(kmer_length=k, n_base_code=n_code)
    try:
        for c in cases:
            t0 = time.perf_counter()
            chk.upload(ctx, c)
            t1 = time.perf_counter()
            chk.compare(ctx, c)
            print("%s: %d alleles, upload %.3f s, restatement + comparison %.3f s" % (c.name, len(c.seqs), t1 - t0, time.perf_counter() - t1))
    finally:
        ctx.close()


def test_transposed_copy_switched_off(built):
    """2. T1K_REF_TRANSPOSE=0 (read once per process: a process of its own): no basesT, no blockT, the rest as with it"""
    env = dict(os.environ, T1K_REF_TRANSPOSE="0")
    r = subprocess.run([sys.executable, os.path.abspath(chk.__file__), "transpose_off_k11_n3"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]


def test_second_upload_leaves_nothing_behind(built):
    """3. a smaller, different reference uploaded over a larger one on the same context: bucket counts, bitmaps and directory are those of
    the second alone; and the first again over the second"""
    big, small, tiny = rc.get("dir_A1025_k11_n3"), rc.get("order_multi_k11_n3"), rc.get("haspre_k11_n3")
    assert len(big.seqs) > len(small.seqs) and big.ref().nPost > small.ref().nPost > tiny.ref().nPost and big.ref().dirRows and not small.ref().dirRows
    ctx = t1k_amd.Context(kmer_length=11, n_base_code=3)
    try:
        for c in (big, small, tiny, big, tiny):
            chk.upload(ctx, c)
            chk.compare(ctx, c)
    finally:
        ctx.close()


def test_shared_reference(built):
    """4. a context that took its reference through ref_share reports the same geometry and the same arrays"""
    c = rc.get("dir_A513_k11_n3")
    src, dst = t1k_amd.Context(kmer_length=11, n_base_code=3), t1k_amd.Context(kmer_length=11, n_base_code=3)
    try:
        with pytest.raises(t1k_amd.T1kError, match=r"t1k_ref_view_geometry failed \(-1\).*no reference"):
            dst.ref_geometry()
        chk.upload(src, c)
        dst.ref_share(src)
        assert chk.compare(dst, c) == chk.compare(src, c)
    finally:
        dst.close()
        src.close()


def test_slices_are_bounds_checked(built):
    c = rc.get("order_multi_k11_n3")
    ctx = t1k_amd.Context(kmer_length=11, n_base_code=3)
    try:
        with pytest.raises(t1k_amd.T1kError, match=r"t1k_ref_view_copy failed \(-1\).*no reference"):
            ctx.ref_array("bases", 0, 1)
        chk.upload(ctx, c)
        geo = ctx.ref_geometry()
        for i, (name, _) in enumerate(t1k_amd.REF_ARRAYS):
            n = geo["len"][name]
            assert len(ctx.ref_array(name, n, 0)) == 0
            for first, count in ((n, 1), (0, n + 1), (n + 1, 0)):
                with pytest.raises(t1k_amd.T1kError, match=r"t1k_ref_view_copy failed \(-1\)"):
                    ctx.ref_array(name, first, count)
            room = np.zeros(16, np.uint64)
            assert t1k_amd.lib().t1k_ref_view_copy(ctx.h, i, 1, (1 << 64) - 1, room.ctypes.data) == -1  # (first + count wraps to 0)
            if n >= 3:
                assert np.array_equal(ctx.ref_array(name, 1, n - 2), ctx.ref_array(name)[1:n - 1])
        assert t1k_amd.lib().t1k_ref_view_copy(ctx.h, len(t1k_amd.REF_ARRAYS), 0, 0, None) == -1
        assert t1k_amd.lib().t1k_ref_view_copy(ctx.h, -1, 0, 0, None) == -1
    finally:
        ctx.close()


def test_failed_upload_leaves_no_reference(built):
    """an upload that fails after the old arrays were freed (an allele of 2^20 bases) leaves a context without a reference: the view and
    the stages refuse instead of reading freed memory; the next upload works"""
    c = rc.get("order_multi_k11_n3")
    ctx = t1k_amd.Context(kmer_length=11, n_base_code=3)
    try:
        chk.upload(ctx, c)
        with pytest.raises(t1k_amd.T1kError, match=r"t1k_ref_upload failed \(-1\).*2\^20"):
            ctx.ref_upload(["ACGT" * (1 << 18)])
        with pytest.raises(t1k_amd.T1kError, match=r"no reference"):
            ctx.ref_geometry()
        with pytest.raises(t1k_amd.T1kError, match=r"no reference"):
            ctx.ref_array("kStart", 0, 1)
        chk.upload(ctx, c)
        chk.compare(ctx, c)
    finally:
        ctx.close()


def test_seeding_reads_the_lists_the_view_shows(built):
    """5. one link to the consumers: a dozen reads of the word-straddle case with the seed report on -- every used k-mer's list_len is
    kStart[c + 1] - kStart[c] of the fetched index for the code c of the read's k-mer at that offset"""
    c = rc.get("straddle_k11_n3")
    k = c.k
    reads = [c.seqs[a][s:s + ln] for a, s, ln in ((0, 0, 60), (0, 20, 64), (0, 31, 45), (0, 40, 60), (1, 0, 70), (1, 30, 70), (2, 25, 60), (2, 32, 50), (3, 33, 60), (4, 5, 90),
                                                   (5, 40, 60))]
    reads.append(rr.revcomp(c.seqs[0][10:75]))
    ctx = t1k_amd.Context(kmer_length=k, n_base_code=c.n_code, ref_seq_similarity=0.8)
    try:
        chk.upload(ctx, c)
        k_start = ctx.ref_array("kStart")
        ctx.reads_upload(reads)
        ctx.seed_report_enable()
        ctx.assign_range(0, len(reads))
        seen, counts, masks, ptr, used = ctx.seed_report()
        assert seen.all()
        n = 0
        for i, r in enumerate(reads):
            g = used[ptr[i]:ptr[i + 1]]
            assert len(g), "read %d seeds nothing" % i
            for u in g:
                text = (r if u["strand"] == 0 else rr.revcomp(r))[int(u["read_off"]):int(u["read_off"]) + k]
                assert len(text) == k and "N" not in text
                code = rr.encode(text)
                assert int(u["list_len"]) == int(k_start[code + 1]) - int(k_start[code]) == len(c.ref().list_of(code)), (i, int(u["read_off"]), text)
                n += int(u["list_len"]) > 0
        assert n >= len(reads)
    finally:
        ctx.close()
