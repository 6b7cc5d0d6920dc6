"""The reference index on the device (Context.ref_geometry / ref_array: t1k_ref_view_*) against its restatement (tests/refindex_ref.py),
element for element: compare() is what tests/test_gpu_refindex.py calls for every designed case.  As a program it uploads one case of
tests/refindex_cases.py by name in a process of its own (T1K_REF_TRANSPOSE is read once per process) and exits 0 when all is equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refindex_cases as rc  # noqa: E402
import refindex_ref as rr  # noqa: E402
import util  # noqa: E402,F401
import t1k_amd  # noqa: E402

DENSE = ("kStart", "kHas", "kMulti", "kHasPre", "kDirIdx")


def same(name, got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s holds %s elements, restatement %s" % (what, name, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[0]
        raise AssertionError("%s: %s differs at %s: device %s, restatement %s (%d elements differ)" % (what, name, tuple(at), got[tuple(at)], want[tuple(at)], int((got != want).sum())))


def upload(ctx, case):
    ctx.ref_upload(case.seqs, case.exon)


def compare(ctx, case):
    """every array of the context's index equals the restatement of `case`; -> the geometry"""
    ix, what = case.ref(), case.name
    geo = ctx.ref_geometry()
    want = ix.geometry()
    assert {f: geo[f] for f in want} == want, "%s: geometry %s, restatement %s" % (what, {f: geo[f] for f in want}, want)
    small = ix.small()
    assert set(small) | set(DENSE) == {n for n, _ in t1k_amd.REF_ARRAYS}
    for name, w in small.items():
        assert geo["len"][name] == len(w), "%s: %s holds %d elements, restatement %d" % (what, name, geo["len"][name], len(w))
        got = ctx.ref_array(name)
        if name == "kPost":
            got = np.stack([got["allele"], got["offset"]], axis=1) if len(got) else np.zeros((0, 2), np.uint32)
        same(name, got, w, what)
    n = 1 << (2 * case.k)
    assert [geo["len"][x] for x in DENSE] == [n + 1, (n + 31) // 32, (n + 31) // 32, ((1 << (2 * max(1, case.k - 2))) + 31) // 32, n], what
    if not case.slices:
        for name, w in ix.dense().items():
            same(name, ctx.ref_array(name), w, what)
        return geo
    # k = 15: the cells around the codes of the case's windows and around a few absent ones
    codes = sorted(ix.seen) + [0, 1, n - 1, n // 3, 987654321 % n]
    one = lambda name, i: int(ctx.ref_array(name, i, 1)[0])
    assert one("kStart", n) == ix.nPost and one("kStart", 0) == 0, what
    for c in codes:
        got = ctx.ref_array("kStart", c, 2).tolist()
        assert got == [ix.k_start(c), ix.k_start(c + 1)], "%s: kStart[%d .. %d] device %s, restatement %s" % (what, c, c + 1, got, [ix.k_start(c), ix.k_start(c + 1)])
        assert one("kDirIdx", c) == ix.dir_idx(c), "%s: kDirIdx[%d]" % (what, c)
        w = c >> 5
        assert one("kHas", w) == ix.has_word(w), "%s: kHas word %d" % (what, w)
        assert one("kMulti", w) == ix.multi_word(w), "%s: kMulti word %d" % (what, w)
        for text in (rr.decode(c, case.k), rr.revcomp(rr.decode(c, case.k))):
            p = rr.canonical_prefix(rr.encode(text), case.k) >> 5
            assert one("kHasPre", p) == ix.pre_word(p), "%s: kHasPre word %d" % (what, p)
    return geo


def main(name):
    c = rc.get(name)
    ctx = t1k_amd.Context(kmer_length=c.k, n_base_code=c.n_code)
    try:
        upload(ctx, c)
        compare(ctx, c)
    finally:
        ctx.close()
    print("%s: equal" % name)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
