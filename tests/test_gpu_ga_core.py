"""GPU test (pytest -m gpu) of the gap alignment that the dense DP phase runs (gapAlign: the one-word sweeps t1k_ga_matches_equal_w / t1k_ga_band_w<4>
with the text window in registers, the int32 sweep beyond their range), through Context.gap_count_batch, against
(1) the nm of Context.align_batch -- the traced general DP, which shares no code with these sweeps and which
    test_global_alignment_kernel_vs_reference_vectors pins to the reference's own outputs -- and
(2) the MATCH columns of the committed reference vectors with |length difference| <= 4 (AlignAlgo.hpp:215-421).
Shapes: every pattern length at which the sweeps change row class or reload a window (2 .. 150), both sides of the one-word bound (equal lengths
of 510), each with length differences -4 .. +4; substitution rates far above the three mismatches of the callers' fast path; N in the text, in
the pattern, in both; texts back to back in one packed stream, so that their windows start at every offset against its 32- and 64-base words;
a stream of texts without any N (read without its N mask, as a reference without N is) and one with."""
import gzip
import os
import random

import numpy as np
import pytest

import util
import t1k_amd

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 6, 7, 8, 11, 12, 13, 31, 32, 33, 37, 38, 63, 64, 65, 96, 97, 150]
BOUND = 510   # longest equal-length pair of the one-word sweeps: (510 + 1)^2 <= 262142 < (511 + 1)^2 (t1k_ga_word_ok)
ALPHA = "ACGT"


def _pair(rng, lp, d, text_n, pat_n, two_letter=False):
    letters = "AC" if two_letter else ALPHA
    pat = [rng.choice(letters) for _ in range(lp)]
    sub = rng.choice((0.2, 0.3, 0.4))
    text = []
    indel = {rng.randrange(lp) for _ in range(rng.randrange(3))}
    for i, c in enumerate(pat):
        if i in indel:
            if rng.random() < 0.5:
                continue
            text.append(rng.choice(letters))
        text.append(rng.choice(letters) if rng.random() < sub else c)
    lt = lp + d
    while len(text) < lt:
        text.append(rng.choice(letters))
    text = text[:lt]
    for seq, k in ((text, text_n), (pat, pat_n)):
        for _ in range(k):
            seq[rng.randrange(len(seq))] = "N"
    return "".join(text), "".join(pat)


def _jobs(with_text_n):
    rng = random.Random(29 if with_text_n else 17)
    jobs = []
    for lp in LENGTHS + [BOUND - 1, BOUND, BOUND + 1]:
        reps = 2 if lp >= BOUND - 1 else 4
        for d in range(-4, 5):
            if lp + d < 1 or (d == 0 and lp < 2):
                continue
            for r in range(reps):
                text_n = (r % 2 + 1) if with_text_n else 0
                pat_n = r // 2 if lp > 2 else 0
                jobs.append(_pair(rng, lp, d, min(text_n, lp + d), pat_n, two_letter=(r == 3)))
    return jobs


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


@pytest.fixture(scope="module", params=[False, True], ids=["text_without_N", "text_with_N"])
def case(request, ctx):
    jobs = _jobs(request.param)
    texts, pats = [j[0] for j in jobs], [j[1] for j in jobs]
    assert any("N" in t for t in texts) == request.param and any("N" in p for p in pats)
    _, nm, _, _, _ = ctx.align_batch(texts, pats, want_ops=False)   # the yardstick, once per job set
    return texts, pats, np.array(nm)


def test_job_set_is_not_trivial(case):
    texts, pats, nm = case
    assert 600 < len(texts) < 3000
    mism = np.array([min(len(t), len(p)) for t, p in zip(texts, pats)]) - nm
    big = np.array([len(p) for p in pats]) >= 63
    assert (mism[big] > 3).mean() > 0.9          # far above the fast path's three mismatches
    assert {len(p) for p in pats} >= set(LENGTHS) | {BOUND - 1, BOUND, BOUND + 1}
    assert {len(t) - len(p) for t, p in zip(texts, pats) if len(p) > 8} == set(range(-4, 5))


@pytest.mark.parametrize("lead", [0, 13, 57])
def test_gap_count_vs_traced_alignment(ctx, case, lead):
    """texts back to back behind `lead` bases: three different placements of every window against the stream's words"""
    texts, pats, nm = case
    got = ctx.gap_count_batch(texts, pats, lead="G" * lead)
    offs = lead + np.concatenate(([0], np.cumsum([len(t) for t in texts])[:-1]))
    lens = np.array([len(t) for t in texts])
    assert ((offs % 32) + lens > 32).any() and ((offs % 64) + lens > 64).any() and len(set(offs % 32)) == 32
    bad = np.nonzero(got != nm)[0]
    assert len(bad) == 0, [(int(i), texts[i], pats[i], int(got[i]), int(nm[i])) for i in bad[:5]]


def test_gap_count_vs_reference_vectors(ctx):
    vec = []
    with gzip.open(os.path.join(util.GOLDEN, "ga_vectors.tsv.gz"), "rt") as f:
        for line in f:
            t, p, score, ops = line.rstrip("\n").split("\t")
            if abs(len(t) - len(p)) <= 4 and t and p and not (len(t) == len(p) and len(t) < 2):
                vec.append((t, p, ops.count("0")))
    assert len(vec) > 600
    want = np.array([v[2] for v in vec])
    got = ctx.gap_count_batch([v[0] for v in vec], [v[1] for v in vec])
    assert np.array_equal(got, want), [vec[i] for i in np.nonzero(got != want)[0][:5]]
    clean = [v for v in vec if "N" not in v[0]]   # a stream of texts without N: the path that does not load the text's N mask
    assert len(clean) > 300
    got = ctx.gap_count_batch([v[0] for v in clean], [v[1] for v in clean], lead="ACGTACG")
    assert np.array_equal(got, np.array([v[2] for v in clean]))
