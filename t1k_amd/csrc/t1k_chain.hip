// t1k_amd/csrc/t1k_chain.hip -- chaining of SeqSet::AssignRead on gfx950: the group records that seeding leaves (t1k_seed.hip; record layout in
// t1k_chain_rec.h) -> candidate overlaps per read-end, as a sequence of flat, batch-wide kernels (all integer, HBM/LDS-bound; no MFMA):
//
//   k_chain_fast<*, 0>  one lane per (read-end, strand, allele) group over the whole batch: single-diagonal closed form
//                       (GetOverlapsFromHits 1232-1556 + seed-chain match count 1697-1848); groups that need the gap walk go to the
//                       slow list, groups with hits on several diagonals to the general list
//   k_chain_fast<*, 1>  the gap walk over the slow list: alignments that need a DP are registered in the read-end's memo
//   k_dp_dense          one lane per distinct registered alignment (banded forward sweep, band in registers)
//   k_chain_fast<*, 2>  groups whose memo slot was taken run again behind k_dp_dense (retry list)
//   k_near_hits, k_gather_general, k_chain_general, k_chain_wave, k_general_finish, k_chain_big
//                       groups with hits on several nearby diagonals: their hit lists, then the reference's diagonal-run / LIS logic verbatim
//   k_collect           one workgroup per read-end: strand vote (1619-1648), match counts of candidates that waited for the memo, copy-out
//                       of the winning strand's candidates
//   k_arena_compact, k_csort_*   striped work list -> dense list; counting sort of a dense list by a small key
#include <algorithm>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_memo.h"
#include "t1k_group.h"
#include "t1k_chain_rec.h"

#define GROUP_FAST_MAXLEN 320
#define GENERAL_CAP 128             // hits per group handled by k_chain_general in private memory; larger groups: k_chain_big
#define BIG_CAP 16384
#define GA_BIG_MAX 2048
#define GA_SCRATCH_INTS (6 * (GA_BIG_MAX + 4))

// ------------------------------------------------------------------------------------------------------------------
// group -> candidate overlaps
// ------------------------------------------------------------------------------------------------------------------
struct CandOut {  // packed candidates: 3 u32 each (+ 3 u32 of memo references when stride == 6, multi-diagonal groups)
  uint32_t *dst;
  int n;
  int stride = 3;
  int cap = 0x7FFFFFFF;
  bool overflow = false;
  __device__ void push(int rs, int re, int ss, int se, int m0, int m) {
    if (n >= cap) { overflow = true; return; }
    dst[stride * n + 0] = (uint32_t)rs | ((uint32_t)re << 12);
    dst[stride * n + 1] = (uint32_t)ss | ((uint32_t)m0 << 20);
    dst[stride * n + 2] = (uint32_t)se | ((uint32_t)m << 20);
    if (stride == 6) dst[6 * n + 3] = dst[6 * n + 4] = dst[6 * n + 5] = 0;
    ++n;
  }
  // memo slots whose match counts are still missing from the last pushed candidate's matchCnt (count in bits 24..27 of word 0)
  __device__ void setRefs(const uint32_t *refs, int nref) {
    if (overflow || stride != 6 || n == 0) return;
    uint32_t *d = dst + 6 * (n - 1);
    d[0] |= (uint32_t)nref << 24; d[3] = refs[0]; d[4] = refs[1]; d[5] = refs[2];
  }
};

// seed-chain match count of one gap (SeqSet.hpp:1710-1752 / 1794-1824)
__device__ inline int gapMatches(const ReadCtx &c, int ra, int ga, int lp, int lt, int *gaScratch, int gaMax, unsigned int *dpCounter, unsigned long long *errFlags,
                                 bool *needScratch) {
  if (lp == lt) return t1k_ga_matches_window(c.rb, c.rn, ra, c.gb, c.gn, c.goff + ga, lp, dpCounter, c.refN);
  if (lt == 0 || lp == 0) return 0;
  if (dpCounter) ++*dpCounter;
  T1kSeqView T{c.gb, c.gn, c.goff + ga, c.refN}, P{c.rb, c.rn, ra};
  const int diff = lt > lp ? lt - lp : lp - lt;
  if (diff <= 4) return t1k_ga_count(T, lt, P, lp);  // band in registers
  if (!gaScratch) { *needScratch = true; return 0; }
  int nm = 0;
  if (lt > gaMax) { atomicOr(errFlags, (unsigned long long)ERR_BIGGROUP); return 0; }
  t1k_ga_general(T, lt, P, lp, gaScratch, nullptr, &nm);
  return nm;
}

// Single-diagonal group (the common case: the read differs from the allele by substitutions only).
// NW = number of 32-position words covering a read (5: reads <= 160 bp, 10: reads <= 320 bp).
//   * input: the group's reference diagonal and the bitmask M of read offsets hitting it, accumulated by k_seed_groups; the
//     caller has checked that every other hit lies more than `radius` diagonals away (it cannot join this run,
//     SeqSet.hpp:1360-1392) and that there are at most two such strays (they cannot form a run of >= 3 hits, 1400-1405)
//   * on one diagonal the LIS is the identity and both hit lengths are equal; with M = bitmask of hit read-offsets,
//     covered = popcount(dilate(M, k)) and matchCnt = 2*covered + 2*sum over gaps of GlobalAlignment matches (1697-1760)
//   * a gap with x <= 3 mismatches aligns ungapped (g - x matches, exact, see t1k_ga_matches_window); if the whole span
//     has <= 3 mismatches every gap does and matchCnt = 2*(span - mismatches) in closed form
//   * exact prune: a gap with x > 3 yields at most g - 1 matches, so U = 2*(span - sum_{x<=3} x - #{x>3}) bounds matchCnt;
//     if U / (2*span) < -s the candidate is certain to fail the similarity filter (1838-1840, 1894-1908) and is emitted
//     with matchCnt = U (it is dropped by k_extend either way, and the strand vote only reads matchCnt0)
// multi-word shift-left-or: C |= C << sft (sft < 64), MW 64-bit words, low word first
template <int MW>
__device__ __forceinline__ void shlOr(uint64_t *C, int sft) {
#pragma unroll
  for (int w = MW - 1; w >= 0; --w) {
    uint64_t carry = w > 0 ? (C[w - 1] >> (64 - sft)) : 0ull;
    C[w] |= (C[w] << sft) | carry;
  }
}

// return value: 5 = needs the gap walk (CLOSED only), 1 = finished (out holds 0 or 1 candidate), 2 = run again after the dense DP phase, 3 = candidate pushed with a
// partial matchCnt, refs[] name the memo slots whose match counts are still to be added (DEFER only)
#ifndef GROUP_MAX_REFS     // (t1k_chain_rec.h defines it; tests/test_closed_form_cpu.py compiles this stretch of the file on its own, without the header)
#define GROUP_MAX_REFS 4
#endif
template <int NW, bool DEFER, bool CLOSED>
__device__ inline int groupFastPath(const uint32_t *Mw, int diag, const ReadCtx &c, bool hasN, int k, int hitLenRequired, double simThreshold, CandOut &out,
                                    unsigned int *dpCounter, int strandBit, const GapSink &sink, uint32_t *refs, int *nRefs, int earlyPrune = 1) {
  constexpr int MW = (NW + 1) / 2;  // 64-bit words of the read-offset bitmask
  uint64_t M[MW];
  int onDiag = 0;
#pragma unroll
  for (int i = 0; i < MW; ++i) {
    M[i] = (uint64_t)Mw[2 * i] | ((2 * i + 1 < NW) ? ((uint64_t)Mw[2 * i + 1] << 32) : 0ull);
    onDiag += __popcll(M[i]);
  }
  if (onDiag < 3) return 1;  // minHitRequired (1314, 1400)
  if (onDiag * k < hitLenRequired) return 1;
  int first = -1, last = -1;
#pragma unroll
  for (int w = 0; w < MW; ++w) {
    if (M[w]) {
      if (first < 0) first = w * 64 + __ffsll((long long)M[w]) - 1;
      last = w * 64 + 63 - __clzll((long long)M[w]);
    }
  }
  // covered positions: dilate M by k (bit p set iff some hit offset a has a <= p < a + k), by doubling
  uint64_t C[MW];
#pragma unroll
  for (int w = 0; w < MW; ++w) C[w] = M[w];
  {
    int have = 1;
    while (2 * have <= k) { shlOr<MW>(C, have); have *= 2; }
    if (have < k) shlOr<MW>(C, k - have);
  }
  int cov = 0;
#pragma unroll
  for (int w = 0; w < MW; ++w) cov += __popcll(C[w]);
  // (the dilation may spill past NW*32 only for offsets that cannot occur: a + k <= len <= NW*32)
  if (cov < hitLenRequired) return 1;  // GetTotalHitLengthOnRead/OnSeq (1512-1522)
  const int spanEnd = last + k, span = spanEnd - first;
  // mismatch bits of the span on this diagonal, relative to `first`: bit 2*j of mmw[i] <-> read position first + 32*i + j.
  // Both windows are fetched as NW + 1 consecutive words and funnel-shifted in registers (one burst of independent loads).
  uint64_t mmw[NW];
  int mmT = 0;
  {
    const int64_t g0 = c.goff + (first - diag);
    const int64_t gw = g0 >> 5;
    const int gsh = (int)(g0 & 31) * 2, rsh = (first & 31) * 2;
    const int rw = first >> 5;
    const int nWin = (span + 31) >> 5;
    constexpr int NP = (NW + 2) / 2;  // 16-byte pieces covering NW + 1 words
    uint64_t G[2 * NP], R[2 * NP], GN[2 * NP], RN[2 * NP];
    // (the allele's words from the transposed copy where there is one: lanes = consecutive alleles, the same word of each, one row -- see T1kRefDev::basesT)
    const uint64_t *gt = c.gT ? c.gT + (gw - (c.goff >> 5)) * 64 : nullptr;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const bool need = 2 * j <= nWin;  // the arrays carry spare words, but do not stream what is never used
      t1k_u64x2 g = {0ull, 0ull}, r = {0ull, 0ull}, rn2 = {0ull, 0ull};
      if (need) {
        if (gt) { g.x = gt[(2 * j) * 64]; g.y = gt[(2 * j + 1) * 64]; } else g = *(const t1k_u64x2 *)(c.gb + gw + 2 * j);
        r = *(const t1k_u64x2 *)(c.rb + rw + 2 * j); rn2 = *(const t1k_u64x2 *)(c.rn + rw + 2 * j);
      }
      G[2 * j] = g.x; G[2 * j + 1] = g.y; R[2 * j] = r.x; R[2 * j + 1] = r.y; RN[2 * j] = rn2.x; RN[2 * j + 1] = rn2.y;
      GN[2 * j] = GN[2 * j + 1] = 0ull;
    }
    if (hasN) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (2 * j <= nWin) { const t1k_u64x2 g = *(const t1k_u64x2 *)(c.gn + gw + 2 * j); GN[2 * j] = g.x; GN[2 * j + 1] = g.y; }
      }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      mmw[i] = 0;
      if (i < nWin) {
        const uint64_t g = (G[i] >> gsh) | ((G[i + 1] << 1) << (63 - gsh)), r = (R[i] >> rsh) | ((R[i + 1] << 1) << (63 - rsh));
        const uint64_t nn = ((GN[i] >> gsh) | ((GN[i + 1] << 1) << (63 - gsh))) | ((RN[i] >> rsh) | ((RN[i + 1] << 1) << (63 - rsh)));
        const uint64_t xo = g ^ r;
        uint64_t mm = (xo | (xo >> 1)) & T1K_EVEN & ~nn;
        const int rem = span - 32 * i;
        if (rem < 32) mm &= t1k_lowmask(rem);
        mmw[i] = mm;
        mmT += __popcll(mm);
      }
    }
  }
  int matchCnt;
  int result = 1;
  // next uncovered / covered position >= from (lowest clear / set bit of C at or above it)
  auto nextClear = [&](int from) -> int {
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      if (from < (w + 1) * 64) {
        uint64_t inv = ~C[w];
        if (from > w * 64) inv &= ~0ull << (from - w * 64);
        if (inv) return w * 64 + __ffsll((long long)inv) - 1;
      }
    }
    return MW * 64;
  };
  auto nextSet = [&](int from) -> int {
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      if (from < (w + 1) * 64) {
        uint64_t v = C[w];
        if (from > w * 64) v &= ~0ull << (from - w * 64);
        if (v) return w * 64 + __ffsll((long long)v) - 1;
      }
    }
    return MW * 64;
  };
  auto mmIn = [&](int gsAbs, int geAbs) -> int {  // mismatches in read positions [gsAbs, geAbs)
    const int gs = gsAbs - first, ge = geAbs - first;
    int x = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      const int p0 = q * 32;
      if (p0 < ge && p0 + 32 > gs) {
        uint64_t msk = ~0ull;
        if (gs > p0) msk &= ~t1k_lowmask(gs - p0);
        if (ge < p0 + 32) msk &= t1k_lowmask(ge - p0);
        x += __popcll(mmw[q] & msk);
      }
    }
    return x;
  };
  if (mmT <= 3) matchCnt = 2 * (span - mmT);
  else if (CLOSED) {
    // first pass: the closed form ... and the groups that are certain to fail the similarity filter whatever their gaps hold.  Every gap
    // (maximal uncovered run inside the span) with a mismatch costs at least one match -- x of them if x <= 3, one or more if x > 3 --
    // so U' = 2 * (span - #gaps holding a mismatch) bounds the exact prune bound U of the gap walk from above; U' / (2 * span) < s
    // means the candidate is dropped (k_collect), and like the walk's pruned candidates it leaves with the bound as its matchCnt
    // (nothing reads the matchCnt of a dropped candidate; the strand vote reads matchCnt0 = 2 * cov).  The gaps are counted without a
    // walk: relative to `first`, X = uncovered positions, E = mismatching positions (a subset of X: covered positions are exact
    // k-mer hits); in X + E every run of X that holds a bit of E carries out exactly once into the covered position above it.
    uint64_t X[MW], E[MW];
    {
      const int ws = first >> 6, bs = first & 63;
#pragma unroll
      for (int w = 0; w < MW; ++w) {
        uint64_t lo = 0, hi = 0;
#pragma unroll
        for (int v = 0; v < MW; ++v) {
          if (v == w + ws) lo = C[v];
          if (v == w + ws + 1) hi = C[v];
        }
        const uint64_t crel = bs ? ((lo >> bs) | (hi << (64 - bs))) : lo;
        const int rem = span - 64 * w;
        X[w] = rem <= 0 ? 0ull : (~crel & (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull)));
        uint64_t e = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (2 * w + h < NW) {
            uint64_t x = mmw[2 * w + h] & 0x5555555555555555ull;
            x = (x | (x >> 1)) & 0x3333333333333333ull; x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full; x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
            x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull; x = (x | (x >> 16)) & 0xFFFFFFFFull;
            e |= x << (32 * h);
          }
        }
        E[w] = e & X[w];
      }
    }
    int nGaps = 0;
    uint64_t carry = 0;
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      const uint64_t s1 = X[w] + E[w], s2 = s1 + carry;
      carry = ((s1 < X[w]) | (s2 < s1)) ? 1ull : 0ull;
      nGaps += __popcll(s2 & ~X[w]);
    }
    const int bound = 2 * (span - nGaps);
    if (earlyPrune && (double)bound / (double)(2 * span) < simThreshold) matchCnt = bound;
    else if (earlyPrune < 2) return 5;  // the gap walk decides (compacted list of these groups)
    else {
      // ... unless its first pass already does: per gap the mismatch count (all in the registers this pass holds).  No gap with more than
      // three mismatches => every gap aligns ungapped and the count is exact; or the walk's own bound U = 2 * (span - sum of the small gaps'
      // mismatches - #big gaps) fails the similarity filter => certain to be dropped.  Round 4 counted 21 % + 39 % of the groups that used to
      // go to k_chain_fast<*, 1> in these two kinds (profiles/r04_walk_classes.txt); only the rest needs the memo and is listed for it.
      int sumSmall = 0, nBig = 0;
      int pos = first;
      while (true) {
        int gs = nextClear(pos);
        if (gs >= spanEnd) break;
        int ge = nextSet(gs);
        if (ge > spanEnd) ge = spanEnd;
        const int x = mmIn(gs, ge);
        if (x <= 3) sumSmall += x; else ++nBig;
        pos = ge;
      }
      const int upper = 2 * (span - sumSmall - nBig);
      if (nBig != 0 && !((double)upper / (double)(2 * span) < simThreshold)) return 5;
      matchCnt = upper;
    }
  }
  else {
    // walk the gaps (maximal uncovered runs inside the span)
    int sumSmall = 0, nBig = 0;
    int pos = first;
    // pass 1: per-gap mismatch counts -> upper bound
    while (true) {
      int gs = nextClear(pos);
      if (gs >= spanEnd) break;
      int ge = nextSet(gs);
      if (ge > spanEnd) ge = spanEnd;
      int x = mmIn(gs, ge);
      if (x <= 3) sumSmall += x; else ++nBig;
      pos = ge;
    }
    const int upper = 2 * (span - sumSmall - nBig);
#ifdef T1K_WALK_STATS
    { const int cls = nBig == 0 ? 0 : ((double)upper / (double)(2 * span) < simThreshold) ? 1 : 2;
      for (int c = 0; c < 3; ++c) { const unsigned long long mk = __ballot(cls == c); if (mk && (int)(threadIdx.x & 63) == __ffsll((long long)mk) - 1) atomicAdd(&sink.counters[T1K_WIN_WALK_STATS + c], (unsigned long long)__popcll(mk)); } }
#endif
    if (nBig == 0) matchCnt = upper;  // exact
    else if ((double)upper / (double)(2 * span) < simThreshold) matchCnt = upper;  // certain to be dropped; no DP needed
    else {
      int gapMatch = 0, nref = 0;
      bool again = false;
      pos = first;
      while (true) {
        int gs = nextClear(pos);
        if (gs >= spanEnd) break;
        int ge = nextSet(gs);
        if (ge > spanEnd) ge = spanEnd;
        int x = mmIn(gs, ge);
        if (x <= 3) gapMatch += (ge - gs) - x;
        else {
          uint32_t slot = 0;
          int r = gapMatchesCached<DEFER>(c, gs, c.goff + (gs - diag), ge - gs, ge - gs, strandBit, sink, dpCounter, &slot);
          if (r >= 0) gapMatch += r;
          else if (r == -1 && nref < GROUP_MAX_REFS) { refs[nref >> 1] |= slot << (16 * (nref & 1)); ++nref; }
          else again = true;  // keep walking: later gaps register their jobs too
        }
        pos = ge;
      }
      if (again) return 2;
      matchCnt = 2 * cov + 2 * gapMatch;
      if (nref) { *nRefs = nref; result = 3; }
    }
  }
  out.push(first, last + k - 1, first - diag, last - diag + k - 1, 2 * cov, matchCnt);
  return result;
}

// General group (several diagonals): restates GetOverlapsFromHits 1338-1551 and the chain walk 1697-1833.
// A[n] sorted copy of the hits, B[n] concordant hits, C[n] packs top (low 16) / link (high 16) of the LIS.
// Arr: work-array accessor (plain pointer, or LaneArr = LDS arrays interleaved over the lanes of a wavefront)
// second half of one diagonal run: B[0..m) = the run's hits nearest to the dominant diagonal, sorted by (allele offset, read offset);
// LIS over the read offsets, chain -> A[s..), hit lengths, seed-chain match count, candidate (SeqSet.hpp:352-436, 1512-1551, 1697-1833)
template <class Arr>
__device__ inline void chainRun(const ReadCtx &c, int k, int hitLenRequired, Arr A, Arr B, Arr C, int s, int m, int *gaScratch, int gaMax, CandOut &out,
                                unsigned int *dpCounter, unsigned long long *errFlags, bool *needScratch, const GapSink *sink, int strandBit, bool chainReady = false) {
    int ret, lenR, lenS;
    if (!t1k_run_lis(A, B, C, s, m, k, hitLenRequired, &ret, &lenR, &lenS, chainReady)) return;
    // seed-chain match count (1697-1833).  With a sink the alignments are registered in the read-end's memo instead of being
    // run here; the candidate then carries the memo slots (k_general_finish adds their match counts).
    uint32_t refs[3] = {0, 0, 0};
    int nref = 0;
    auto gapM = [&](int ra, int ga, int lp, int lt) -> int {
      if (!sink) return gapMatches(c, ra, ga, lp, lt, gaScratch, gaMax, dpCounter, errFlags, needScratch);
      if (lp <= 0 || lt <= 0) return 0;
      const int diff = lt > lp ? lt - lp : lp - lt;
      if (diff > 4) { *needScratch = true; return 0; }
      uint32_t slot = 0;
      const int r = gapMatchesCached<true>(c, ra, c.goff + ga, lp, lt, strandBit, *sink, dpCounter, &slot);
      if (r >= 0) return r;
      if (r == -1 && nref < GROUP_MAX_REFS) { refs[nref >> 1] |= slot << (16 * (nref & 1)); ++nref; return 0; }
      if (dpCounter) ++*dpCounter;
      return gapAlign(c, ra, c.goff + ga, lp, lt);
    };
    int matchCnt = 2 * k;
    for (int i = 1; i < ret; ++i) {
      int pa = (int)(A[s + i - 1] & 0xFFF), pb = (int)(A[s + i - 1] >> 12), qa = (int)(A[s + i] & 0xFFF), qb = (int)(A[s + i] >> 12);
      bool sameDiag = (pb - pa) == (qb - qa);
      bool readOv = pa + k - 1 >= qa, seqOv = pb + k - 1 >= qb;
      if (sameDiag) {
        if (readOv) matchCnt += 2 * (qa - pa);
        else matchCnt += 2 * k + 2 * gapM(pa + k, pb + k, qa - (pa + k), qb - (pb + k));
      } else {
        if (readOv && !seqOv) matchCnt += 2 * (qa - pa);
        else if (!readOv && seqOv) matchCnt += 2 * (qb - pb);
        else if (readOv && seqOv) matchCnt += 2 * ((qa - pa) < (qb - pb) ? (qa - pa) : (qb - pb));
        else matchCnt += 2 * k + 2 * gapM(pa + k, pb + k, qa - (pa + k), qb - (pb + k));
      }
    }
    int rs = (int)(A[s] & 0xFFF), ss = (int)(A[s] >> 12);
    int re = (int)(A[s + ret - 1] & 0xFFF) + k - 1, se = (int)(A[s + ret - 1] >> 12) + k - 1;
    out.push(rs, re, ss, se, 2 * lenR, matchCnt);
    out.setRefs(refs, nref);
}

template <class Arr>
__device__ inline void groupGeneral(const uint32_t *h, int n, const ReadCtx &c, int k, int radius, int hitLenRequired, Arr A, Arr B,
                                     Arr C, int *gaScratch, int gaMax, CandOut &out, unsigned int *dpCounter, unsigned long long *errFlags, bool *needScratch,
                                     const GapSink *sink = nullptr, int strandBit = 0) {
  // insertion sort into A
  for (int i = 0; i < n; ++i) {
    uint32_t x = h[i];
    int j = i - 1;
    while (j >= 0 && hitKeyLess(x, A[j])) { A[j + 1] = A[j]; --j; }
    A[j + 1] = x;
  }
  for (int s = 0; s < n;) {
    auto diagOf = [](uint32_t x) { return (int)(x & 0xFFF) - (int)(x >> 12); };
    int curDiff = diagOf(A[s]), curCnt = 1, domCnt = 0, dominant = 0;
    int e = s + 1;
    for (; e < n; ++e) {
      int d = diagOf(A[e]) - diagOf(A[e - 1]);
      if (d < 0) d = -d;
      if (d > radius) break;
      if (d == 0) ++curCnt;
      else {
        if (curCnt > domCnt) { dominant = curDiff; domCnt = curCnt; }
        curDiff = diagOf(A[e]); curCnt = 1;
      }
    }
    if (curCnt > domCnt) dominant = curDiff;
    if (e - s < 3 || (e - s) * k < hitLenRequired) { s = e; continue; }
    // nearest-to-dominant filter per read offset (1437-1456)
    int m = 0;
    for (int q = s; q < e; ++q) {
      int a = (int)(A[q] & 0xFFF);
      int dq = diagOf(A[q]) - dominant; if (dq < 0) dq = -dq;
      bool keep = true;
      for (int r = s; r < e; ++r) {
        if ((int)(A[r] & 0xFFF) != a) continue;
        int dr = diagOf(A[r]) - dominant; if (dr < 0) dr = -dr;
        if (dr < dq) { keep = false; break; }
      }
      if (keep) {  // insertion by (alleleOff, readOff) == packed value order (CompSortPairBInc)
        uint32_t x = A[q];
        int j = m - 1;
        while (j >= 0 && x < B[j]) { B[j + 1] = B[j]; --j; }
        B[j + 1] = x;
        ++m;
      }
    }
    chainRun(c, k, hitLenRequired, A, B, C, s, m, gaScratch, gaMax, out, dpCounter, errFlags, needScratch, sink, strandBit);
    s = e;
  }
}

// A multi-diagonal group whose hit list k_near_hits found to be a chain already (two diagonals, the hits of one entirely before the
// other's on the read AND on the allele; written in that order): one diagonal run (the diagonals lie within `radius`), every read offset
// occurs once so the nearest-to-dominant filter keeps everything, the order by allele offset is the order given, its read offsets ascend
// strictly so the LIS is the whole list, no allele offset repeats.  What is left of GetOverlapsFromHits are the length tests and the
// chain walk -- the same code as the general path runs after its sorts (SeqSet.hpp:1400-1405, 1468, 1512-1551, 1697-1833).
template <class Arr>
__device__ inline void groupSimple(const uint32_t *h, int n, const ReadCtx &c, int k, int hitLenRequired, Arr A, CandOut &out, unsigned int *dpCounter,
                                   unsigned long long *errFlags, bool *needScratch, const GapSink *sink, int strandBit) {
  for (int i = 0; i < n; ++i) A[i] = h[i];
  if (n < 3 || n * k < hitLenRequired) return;
  chainRun(c, k, hitLenRequired, A, A, A, 0, n, nullptr, 0, out, dpCounter, errFlags, needScratch, sink, strandBit, true);
}

// key of the strand vote: _overlap::operator< with similarity == 0 (SeqSet.hpp:103-127, 1623-1627); smaller = better
struct VoteKey {
  uint64_t hi, lo;
  __device__ bool operator<(const VoteKey &o) const { return hi != o.hi ? hi < o.hi : lo < o.lo; }
};
__device__ __forceinline__ VoteKey voteKey(int matchCnt0, int rs, int re, uint32_t allele, int strandPlus, int ss, int se) {
  VoteKey k;
  k.hi = ((uint64_t)(4095 - matchCnt0) << 40) | ((uint64_t)(4095 - (re - rs)) << 26) | ((uint64_t)allele << 1) | (uint64_t)strandPlus;
  k.lo = ((uint64_t)rs << 52) | ((uint64_t)re << 40) | ((uint64_t)ss << 20) | (uint64_t)se;
  return k;
}


__device__ __forceinline__ ReadCtx makeCtx(const ChainArgs &P, uint32_t re, int pass, uint32_t allele) {
  const int S = P.reads.S;
  ReadCtx c{P.reads.bases + ((uint64_t)re * 2 + pass) * S, P.reads.nmask + ((uint64_t)re * 2 + pass) * S, (int)P.reads.len[re], P.ref.bases, P.ref.nmask,
            (int64_t)P.ref.alleleOff[allele], (int)P.ref.alleleLen[allele], P.ref.anyN != 0};
  if (P.ref.basesT) c.gT = P.ref.basesT + (uint64_t)P.ref.blockT[allele >> 6] + (allele & 63u);
  return c;
}

// ------------------------------------------------------------------------------------------------------------------
// K2 / K4: single-diagonal chain, one lane per group record
// record words: 0 re|strand, 1 allele, 2 diagonal + stray counts, 3.. M   -> after chaining: 2 = state, 3..5 packed candidate (3 = side-arena base for
// multi-diagonal groups), 6..7 memo slots still to be added
// ------------------------------------------------------------------------------------------------------------------
// MODE 0: all records, closed form only (the rest -> slow list; multi-diagonal groups -> general list)
// MODE 1: slow list: gap walk, alignments registered in the memo (-> finish list / retry list)
// MODE 2: retry list after k_dp_dense: alignments from the memo or inline
// MODE 1 and 2 read their list's length at nDev (the total word k_arena_compact left) and stride over the list, so a grid sized from an
// estimate (t1k_run_chain) covers whatever the device counted; nItems is ignored.  MODE 0 (no list: blockIdx.y = arena stripe, its length
// from the stripe's cursor) is the straight-line form, one record per thread over a grid that covers what a stripe CAN hold: the striding
// loop costs the closed-form pass 16 VGPRs and with them a wavefront per SIMD (78 -> 94), and workgroups beyond the cursor end at once.
template <int NW, int MODE>
__global__ __launch_bounds__(WG) void k_chain_fast(ChainArgs P, const uint32_t *list, uint32_t nItems, const unsigned long long *nDev) {
  constexpr bool DEFER = MODE != 2;
  constexpr bool LOOP = MODE != 0;
  unsigned int dpLocal = 0, fastLocal = 0;
  if (nDev && P.counters[T1K_CTR_ERR]) return;  // an arena overflowed earlier in this submission: the range runs again, nothing of this pass is kept
  // list mode: 1-D grid over a dense list of record indices; all records: blockIdx.y = arena segment, blockIdx.x strides over the segment
  const uint32_t limit = list ? (nDev ? (uint32_t)*nDev : nItems)
                              : (uint32_t)min(*t1k_arena_cursor(P.counters, T1K_AR_GROUPS, blockIdx.y), (unsigned long long)P.groupSegCap);
  const uint32_t step = gridDim.x * WG;
#pragma unroll 1
  for (uint32_t base = blockIdx.x * WG; base < limit; base += step) {  // (lists hold fewer than 2^32 - step entries)
  int kind = 0;
  uint32_t gi = 0;
  const uint32_t gid = base + threadIdx.x;
  const bool valid = gid < limit;
  if (valid) gi = list ? list[gid] : blockIdx.y * P.groupSegCap + gid;
  if (valid) {
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    constexpr int RW = NW == 5 ? 8 : 16;
    uint32_t rv[RW];  // the record, fetched as 16-byte pieces
#pragma unroll
    for (int w = 0; w < RW / 4; ++w) {
      const uint4 q4 = ((const uint4 *)rec)[w];
      rv[4 * w] = q4.x; rv[4 * w + 1] = q4.y; rv[4 * w + 2] = q4.z; rv[4 * w + 3] = q4.w;
    }
    const uint32_t re = rv[0] & 0x7FFFFFFFu, allele = rv[1];
    const int pass = (rv[0] >> 31) ? 0 : 1;
    const bool general = recIsGeneral(rv[2]);
    if (general) kind = 4;
    else {
      uint32_t Mw[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) Mw[w] = rv[3 + w];
      ReadCtx c = makeCtx(P, re, pass, allele);
      // (the transposed copy pays where the lanes hold consecutive alleles: the pass over ALL records.  The gap walk's list is a scattered 40 % of them --
      // measured with the copy: its fabric traffic went UP by a third, six lines a lane instead of one or two; profiles/r06_callC_*.log)
      if (MODE != 0) c.gT = nullptr;
      uint32_t cbuf[3];
      CandOut out{cbuf, 0};
      const GapSink sink{P.memo + (uint64_t)re * GAP_CACHE, P.jobStr, P.counters, re * GAP_CACHE, P.jobSegCap, T1K_AR_JOBS};
      uint32_t refs[2] = {0, 0};
      int nRefs = 0;
      kind = groupFastPath<NW, DEFER, MODE == 0>(Mw, recDiag(rv[2]), c, P.ref.alleleHasN[allele] != 0, P.k, P.hitLenRequired, P.sim, out, &dpLocal, pass, sink, refs, &nRefs, P.earlyPrune);
      if (kind == 3) {  // matchCnt lacks the registered alignments: k_collect adds them from the memo
        // words 2..7: state (= number of memo slots to add), candidate, slots
        ((uint2 *)rec)[1] = make_uint2((uint32_t)nRefs, cbuf[0]);
        ((uint2 *)rec)[2] = make_uint2(cbuf[1], cbuf[2]);
        ((uint2 *)rec)[3] = make_uint2(refs[0], refs[1]);
      } else if (kind == 1) {
        ++fastLocal;
        if (out.n) { ((uint2 *)rec)[1] = make_uint2(REC_DONE | 1u, cbuf[0]); ((uint2 *)rec)[2] = make_uint2(cbuf[1], cbuf[2]); }
        else if (MODE != 0) rec[2] = REC_DONE;
        // (MODE 0, no candidate -- six in ten groups: the record is left as seeding wrote it.  Word 2 still holds the diagonal word: neither REC_DONE nor a
        // pending count (it is at least 2^20), which k_collect reads as "no candidate".  Round 6: a 4-byte store into a record nobody reads again was a
        // 32-byte write on the fabric, 0.19 TB per 10 M-pair step)
      }
    }
  }
  // list appends: one atomic per wavefront, list and arena segment (a full segment shows in its cursor; the host fails the batch)
  if (kind == 2) { const uint32_t q = t1k_arena_append(P.counters, T1K_AR_RETRY, P.listSegCap); if (q != T1K_ARENA_FULL) P.retryStr[q] = gi; }
  if (kind == 3) { const uint32_t q = t1k_arena_append(P.counters, T1K_AR_FINISH, P.listSegCap); if (q != T1K_ARENA_FULL) P.finishStr[q] = gi; }
  if (kind == 4) { const uint32_t q = t1k_arena_append(P.counters, T1K_AR_GENERAL, P.rareSegCap); if (q != T1K_ARENA_FULL) P.generalStr[q] = gi; }
  if (kind == 5) { const uint32_t q = t1k_arena_append(P.counters, T1K_AR_SLOW, P.listSegCap); if (q != T1K_ARENA_FULL) P.slowStr[q] = gi; }
  if (!LOOP) break;
  }
  t1k_stat_add(P.counters, T1K_STAT_DP, dpLocal);
  t1k_stat_add(P.counters, T1K_STAT_FAST, fastLocal);
}

// K3: one lane per registered alignment
__global__ __launch_bounds__(WG) void k_dp_dense(ChainArgs P, const uint32_t *jobs, uint32_t nJobs, const unsigned long long *nDev) {
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nJobs = (uint32_t)*nDev; }
  unsigned int dpLocal = 0;
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nJobs; q += gridDim.x * blockDim.x) {
    const uint32_t tag = jobs[q];
    const uint32_t re = tag / GAP_CACHE;
    unsigned long long *slot = P.memo + tag;
    const unsigned long long e = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int sb = (int)(e & 1), d = (int)((e >> 1) & 0xF) - 4, lp = (int)((e >> 5) & 0x1FF), readPos = (int)((e >> 14) & 0x7FF);
    const int S = P.reads.S;
    ReadCtx c{P.reads.bases + ((uint64_t)re * 2 + sb) * S, P.reads.nmask + ((uint64_t)re * 2 + sb) * S, 0, P.ref.bases, P.ref.nmask, 0, 0, P.ref.anyN != 0};
    const int m = gapAlign<true>(c, readPos, GAP_GPOS(e), lp, lp + d);  // (lengths as gapMatchesCached registered them)
    ++dpLocal;
    __hip_atomic_store(slot, (e & ~(GAP_PENDING << 25)) | ((unsigned long long)m << 25), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  t1k_stat_add(P.counters, T1K_STAT_DP, dpLocal);
}

// re-derive the hit list of one (read-end, strand, allele) group from the used posting lists kept by k_seed_groups:
// the allele's postings are a contiguous run of each list (lists are sorted by allele, then offset)
__device__ inline int gatherHits(const ChainArgs &P, uint32_t re, int pass, uint32_t allele, uint32_t *h, int cap) {
  const int maxK = (int)P.maxK;
  const uint32_t nPlus = P.usedCount[2 * re], nMinus = P.usedCount[2 * re + 1];
  const uint32_t b = pass == 0 ? 0 : nPlus, e = pass == 0 ? nPlus : nPlus + nMinus;
  const uint32_t *uo = P.usedOut + (uint64_t)re * maxK * 4;
  int n = 0;
  for (uint32_t u = b; u < e; ++u) {
    const uint32_t rOff = uo[4 * u], st = uo[4 * u + 1], ln = uo[4 * u + 2];
    uint32_t l = 0, r = ln;
    while (l < r) { uint32_t m = (l + r) >> 1; if (P.ref.kPost[st + m].allele < allele) l = m + 1; else r = m; }
    for (; l < ln; ++l) {
      const T1kPosting pst = P.ref.kPost[st + l];
      if (pst.allele != allele) break;
      if (n < cap) h[n] = (pst.offset << 12) | rOff;
      ++n;
    }
  }
  return n;
}

#define GENERAL_SMALL 32   // hits per group handled one lane per group (k_chain_general)
#define WAVE_CAP 4096      // ... one wavefront per group with the work arrays in LDS (k_chain_wave); beyond: k_chain_big
// K5a: hit lists of the multi-diagonal groups.  One wavefront per group: the lanes share the read-end's used posting lists,
// each finds the allele's run in its lists (sorted by allele, then offset) and the hits are written to the hit arena;
// record word 4 = arena offset, word 5 = hit count (0xFFFFFFFF: handed to k_chain_big)
// ROUNDS: used lists of one strand over the 64 lanes (5: reads <= 320 bp; 16: up to T1K_LONG_READ_LEN)
// ------------------------------------------------------------------------------------------------------------------
// K5a': hit lists of the multi-diagonal groups WITHOUT the posting lists.  Most such groups have all their hits within `radius` diagonals
// of the reference diagonal (a read with an indel: every one of its ~2000 groups; an allele with a small indel under the read): far == 0
// in the record.  A hit is a posting (allele, b) of a USED list of read offset a: the read's k-mer at a equals the allele's at b, that
// k-mer of the allele was inserted (the `posted` bitmap of the index: valid + the reference's insert rule), and a's list is used (the
// read-end's used-offset mask).  All three are bit masks over the read offsets, per diagonal d = a - b -- so one lane rebuilds the hit
// list of a group from the packed read, ~7 words of the allele's text and of `posted`, with shifts and ANDs, for the 2 * radius + 1
// diagonals, instead of a wavefront bisecting ~130 posting lists (k_gather_general: 9 dependent loads a lane, 2.8 KB fetched a group).
// Checked, not assumed: the mask of the reference diagonal must equal the record's (which came from the postings themselves), and the
// hits on the other diagonals must number exactly the record's near count; anything else (far strays, a saturated count, windows at
// the ends of the packed text) leaves the group to k_gather_general.  Record word 5 = REC_NEAR_DONE marks a group done here.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t evenBits32(uint64_t x) {  // bit 2j of x -> bit j
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull; x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full; x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull; x = (x | (x >> 16)) & 0xFFFFFFFFull;
  return (uint32_t)x;
}
template <int NW>
__global__ __launch_bounds__(WG) void k_near_hits(ChainArgs P, uint32_t nItems, const unsigned long long *nDev) {
  constexpr int NQ = NW + 1;  // 64-bit words (32 positions each) of the per-position masks: one spare word for the k-mer's reach
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  for (uint32_t qb = blockIdx.x * WG; qb < nItems; qb += gridDim.x * WG) {
  const uint32_t q = qb + threadIdx.x;
  bool toWave = false;
  uint32_t gi = 0;
  if (q < nItems) {
    gi = P.generalList[q];
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    constexpr int RW = NW == 5 ? 8 : 16;
    uint32_t rv[RW];
#pragma unroll
    for (int w = 0; w < RW / 4; ++w) { const uint4 q4 = ((const uint4 *)rec)[w]; rv[4 * w] = q4.x; rv[4 * w + 1] = q4.y; rv[4 * w + 2] = q4.z; rv[4 * w + 3] = q4.w; }
    const uint32_t re = rv[0] & 0x7FFFFFFFu, allele = rv[1];
    const int pass = (rv[0] >> 31) ? 0 : 1;
    const int d0 = recDiag(rv[2]), k = P.k, R = P.radius;
    const uint32_t nearCnt = recNear(rv[2]);
    uint32_t onDiag = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) onDiag += __popc(rv[3 + w]);
    const int64_t goff = (int64_t)P.ref.alleleOff[allele];
    const int alleleLen = (int)P.ref.alleleLen[allele];
    const int64_t W0 = goff - d0 - R;  // global position under read offset 0 on the diagonal d0 + R
    const int64_t lastWord = (W0 >> 5) + NQ + 2;
    bool ok = recFar(rv[2]) == 0 && nearCnt > 0 && nearCnt < 31 && R <= 15 && W0 >= 0 && (uint64_t)lastWord < (P.ref.totalBases >> 5) + 7;
    uint32_t base = T1K_ARENA_FULL;
    const uint32_t n = onDiag + nearCnt;
    if (ok) { base = t1k_arena_alloc(P.counters, T1K_AR_GENHITS, n, P.genHitSegCap); ok = base != T1K_ARENA_FULL; }
    if (ok) {
      const int S = P.reads.S;
      const uint64_t *rb = P.reads.bases + ((uint64_t)re * 2 + pass) * S;
      const uint32_t *um = P.usedMask + ((uint64_t)re * 2 + pass) * T1K_USED_MASK_WORDS;
      uint64_t Rr[NQ], G[NQ + 2], PG[NQ + 2];
#pragma unroll
      for (int j = 0; j < NQ; ++j) Rr[j] = j < S ? rb[j] : 0ull;
      const uint64_t *gb = P.ref.bases + (W0 >> 5), *pb = P.ref.posted + (W0 >> 5);
#pragma unroll
      for (int j = 0; j < NQ + 2; ++j) { G[j] = gb[j]; PG[j] = pb[j]; }
      const int sh0 = (int)(W0 & 31);
      uint32_t w = base, cntNear = 0;
      bool same0 = false;
      int nearDiags = 0, d1 = 0;    // near diagonals that hold hits; the first one and its mask
      uint32_t M1[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) M1[j] = 0;
      for (int dl = -R; dl <= R; ++dl) {
        const int d = d0 + dl;
        const int o = sh0 + (R - dl);          // base offset of read position 0 inside G (0 .. 31 + 2R < 64)
        const bool up = o >= 32;
        const int bsh = (o & 31) * 2;
        uint64_t acc[NQ], pst[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const uint64_t lo = up ? G[j + 1] : G[j], hi = up ? G[j + 2] : G[j + 1];
          const uint64_t g = bsh ? ((lo >> bsh) | (hi << (64 - bsh))) : lo;
          const uint64_t x = g ^ Rr[j];
          acc[j] = ~(x | (x >> 1)) & 0x5555555555555555ull;   // bit 2p: the bases at position 32 j + p are equal
          const uint64_t pl = up ? PG[j + 1] : PG[j], ph = up ? PG[j + 2] : PG[j + 1];
          pst[j] = bsh ? ((pl >> bsh) | (ph << (64 - bsh))) : pl;
        }
        // acc(a) = AND over t < k of eq(a + t), by doubling (a shift by m positions = 2 m bits towards lower positions)
        auto andShifted = [&](int m) {
          const int b = 2 * m;
#pragma unroll
          for (int j = 0; j < NQ; ++j) { const uint64_t nx = j + 1 < NQ ? acc[j + 1] : 0ull; acc[j] &= (acc[j] >> b) | (nx << (64 - b)); }
        };
        {
          int have = 1;
          while (2 * have <= k) { andShifted(have); have *= 2; }
          if (have < k) andShifted(k - have);
        }
        // hits of this diagonal: equal k-mers, posted in the index, the read offset's list used, the k-mer inside THIS allele
        const int aLo = d > 0 ? d : 0, aHi = d + alleleLen - k;  // b = a - d in [0, alleleLen - k]
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          uint32_t m = evenBits32(acc[j] & pst[j]) & um[j];
          const int p0 = 32 * j;
          if (aLo > p0) m &= aLo - p0 >= 32 ? 0u : ~0u << (aLo - p0);
          if (aHi < p0 + 31) m &= aHi < p0 ? 0u : ~0u >> (31 - (aHi - p0));
          if (dl == 0) { if (j == 0) same0 = true; same0 = same0 && m == rv[3 + j]; continue; }
          if (m) {
            if (nearDiags == 0 || d1 != d) { ++nearDiags; if (nearDiags == 1) d1 = d; }
            if (nearDiags == 1) M1[j] = m;
          }
          cntNear += __popc(m);
          while (m) {
            const int p = __ffs((int)m) - 1;
            m &= m - 1;
            const uint32_t a = (uint32_t)(p0 + p);
            if (w < base + n) P.genHits[w] = ((uint32_t)((int)a - d) << 12) | a;
            ++w;
          }
        }
      }
      ok = same0 && cntNear == nearCnt;
      // two diagonals whose hits follow one another on the read and on the allele: the list IS its chain (groupSimple)
      bool simple = false;
      if (ok && P.nearSimple && nearDiags == 1 && n >= 3 && (int)n * k >= P.hitLenRequired) {
        int lo0 = -1, hi0 = -1, lo1 = -1, hi1 = -1;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          if (rv[3 + j]) { if (lo0 < 0) lo0 = 32 * j + __ffs((int)rv[3 + j]) - 1; hi0 = 32 * j + 31 - __clz((int)rv[3 + j]); }
          if (M1[j]) { if (lo1 < 0) lo1 = 32 * j + __ffs((int)M1[j]) - 1; hi1 = 32 * j + 31 - __clz((int)M1[j]); }
        }
        const bool first0 = hi0 < lo1 && hi0 - d0 < lo1 - d1, first1 = hi1 < lo0 && hi1 - d1 < lo0 - d0;
        if (first0 || first1) {
          simple = true;
          w = base;
          for (int part = 0; part < 2; ++part) {
            const bool zero = (part == 0) == first0;  // this part is the reference diagonal's
            const int dd = zero ? d0 : d1;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
              uint32_t m = zero ? rv[3 + j] : M1[j];
              while (m) {
                const int p = __ffs((int)m) - 1;
                m &= m - 1;
                const uint32_t a = (uint32_t)(32 * j + p);
                P.genHits[w++] = ((uint32_t)((int)a - dd) << 12) | a;
              }
            }
          }
        }
      }
      if (ok && simple) { rec[3] = base; rec[4] = n; rec[6] = 1u; toWave = n > 3 * GENERAL_SMALL; }
      else if (ok) {
        rec[6] = 0u;
        // ... and the reference diagonal's own hits, from the record's mask
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          uint32_t m = rv[3 + j];
          while (m) {
            const int p = __ffs((int)m) - 1;
            m &= m - 1;
            const uint32_t a = (uint32_t)(32 * j + p);
            P.genHits[w++] = ((uint32_t)((int)a - d0) << 12) | a;
          }
        }
        rec[3] = base; rec[4] = n;
        toWave = n > GENERAL_SMALL;
      }
    }
    rec[5] = ok ? REC_NEAR_DONE : 0u;
    if (!ok) rec[6] = 0u;
#ifdef T1K_NEAR_STATS
    {  // what the multi-diagonal groups are (profiles/r04_multidiag_classes.txt)
      int cls = T1K_NEAR_FALLBACK;
      if (recFar(rv[2]) != 0) cls = T1K_NEAR_FAR; else if (nearCnt == 31) cls = T1K_NEAR_SATURATED; else if (ok) cls = rec[6] == 1u ? (n > 96 ? T1K_NEAR_CHAIN_LARGE : T1K_NEAR_CHAIN_SMALL) : (n > 32 ? T1K_NEAR_NOCHAIN_LARGE : T1K_NEAR_NOCHAIN_SMALL);
      atomicAdd(&P.counters[T1K_WIN_NEAR_STATS + cls], 1ull);
    }
#endif
  }
  if (toWave) { const uint32_t wq = t1k_arena_append(P.counters, T1K_AR_WAVE, P.rareSegCap); if (wq != T1K_ARENA_FULL) P.waveStr[wq] = gi; }
  }
}

template <int ROUNDS>
__global__ __launch_bounds__(WG) void k_gather_general(ChainArgs P, uint32_t nItems, int skipDone, const unsigned long long *nDev) {
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * WG + threadIdx.x) >> 6, nWaves = gridDim.x * (WG / 64);
  const int maxK = (int)P.maxK;
  static_assert(ROUNDS * 64 >= GROUP_FAST_MAXLEN, "lists of one strand");
  for (uint32_t q = wave; q < nItems; q += nWaves) {
    const uint32_t gi = P.generalList[q];
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    if (skipDone && rec[5] == REC_NEAR_DONE) continue;  // k_near_hits wrote this group's hits (uniform over the wavefront)
    const uint32_t re = rec[0] & 0x7FFFFFFFu, allele = rec[1];
    const int pass = (rec[0] >> 31) ? 0 : 1;
    const uint32_t nPlus = P.usedCount[2 * re], nMinus = P.usedCount[2 * re + 1];
    const uint32_t b = pass == 0 ? 0 : nPlus, e = pass == 0 ? nPlus : nPlus + nMinus;
    const uint32_t *uo = P.usedOut + (uint64_t)re * maxK * 4;
    uint32_t first[ROUNDS], cnt[ROUNDS], mine = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const uint32_t u = b + lane + 64 * r;
      first[r] = 0; cnt[r] = 0;
      if (u < e) {
        const uint32_t st = uo[4 * u + 1], ln = uo[4 * u + 2], dr = uo[4 * u + 3];
        uint32_t l = 0, rr = ln;
        if (dr != T1K_NO_DIR) {  // a long list: its chunk directory narrows the search to the allele's chunk of T1K_SEED_CHUNK sequences
          const uint32_t *dir = P.ref.kDir + (uint64_t)dr * P.ref.kDirStride;
          const uint32_t ci = allele / T1K_SEED_CHUNK;
          l = dir[ci]; rr = dir[ci + 1];
        }
        while (l < rr) { uint32_t m = (l + rr) >> 1; if (P.ref.kPost[st + m].allele < allele) l = m + 1; else rr = m; }
        uint32_t c = 0;
        while (l + c < ln && P.ref.kPost[st + l + c].allele == allele) ++c;
        first[r] = st + l; cnt[r] = c; mine += c;
      }
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t y = __shfl_up(incl, o, 64); if (lane >= o) incl += y; }
    const uint32_t n = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 0) {
      if (n > WAVE_CAP) {  // k_chain_big gathers for itself
        const uint32_t bq = t1k_arena_append(P.counters, T1K_AR_BIG, P.rareSegCap);
        if (bq != T1K_ARENA_FULL) P.bigStr[bq] = gi;
        rec[4] = 0xFFFFFFFFu;
      } else {
        base = n ? t1k_arena_alloc(P.counters, T1K_AR_GENHITS, n, P.genHitSegCap) : 0u;
        rec[3] = base; rec[4] = n;
        if (n > GENERAL_SMALL) {  // one wavefront per group (k_chain_wave)
          const uint32_t wq = t1k_arena_append(P.counters, T1K_AR_WAVE, P.rareSegCap);
          if (wq != T1K_ARENA_FULL) P.waveStr[wq] = gi;
        }
      }
    }
    base = __shfl(base, 0, 64);
    if (n <= WAVE_CAP && base != T1K_ARENA_FULL) {
      uint32_t w = base + incl - mine;
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const uint32_t u = b + lane + 64 * r;
        if (cnt[r]) {
          const uint32_t rOff = uo[4 * u];
          for (uint32_t j = 0; j < cnt[r]; ++j) P.genHits[w++] = (P.ref.kPost[first[r] + j].offset << 12) | rOff;
        }
      }
    }
  }
}

// K5b: multi-diagonal groups with at most GENERAL_SMALL hits, one lane per group, 64-thread workgroups; the three work arrays
// live in LDS, interleaved over the lanes (24 KB).  Alignments go through the read-end's memo (registered now, run by
// k_dp_dense, added by k_general_finish); groups that need an alignment wider than the register band go to k_chain_big.
// useSimple: record word 6 = 1 marks a group whose hit list k_near_hits wrote as its chain (groupSimple: no sorts, no LIS, one array -- up
// to 3 * GENERAL_SMALL hits in the same LDS)
__global__ __launch_bounds__(64) void k_chain_general(ChainArgs P, uint32_t nItems, int useSimple, const unsigned long long *nDev) {
  __shared__ uint32_t sArr[3 * GENERAL_SMALL * 64];
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  unsigned int dpLocal = 0, genLocal = 0;
  for (uint32_t qb = blockIdx.x * 64; qb < nItems; qb += gridDim.x * 64) {  // (a lane's work arrays are its own: no barrier between the rounds)
  const uint32_t q = qb + threadIdx.x;
  uint32_t nHits = 0xFFFFFFFFu;
  bool simple = false;
  if (q < nItems) {
    const uint32_t *r0 = P.recs + (uint64_t)P.generalList[q] * P.recStride;
    nHits = r0[4];
    simple = useSimple && r0[5] == REC_NEAR_DONE && r0[6] == 1u;
  }
  if (nHits <= GENERAL_SMALL || (simple && nHits <= 3 * GENERAL_SMALL)) {
    const uint32_t gi = P.generalList[q];
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    const uint32_t re = rec[0] & 0x7FFFFFFFu, allele = rec[1];
    const int pass = (rec[0] >> 31) ? 0 : 1;
    ReadCtx c = makeCtx(P, re, pass, allele);
    const int n = (int)nHits;
    if (rec[3] == T1K_ARENA_FULL) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_STAGECAP);
    const uint32_t *hh = P.genHits + (rec[3] == T1K_ARENA_FULL ? 0u : rec[3]);
    bool needScratch = false;
    uint32_t cbuf[2 * GENERAL_SMALL + 6];  // a candidate needs >= 3 hits
    CandOut out{cbuf, 0, 6, GENERAL_SMALL / 3 + 1};
    const GapSink sink{P.memo + (uint64_t)re * GAP_CACHE, P.genJobStr, P.counters, re * GAP_CACHE, P.genJobSegCap, T1K_AR_GENJOBS};
    LaneArr A{sArr + threadIdx.x}, B{sArr + GENERAL_SMALL * 64 + threadIdx.x}, C{sArr + 2 * GENERAL_SMALL * 64 + threadIdx.x};
    if (simple) groupSimple(hh, n, c, P.k, P.hitLenRequired, A, out, &dpLocal, &P.counters[T1K_CTR_ERR], &needScratch, &sink, pass);
    else groupGeneral(hh, n, c, P.k, P.radius, P.hitLenRequired, A, B, C, nullptr, 0, out, &dpLocal, &P.counters[T1K_CTR_ERR], &needScratch, &sink, pass);
    if (needScratch) { const uint32_t b = t1k_arena_append(P.counters, T1K_AR_BIG, P.rareSegCap); if (b != T1K_ARENA_FULL) P.bigStr[b] = gi; }
    else {
      ++genLocal;
      uint32_t base = 0;
      if (out.n) {
        base = t1k_arena_alloc(P.counters, T1K_AR_GENCAND, (uint32_t)out.n, P.genCandSegCap);
        if (base == T1K_ARENA_FULL) { atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_STAGECAP); out.n = 0; base = 0; }
        for (int i = 0; i < 6 * out.n; ++i) P.genCand[(uint64_t)base * 6 + i] = cbuf[i];
      }
      rec[3] = base;
      rec[2] = REC_DONE | 0x40000000u | (uint32_t)out.n;  // bit30: candidates live in the side arena
    }
  }
  }
  t1k_stat_add(P.counters, T1K_STAT_DP, dpLocal);
  t1k_stat_add(P.counters, T1K_STAT_GENERAL, genLocal);
}

// K5b': multi-diagonal groups with GENERAL_SMALL < hits <= WAVE_CAP, one wavefront per group.  The quadratic steps of
// GetOverlapsFromHits (sort by diagonal, nearest-to-dominant filter, sort by allele offset; SeqSet.hpp:1338-1456) are spread
// over the lanes as rank sorts; the LIS and the chain walk of each diagonal run are done by lane 0 (chainRun).
// cap / above: this launch takes the groups with above < hits <= cap and has 3 * cap words of LDS (round 5: the list is run twice -- most of
// these groups hold a few dozen hits, and with room for WAVE_CAP of them a workgroup's 48 KB left three wavefronts on a compute unit)
__global__ __launch_bounds__(64) void k_chain_wave(ChainArgs P, uint32_t nItems, const unsigned long long *nDev, uint32_t cap, uint32_t above) {
  extern __shared__ uint32_t sW[];  // A | B | C, cap words each
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  uint32_t *A = sW, *B = sW + cap, *C = sW + 2 * cap;
  const int lane = threadIdx.x;
  unsigned int dpLocal = 0, genLocal = 0;
  auto diagOf = [](uint32_t x) { return (int)(x & 0xFFF) - (int)(x >> 12); };
  for (uint32_t q = blockIdx.x; q < nItems; q += gridDim.x) {
    const uint32_t gi = P.waveList[q];
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    const uint32_t re = rec[0] & 0x7FFFFFFFu, allele = rec[1];
    const int pass = (rec[0] >> 31) ? 0 : 1;
    const int n = (int)rec[4];
    if ((uint32_t)n <= above || (uint32_t)n > cap) continue;  // (the other launch's; uniform over the wavefront)
    const bool lost = rec[3] == T1K_ARENA_FULL;
    if (lost && lane == 0) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_STAGECAP);
    const uint32_t *hh = P.genHits + (lost ? 0u : rec[3]);
    ReadCtx c = makeCtx(P, re, pass, allele);
    const int k = P.k;
    __syncthreads();  // the previous group's arrays are dead
    for (int i = lane; i < n; i += 64) C[i] = hh[i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {  // rank sort by (diagonal, allele offset, read offset): CompSortHitCoordDiff (266-274)
      const uint32_t x = C[i];
      int r = 0;
      for (int j = 0; j < n; ++j) r += hitKeyLess(C[j], x) ? 1 : 0;
      A[r] = x;
    }
    __syncthreads();
    bool needScratch = false;
    uint32_t cbuf[192];  // lane 0: at most 32 candidates are kept per group
    CandOut out{cbuf, 0, 6, 32};
    const GapSink sink{P.memo + (uint64_t)re * GAP_CACHE, P.genJobStr, P.counters, re * GAP_CACHE, P.genJobSegCap, T1K_AR_GENJOBS};
    for (int s = 0; s < n;) {  // wave-uniform: every lane tracks the run boundaries
      int curDiff = diagOf(A[s]), curCnt = 1, domCnt = 0, dominant = 0;
      int e = s + 1;
      for (; e < n; ++e) {
        int d = diagOf(A[e]) - diagOf(A[e - 1]);
        if (d < 0) d = -d;
        if (d > P.radius) break;
        if (d == 0) ++curCnt;
        else {
          if (curCnt > domCnt) { dominant = curDiff; domCnt = curCnt; }
          curDiff = diagOf(A[e]); curCnt = 1;
        }
      }
      if (curCnt > domCnt) dominant = curDiff;
      if (e - s < 3 || (e - s) * k < P.hitLenRequired) { s = e; continue; }
      // nearest-to-dominant filter per read offset (1437-1456): keep flags in C
      int mine = 0;
      for (int qq = s + lane; qq < e; qq += 64) {
        const int a = (int)(A[qq] & 0xFFF);
        int dq = diagOf(A[qq]) - dominant; if (dq < 0) dq = -dq;
        bool keep = true;
        for (int r = s; r < e; ++r) {
          if ((int)(A[r] & 0xFFF) != a) continue;
          int dr = diagOf(A[r]) - dominant; if (dr < 0) dr = -dr;
          if (dr < dq) { keep = false; break; }
        }
        C[qq] = keep ? 1u : 0u;
        mine += keep ? 1 : 0;
      }
      for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
      const int m = mine;
      __syncthreads();
      for (int qq = s + lane; qq < e; qq += 64) {  // kept hits by (allele offset, read offset) == packed value (CompSortPairBInc)
        if (!C[qq]) continue;
        const uint32_t x = A[qq];
        int r = 0;
        for (int t = s; t < e; ++t) r += (C[t] && A[t] < x) ? 1 : 0;
        B[r] = x;
      }
      __syncthreads();
      if (lane == 0) chainRun(c, k, P.hitLenRequired, A, B, C, s, m, nullptr, 0, out, &dpLocal, &P.counters[T1K_CTR_ERR], &needScratch, &sink, pass);
      __syncthreads();
      s = e;
    }
    if (lane == 0) {
      if (out.overflow) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_BIGGROUP);
      if (needScratch) { const uint32_t b = t1k_arena_append(P.counters, T1K_AR_BIG, P.rareSegCap); if (b != T1K_ARENA_FULL) P.bigStr[b] = gi; }
      else {
        ++genLocal;
        uint32_t base = 0;
        if (out.n) {
          base = t1k_arena_alloc(P.counters, T1K_AR_GENCAND, (uint32_t)out.n, P.genCandSegCap);
          if (base == T1K_ARENA_FULL) { atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_STAGECAP); out.n = 0; base = 0; }
          for (int i = 0; i < 6 * out.n; ++i) P.genCand[(uint64_t)base * 6 + i] = cbuf[i];
        }
        rec[3] = base;
        rec[2] = REC_DONE | 0x40000000u | (uint32_t)out.n;
      }
    }
  }
  t1k_stat_add(P.counters, T1K_STAT_DP, dpLocal);
  t1k_stat_add(P.counters, T1K_STAT_GENERAL, genLocal);
}

// K5c: add the memo's match counts to the candidates of the multi-diagonal groups
__global__ __launch_bounds__(WG) void k_general_finish(ChainArgs P, uint32_t nItems, const unsigned long long *nDev) {
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nItems; q += gridDim.x * blockDim.x) {
  const uint32_t *rec = P.recs + (uint64_t)P.generalList[q] * P.recStride;
  if ((rec[2] & (REC_DONE | 0x40000000u)) != (REC_DONE | 0x40000000u)) continue;  // not chained yet (waits for k_chain_big)
  const uint32_t re = rec[0] & 0x7FFFFFFFu, nc = rec[2] & 0x3FFFFFFFu;
  const unsigned long long *memo = P.memo + (uint64_t)re * GAP_CACHE;
  for (uint32_t j = 0; j < nc; ++j) {
    uint32_t *g = P.genCand + ((uint64_t)rec[3] + j) * 6;
    const int nref = (int)((g[0] >> 24) & 0xF);
    if (!nref) continue;
    uint32_t sum = 0;
    for (int i = 0; i < nref; ++i) {
      const uint32_t slot = (g[3 + (i >> 1)] >> (16 * (i & 1))) & 0xFFFFu;
      const unsigned long long e = __hip_atomic_load(&memo[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t v = GAP_VAL(e);
      if (v == GAP_PENDING) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_MEMO);
      sum += v;
    }
    g[2] += (2u * sum) << 20;
    g[0] &= 0x00FFFFFFu;
  }
  }
}

// what is left: groups with more than WAVE_CAP hits, or a gap whose two sides differ by more than the register band covers.
// One working lane per 64-thread workgroup; sort arrays in HBM scratch, the rows of the general alignment in LDS.
__global__ __launch_bounds__(64) void k_chain_big(ChainArgs P, uint32_t nItems, const unsigned long long *nDev) {
  __shared__ int sGa[GA_SCRATCH_INTS];
  if (threadIdx.x != 0) return;
  if (nDev) { if (P.counters[T1K_CTR_ERR]) return; nItems = (uint32_t)*nDev; }
  const uint32_t t = blockIdx.x, nT = gridDim.x;
  uint32_t *mine = P.bigScratch + (uint64_t)t * (4 * BIG_CAP);
  unsigned int dpLocal = 0;
  for (uint32_t q = t; q < nItems; q += nT) {
    const uint32_t gi = P.bigList[q];
    uint32_t *rec = P.recs + (uint64_t)gi * P.recStride;
    const uint32_t re = rec[0] & 0x7FFFFFFFu, allele = rec[1];
    const int pass = (rec[0] >> 31) ? 0 : 1;
    ReadCtx c = makeCtx(P, re, pass, allele);
    uint32_t *hh = mine + 3 * BIG_CAP;
    const int n = gatherHits(P, re, pass, allele, hh, BIG_CAP);
    if (n > BIG_CAP) { atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_BIGGROUP); rec[2] = REC_DONE; continue; }
    bool dummy = false;
    uint32_t cbuf[192];  // at most 32 candidates are kept per group
    CandOut o2{cbuf, 0, 6, 32};
    groupGeneral(hh, n, c, P.k, P.radius, P.hitLenRequired, mine, mine + BIG_CAP, mine + 2 * BIG_CAP, sGa, GA_BIG_MAX, o2, &dpLocal,
                 &P.counters[T1K_CTR_ERR], &dummy);
    if (o2.overflow) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_BIGGROUP);
    uint32_t base = 0;
    if (o2.n) {
      base = t1k_arena_alloc(P.counters, T1K_AR_GENCAND, (uint32_t)o2.n, P.genCandSegCap);
      if (base == T1K_ARENA_FULL) { atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_STAGECAP); o2.n = 0; base = 0; }
      for (int i = 0; i < 6 * o2.n; ++i) P.genCand[(uint64_t)base * 6 + i] = cbuf[i];
    }
    rec[3] = base;
    rec[2] = REC_DONE | 0x40000000u | (uint32_t)o2.n;
    atomicAdd(&P.counters[T1K_CTR_BIG_GROUPS], 1ull);
  }
  if (dpLocal) atomicAdd(&P.counters[T1K_CTR_DP], (unsigned long long)dpLocal);
}

// ------------------------------------------------------------------------------------------------------------------
// K6: strand vote + copy-out, one workgroup per read-end
// ------------------------------------------------------------------------------------------------------------------

// the similarity / low-complexity filter on a seed candidate (SeqSet.hpp:1838-1845, 1894-1908): candidates that fail it take no
// further part (they only counted for the strand vote), so they are never copied out.  The low-complexity test (SeqSet.hpp:458-485)
// asks for the number of A / C / G / T among the non-N bases of a read span; a workgroup works on one read-end, so it keeps prefix
// counts of the four bases for both strands in LDS (sBaseCnt[strand][base][p] = occurrences in [0, p)) and a span costs eight reads.
template <int MAXLEN>
__device__ __forceinline__ bool lowComplexityFromCounts(const uint16_t (*cnt)[MAXLEN + 1], int rs, int re) {
  const int L = re - rs + 1;
  int low = 0, lowTotal = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int c = (int)cnt[b][re + 1] - (int)cnt[b][rs];
    if (c <= 2) { ++low; lowTotal += c; }
  }
  if (lowTotal * 7 >= L) return false;
  return low >= 2;
}
template <int MAXLEN>
__device__ __forceinline__ bool keepCandidate(const ChainArgs &P, const uint16_t (*baseCnt)[4][MAXLEN + 1], int plus, uint32_t w0, uint32_t w1, uint32_t w2) {
  const int rs = (int)(w0 & 0xFFF), rend = (int)((w0 >> 12) & 0xFFF), ss = (int)(w1 & 0xFFFFF), se = (int)(w2 & 0xFFFFF);
  const int matchCnt = (int)(w2 >> 20);
  const double sim = (double)matchCnt / (double)(se - ss + 1 + rend - rs + 1);
  if (sim < P.sim) return false;
  if (lowComplexityFromCounts<MAXLEN>(baseCnt[plus ? 0 : 1], rs, rend)) return !(0.0 < P.sim);  // similarity becomes 0
  return true;
}

// A single-diagonal group whose candidate still waits for registered alignments (record word 2 = their number, words 6..7 their memo
// slots; k_dp_dense has run them): the match counts are added here, where the record is read anyway -- rounds 1-3 fetched and
// rewrote those records in a launch of its own (1.9 GB fetched per range for scattered 32-byte records).  Returns the candidate's word 2.
__device__ __forceinline__ uint32_t pendingMatchWord(const ChainArgs &P, uint32_t re, uint32_t nRefs, uint32_t w2, uint32_t s0, uint32_t s1) {
  const unsigned long long *memo = P.memo + (uint64_t)re * GAP_CACHE;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < nRefs; ++i) {
    const uint32_t slot = ((i >> 1 ? s1 : s0) >> (16 * (i & 1))) & 0xFFFFu;
    const unsigned long long e = __hip_atomic_load(&memo[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t v = GAP_VAL(e);
    if (v == GAP_PENDING) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_MEMO);  // cannot happen: every registered job is run by k_dp_dense
    sum += v;
  }
  return w2 + ((2u * sum) << 20);
}

// MAXLEN: longest read of the launch (T1K_MAX_READ_LEN, or T1K_LONG_READ_LEN for a window with longer reads: 16 KB of prefix counts)
#if T1K_COLLECT_WAVES > 0
#define T1K_COLLECT_ATTR T1K_WAVES_ATTR_(T1K_COLLECT_WAVES)
#else
#define T1K_COLLECT_ATTR
#endif
template <int MAXLEN>
__global__ __launch_bounds__(WG) T1K_COLLECT_ATTR void k_collect(ChainArgs P) {
  __shared__ uint32_t warpSums[4];
  __shared__ uint16_t sBaseCnt[2][4][MAXLEN + 1];
  __shared__ uint64_t sVote[2 * WG];
  uint64_t *sVoteHi = sVote, *sVoteLo = sVote + WG;
  __shared__ uint32_t sBase;
  // the read-end's chunk table (at most 2 x 256 + 2 chunks: the launcher refuses references with more seeding chunks): record index of
  // each chunk's first record, prefix of the chunk lengths, the chunks' strands; the copy-out pass's own prefix lives in the vote arrays,
  // which are dead by then
  constexpr int MAXCH = 2 * 256 + 2;
  __shared__ uint32_t sCs[MAXCH], sPre[MAXCH + 1], sNCh;
  __shared__ uint8_t sChPlus[MAXCH];
  uint32_t *sPreW = (uint32_t *)sVote;
  static_assert(sizeof(uint64_t) * 2 * WG >= sizeof(uint32_t) * (MAXCH + 1), "the copy-out prefix does not fit the vote arrays");
  // one bit per group record of the read-end (in chunk order): "the copy-out pass has to look at this record" -- its only candidate passed
  // the filter, or it holds several (multi-diagonal groups).  The vote pass reads every record anyway; the copy-out pass then loads the
  // 40 % that hold something instead of all of them again (records beyond the bitmap's reach are simply looked at).
  constexpr uint32_t KEEP_BITS = 65536;
  __shared__ uint32_t sKeepBits[KEEP_BITS / 32];
  const int tid = threadIdx.x;
  const uint32_t stride = P.recStride;
  if (P.devDriven && P.counters[T1K_CTR_ERR]) return;  // an arena overflowed earlier in this submission: the range runs again
  __shared__ uint32_t sNextRe;  // read-ends handed out one at a time (device counter): their group counts differ by orders of magnitude
  uint32_t hoNext = 0, hoLeft = 0;
  for (;;) {
    __syncthreads();
    if (tid == 0) {  // (T1K_RE_HANDOUT read-ends per atomic on the hand-out word: round 6)
      if (hoLeft == 0) { hoNext = (uint32_t)atomicAdd(&P.counters[T1K_CTR_COLLECT_HANDOUT], (unsigned long long)T1K_COLLECT_HANDOUT); hoLeft = T1K_COLLECT_HANDOUT; }
      sNextRe = hoNext++; --hoLeft;
    }
    __syncthreads();
    const uint32_t re = sNextRe;
    if (re >= P.reads.nReadEnds) break;
    const uint32_t *cs = P.chunkStart + (uint64_t)re * P.maxChunks, *cc = P.chunkCount + (uint64_t)re * P.maxChunks;
    for (uint32_t i = tid; i < KEEP_BITS / 32; i += WG) sKeepBits[i] = 0;
    {  // prefix counts of the four bases (non-N positions only) of both strands of this read-end
      const int len = (int)P.reads.len[re], S = P.reads.S;
      for (int idx = tid; idx < 2 * (len + 1); idx += WG) {
        const int strand = idx / (len + 1), p = idx - strand * (len + 1);
        const uint64_t *rb = P.reads.bases + ((uint64_t)re * 2 + strand) * S, *rn = P.reads.nmask + ((uint64_t)re * 2 + strand) * S;
        int c[4] = {0, 0, 0, 0};
        for (int o = 0; o < p; o += 32) {
          const uint64_t x = rb[o >> 5], nn = rn[o >> 5];
          const uint64_t valid = T1K_EVEN & ~nn & t1k_lowmask(p - o);
          const uint64_t lo = x & T1K_EVEN, hi = (x >> 1) & T1K_EVEN;
          c[0] += __popcll(~lo & ~hi & valid); c[1] += __popcll(lo & ~hi & valid); c[2] += __popcll(~lo & hi & valid); c[3] += __popcll(lo & hi & valid);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) sBaseCnt[strand][b][p] = (uint16_t)c[b];
      }
      __syncthreads();
    }
    // The chunk table of the read-end (runs of records per strand and allele chunk, recorded densely) as a prefix over ONE record index r:
    // both passes below walk r in strides of the workgroup, so a pass issues ceil(records / 256) rounds of loads -- chunk by chunk it was
    // one or two rounds per chunk, ten to twenty chunks a read-end, each behind a dependent load of the chunk's start and count.
    if (tid < 64) {
      uint32_t carry = 0, nDense = 0;
      bool open = true;
      if (tid == 0) sPre[0] = 0;
      for (int base = 0; base < P.maxChunks && open; base += 64) {
        const int ch = base + tid;
        const uint32_t n = ch < P.maxChunks ? cc[ch] : 0u;
        const uint32_t st = ch < P.maxChunks ? cs[ch] : 0u;  // (requested with the count: used only for the recorded chunks)
        const unsigned long long zero = __ballot(n == 0);
        const int live = zero ? __ffsll((long long)zero) - 1 : 64;  // chunks of this strip in front of the first empty one
        uint32_t x = tid < live ? n : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (tid >= o) x += y; }
        if (tid < live) { sCs[ch] = st; sPre[ch + 1] = carry + x; }
        carry += __shfl(x, 63, 64);
        nDense += (uint32_t)live;
        open = live == 64;
      }
      if (tid == 0) sNCh = nDense;
    }
    __syncthreads();
    const int nCh = (int)sNCh;
    const uint32_t nRec = sPre[nCh];
    auto chunkOf = [&](uint32_t r) {  // the chunk that holds record index r: the last one that starts at or before it
      int lo = 0, hi = nCh;
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sPre[mid] <= r) lo = mid; else hi = mid; }
      return lo;
    };
    VoteKey best; best.hi = ~0ull; best.lo = ~0ull;
    uint32_t nCand[2] = {0, 0};
    for (uint32_t r0 = tid; r0 < nRec; r0 += 2 * WG) {
      // two records per lane and round, both requested before either is looked at
      uint4 hdv[2], cwv[2];
      uint32_t rv[2];
      bool first[2];
      int chv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        rv[u] = r0 + u * WG;
        hdv[u] = make_uint4(0u, 0u, 0u, 0u); cwv[u] = hdv[u]; first[u] = false; chv[u] = 0;
        if (rv[u] < nRec) {
          chv[u] = chunkOf(rv[u]);
          first[u] = rv[u] == sPre[chv[u]];
          const uint32_t *rec = P.recs + (uint64_t)(sCs[chv[u]] + (rv[u] - sPre[chv[u]])) * stride;
          hdv[u] = ((const uint4 *)rec)[0]; cwv[u] = ((const uint4 *)rec)[1];  // words 0..3: re|strand, allele, state, candidate word 0 (or side-arena base); 4..5: candidate words 1, 2
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (rv[u] >= nRec) continue;
        const uint4 hd = hdv[u], cw = cwv[u];
        const bool pend = recPending(hd.z);
        const uint32_t nc = pend ? 1u : ((hd.z & REC_DONE) ? (hd.z & 0x3FFFFFFFu) : 0u);   // (neither: a group the closed-form pass ended without a candidate, left as seeded)
        const uint32_t w2own = pend ? pendingMatchWord(P, re, hd.z, cw.y, cw.z, cw.w) : cw.y;
        const int plus = (int)(hd.x >> 31);
        if (first[u]) sChPlus[chv[u]] = (uint8_t)plus;  // a chunk holds one strand
        uint32_t kept = 0;
        for (uint32_t j = 0; j < nc; ++j) {
          uint32_t w0 = hd.w, w1 = cw.x, w2 = w2own;
          if (hd.z & 0x40000000u) { const uint32_t *g = P.genCand + ((uint64_t)hd.w + j) * 6; w0 = g[0]; w1 = g[1]; w2 = g[2]; }
          VoteKey vk = voteKey((int)(w1 >> 20), (int)(w0 & 0xFFF), (int)((w0 >> 12) & 0xFFF), hd.y, plus, (int)(w1 & 0xFFFFF), (int)(w2 & 0xFFFFF));
          if (vk < best) best = vk;
          const uint32_t kc = keepCandidate<MAXLEN>(P, sBaseCnt, plus, w0, w1, w2) ? 1u : 0u;
          nCand[plus] += kc; kept += kc;
        }
        if (kept && rv[u] < KEEP_BITS) atomicOr(&sKeepBits[rv[u] >> 5], 1u << (rv[u] & 31));
      }
    }
    sVoteHi[tid] = best.hi; sVoteLo[tid] = best.lo;
    __syncthreads();
    for (int o = WG / 2; o > 0; o >>= 1) {
      if (tid < o) {
        VoteKey a{sVoteHi[tid], sVoteLo[tid]}, b{sVoteHi[tid + o], sVoteLo[tid + o]};
        if (b < a) { sVoteHi[tid] = b.hi; sVoteLo[tid] = b.lo; }
      }
      __syncthreads();
    }
    const uint32_t winPlus = (uint32_t)(sVoteHi[0] & 1);
    __syncthreads();
    uint32_t totWin;
    t1k_block_scan_exclusive(nCand[winPlus], warpSums, &totWin);
    if (tid == 0) {
      unsigned long long b = totWin ? atomicAdd(&P.counters[T1K_CTR_CAND], (unsigned long long)totWin) : 0ull;
      if (b + totWin > P.candCap) { atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_CANDCAP); sBase = 0xFFFFFFFFu; P.candStart[re] = 0; P.candCount[re] = 0; }
      else { sBase = (uint32_t)b; P.candStart[re] = (uint32_t)b; P.candCount[re] = totWin; }
    }
    __syncthreads();
    if (sBase != 0xFFFFFFFFu && totWin) {
      // chunks are in the reference's order ('-' strand first, alleles ascending); copy the winning strand's candidates in order:
      // a second prefix, over the winning strand's chunks alone (the others are empty in it), gives the pass its own dense index
      if (tid < 64) {
        uint32_t carry = 0;
        if (tid == 0) sPreW[0] = 0;
        for (int base = 0; base < nCh; base += 64) {
          const int ch = base + tid;
          uint32_t x = (ch < nCh && sChPlus[ch] == (uint8_t)winPlus) ? sPre[ch + 1] - sPre[ch] : 0u;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (tid >= o) x += y; }
          if (ch < nCh) sPreW[ch + 1] = carry + x;
          carry += __shfl(x, 63, 64);
        }
      }
      __syncthreads();
      const uint32_t nWin = sPreW[nCh];
      uint32_t written = 0;
      for (uint32_t i0 = 0; i0 < nWin; i0 += WG) {
        const uint32_t q = i0 + tid;
        uint32_t ridx = 0, g = 0;
        if (q < nWin) {
          int lo = 0, hi = nCh;  // the last chunk that starts at or before q in the winning strand's index (an empty one never is the last)
          while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sPreW[mid] <= q) lo = mid; else hi = mid; }
          ridx = sPre[lo] + (q - sPreW[lo]);
          g = sCs[lo] + (q - sPreW[lo]);
        }
        const bool look = q < nWin && (ridx >= KEEP_BITS || ((sKeepBits[ridx >> 5] >> (ridx & 31)) & 1u));
        uint4 hd = make_uint4(0u, 0u, 0u, 0u), cw = make_uint4(0u, 0u, 0u, 0u);
        if (look) { const uint32_t *rec = P.recs + (uint64_t)g * stride; hd = ((const uint4 *)rec)[0]; cw = ((const uint4 *)rec)[1]; }
        const bool pend = look && recPending(hd.z);
        const uint32_t nc = look ? (pend ? 1u : ((hd.z & REC_DONE) ? (hd.z & 0x3FFFFFFFu) : 0u)) : 0;
        const uint32_t w2own = pend ? pendingMatchWord(P, re, hd.z, cw.y, cw.z, cw.w) : cw.y;
        uint32_t keepMask = 0, nk = 0;  // a group holds at most 32 candidates
        for (uint32_t j = 0; j < nc; ++j) {
          uint32_t w0 = hd.w, w1 = cw.x, w2 = w2own;
          if (hd.z & 0x40000000u) { const uint32_t *gc = P.genCand + ((uint64_t)hd.w + j) * 6; w0 = gc[0]; w1 = gc[1]; w2 = gc[2]; }
          if (keepCandidate<MAXLEN>(P, sBaseCnt, (int)winPlus, w0, w1, w2)) { keepMask |= 1u << j; ++nk; }
        }
        uint32_t tot;
        uint32_t off = t1k_block_scan_exclusive(nk, warpSums, &tot);
        for (uint32_t j = 0; j < nc; ++j) {
          if (!((keepMask >> j) & 1u)) continue;
          uint32_t w0 = hd.w, w1 = cw.x, w2 = w2own;
          if (hd.z & 0x40000000u) { const uint32_t *gc = P.genCand + ((uint64_t)hd.w + j) * 6; w0 = gc[0]; w1 = gc[1]; w2 = gc[2]; }
          T1kCand cd;
          cd.allele = hd.y | (winPlus ? 0x80000000u : 0);
          cd.readSE = (w0 & 0xFFF) | (((w0 >> 12) & 0xFFF) << 16);
          cd.seqStart = (int)(w1 & 0xFFFFF); cd.seqEnd = (int)(w2 & 0xFFFFF);
          cd.match = (w1 >> 20) | ((w2 >> 20) << 16);
          cd.re = re;
          P.cand[(uint64_t)sBase + written + off] = cd;
          ++off;
        }
        written += tot;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
size_t t1k_chain_big_scratch_u32() { return (size_t)4 * BIG_CAP + GA_SCRATCH_INTS; }
int t1k_chain_max_chunks(uint32_t nAlleles) { return 2 * (int)((nAlleles + CHUNK_A - 1) / CHUNK_A) + 2; }
int t1k_chain_memo_entries() { return GAP_CACHE; }
int t1k_chain_rec_stride(int maxLen) { return maxLen <= 160 ? 8 : 16; }  // u32 per record (32 / 64 bytes)
int t1k_chain_max_kmers(int maxLen, int k) { return (2 * std::max(1, maxLen - k + 1) + 3) / 4 * 4; }
int t1k_chain_used_u32(int maxK) { return maxK * 4; }  // per used list: read offset, list start, list length, directory row

// striped list -> dense list; grid (blocks, T1K_NSTRIPE)
// The first workgroup also leaves the dense list's length in the arena's total word (T1K_TOTAL_BASE) for the consumers that take their item
// count from the device, and raises `overflowFlag` in the control word when a stripe is full (the range then runs again with larger lists).
template <class V>
__global__ __launch_bounds__(WG) void k_arena_compact(const V *src, uint32_t segCap, unsigned long long *counters, int arena, V *dst, unsigned long long overflowFlag) {
  const unsigned long long *cursors = counters + T1K_ARENA_BASE + (size_t)arena * T1K_NSTRIPE * T1K_STRIPE_WORDS;
  const uint32_t seg = blockIdx.y;
  uint32_t prefix = 0;
  for (uint32_t s = 0; s < seg; ++s) prefix += (uint32_t)min(cursors[s * T1K_STRIPE_WORDS], (unsigned long long)segCap);
  const uint32_t cnt = (uint32_t)min(cursors[seg * T1K_STRIPE_WORDS], (unsigned long long)segCap);
  if (blockIdx.x == 0 && seg == T1K_NSTRIPE - 1 && threadIdx.x == 0) {
    counters[T1K_TOTAL_BASE + arena] = (unsigned long long)prefix + cnt;
    bool over = false;
    for (uint32_t s = 0; s < T1K_NSTRIPE; ++s) over = over || cursors[s * T1K_STRIPE_WORDS] > (unsigned long long)segCap;
    if (over && overflowFlag) atomicOr(&counters[T1K_CTR_ERR], overflowFlag);
  }
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < cnt; i += gridDim.x * WG) dst[prefix + i] = src[(uint64_t)seg * segCap + i];
}

T1kArenaCounts t1k_arena_counts(const t1k_ctx *ctx, int arena, uint32_t segCap) {
  T1kArenaCounts r{0, 0, false};
  for (int s = 0; s < T1K_NSTRIPE; ++s) {
    unsigned long long c = t1k_cursor(ctx->hRaw, arena, s);
    if (c > segCap) { r.overflow = true; c = segCap; }
    r.total += c;
    r.maxSeg = std::max<uint32_t>(r.maxSeg, (uint32_t)c);
  }
  return r;
}

void t1k_arena_compact(t1k_ctx *ctx, int arena, const uint32_t *src, uint32_t segCap, uint32_t *dst, uint32_t maxSeg) {
  if (!maxSeg) return;
  hipLaunchKernelGGL(k_arena_compact<uint32_t>, dim3(std::min<uint32_t>((maxSeg + WG - 1) / WG, 256u), T1K_NSTRIPE), dim3(WG), 0, ctx->stream, src, segCap,
                     (unsigned long long *)ctx->bCounters.p, arena, dst, 0ull);
}
void t1k_arena_compact64(t1k_ctx *ctx, int arena, const unsigned long long *src, uint32_t segCap, unsigned long long *dst, uint32_t maxSeg) {
  if (!maxSeg) return;
  hipLaunchKernelGGL(k_arena_compact<unsigned long long>, dim3(std::min<uint32_t>((maxSeg + WG - 1) / WG, 256u), T1K_NSTRIPE), dim3(WG), 0, ctx->stream, src, segCap,
                     (unsigned long long *)ctx->bCounters.p, arena, dst, 0ull);
}
// the device-driven form: the grid is sized from an estimate of the fullest stripe (the kernel strides over what is there), the list's length goes to
// the arena's total word, a full stripe raises ERR_GROUPCAP on the device
void t1k_arena_compact_dev(t1k_ctx *ctx, int arena, const uint32_t *src, uint32_t segCap, uint32_t *dst, uint64_t estTotal) {
  const uint32_t perSeg = (uint32_t)std::min<uint64_t>(segCap, estTotal / T1K_NSTRIPE * 2 + WG);
  hipLaunchKernelGGL(k_arena_compact<uint32_t>, dim3(std::max(1u, std::min<uint32_t>((perSeg + WG - 1) / WG, 256u)), T1K_NSTRIPE), dim3(WG), 0, ctx->stream, src, segCap,
                     (unsigned long long *)ctx->bCounters.p, arena, dst, (unsigned long long)ERR_GROUPCAP);
}

// ------------------------------------------------------------------------------------------------------------------
// Counting sort of a dense work list by a small key (<= CS_BINS values), fused with the key's computation: the two in-loop orderings --
// registered alignments by read-window length (wavefronts of k_dp_dense sweep DPs of equal height: mixed lengths ran at 40 % lane
// utilisation), multi-diagonal groups by kind and hit count (k_chain_general) -- are 9- and 8-bit keys over ~10^6 items, for which a
// radix-sort library call (key kernel + three to four launches + its scan state) is out of proportion.  Two launches:
//   k_csort_count    LDS histogram per workgroup, its non-empty bins added to the global histogram
//   k_csort_scatter  every workgroup prefix-sums the global histogram itself (512 values), then tile by tile: LDS histogram with each
//                    item's rank inside the tile, one global atomic per non-empty bin reserves the tile's run inside the bin, items go
//                    out.  The order inside a bin is not defined (nothing downstream depends on it: the consumers' results are per
//                    item).  The last workgroup to finish clears the two global arrays for the next call (ticket counter).
// scratch: [hist CS_BINS | cursor CS_BINS | ticket] u32, zero when the first call starts (allocated zeroed, re-zeroed by every call).
// ------------------------------------------------------------------------------------------------------------------
#define CS_BINS 512
#define CS_TILE (WG * 8)
struct JobLenKey {  // read-window length of a registered alignment (memo entry bits 5..13)
  const unsigned long long *memo;
  __device__ __forceinline__ uint32_t operator()(uint32_t item) const { return (uint32_t)((memo[item] >> 5) & 0x1FF); }
};
struct GroupSizeKey {  // chains first (they skip the sorts: their own wavefronts), each kind by hit count (record word 4 after k_near_hits / k_gather_general)
  const uint32_t *recs; uint32_t stride; int useSimple;
  __device__ __forceinline__ uint32_t operator()(uint32_t item) const {
    const uint32_t *r = recs + (uint64_t)item * stride;
    const bool simple = useSimple && r[5] == REC_NEAR_DONE && r[6] == 1u;
    return simple ? min(r[4], 127u) : 128u + min(r[4], 63u);
  }
};
template <class KeyFn>
__global__ __launch_bounds__(WG) void k_csort_count(const uint32_t *list, uint32_t n, uint32_t *scratch, KeyFn key, const unsigned long long *nDev) {
  __shared__ uint32_t h[CS_BINS];
  if (nDev) n = (uint32_t)*nDev;
  for (int b = threadIdx.x; b < CS_BINS; b += WG) h[b] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) atomicAdd(&h[key(list[i])], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < CS_BINS; b += WG)
    if (h[b]) atomicAdd(&scratch[b], h[b]);
}
template <class KeyFn>
__global__ __launch_bounds__(WG) void k_csort_scatter(const uint32_t *list, uint32_t n, uint32_t *scratch, uint32_t *out, KeyFn key, const unsigned long long *nDev) {
  __shared__ uint32_t base[CS_BINS], h[CS_BINS], off[CS_BINS], warpSums[4];
  __shared__ uint32_t sLast;
  if (nDev) n = (uint32_t)*nDev;
  uint32_t *hist = scratch, *cursor = scratch + CS_BINS, *ticket = scratch + 2 * CS_BINS;
  {  // exclusive prefix of the global histogram (two bins per thread)
    const uint32_t a = hist[2 * threadIdx.x], b = hist[2 * threadIdx.x + 1];
    uint32_t tot;
    const uint32_t ex = t1k_block_scan_exclusive(a + b, warpSums, &tot);
    base[2 * threadIdx.x] = ex; base[2 * threadIdx.x + 1] = ex + a;
  }
  for (uint32_t t0 = blockIdx.x * CS_TILE; t0 < n; t0 += gridDim.x * CS_TILE) {
    for (int b = threadIdx.x; b < CS_BINS; b += WG) h[b] = 0;
    __syncthreads();
    uint32_t item[8], kk[8], rk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t i = t0 + j * WG + threadIdx.x;
      kk[j] = 0xFFFFFFFFu;
      if (i < n) { item[j] = list[i]; kk[j] = key(item[j]); rk[j] = atomicAdd(&h[kk[j]], 1u); }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < CS_BINS; b += WG)
      if (h[b]) off[b] = base[b] + atomicAdd(&cursor[b], h[b]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (kk[j] != 0xFFFFFFFFu) { const uint32_t pos = off[kk[j]] + rk[j]; if (pos < n) out[pos] = item[j]; }  // (pos < n always; the test keeps a scratch left dirty by a killed launch from writing outside the list)
    __syncthreads();
  }
  // the last workgroup out clears the arrays for the next call
  __threadfence();
  if (threadIdx.x == 0) sLast = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (sLast) {
    for (int b = threadIdx.x; b < 2 * CS_BINS; b += WG) scratch[b] = 0;
    if (threadIdx.x == 0) *ticket = 0;
  }
}
// list -> sorted (both n entries); returns `sorted`, or `list` when the scratch cannot be had
// nDev: the list's length is read on the device (n is then the most it can be: the sorted list's room; nEst sizes the grid)
template <class KeyFn>
static const uint32_t *countingSort(t1k_ctx *ctx, const uint32_t *list, uint32_t n, KeyFn key, const unsigned long long *nDev = nullptr, uint64_t nEst = 0) {
  static_assert(CS_BINS == 2 * WG, "two bins per thread in the prefix");
  const size_t head = (2 * CS_BINS + 16) * 4;
  const bool fresh = ctx->bJobSort.bytes < head + (size_t)n * 4;
  if (t1k_ensure(ctx, ctx->bJobSort, head + (size_t)n * 4) != T1K_OK) return list;
  uint32_t *scratch = (uint32_t *)ctx->bJobSort.p, *sorted = scratch + 2 * CS_BINS + 16;
  if (fresh && hipMemsetAsync(scratch, 0, head, ctx->stream) != hipSuccess) return list;  // (a new block: not zero yet; afterwards every call leaves it zero)
  const uint64_t forGrid = nDev ? std::min<uint64_t>(n, nEst) : n;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((forGrid + CS_TILE - 1) / CS_TILE, 1024u));
  hipLaunchKernelGGL(k_csort_count<KeyFn>, dim3(grid), dim3(WG), 0, ctx->stream, list, n, scratch, key, nDev);
  hipLaunchKernelGGL(k_csort_scatter<KeyFn>, dim3(grid), dim3(WG), 0, ctx->stream, list, n, scratch, sorted, key, nDev);
  return sorted;
}
// the same with the number of jobs read on the device (arena's total word); cap = the most there can be, est sizes the grids
void t1k_launch_dp_dense_dev(t1k_ctx *ctx, const ChainArgs &a, const uint32_t *jobs, int arena, uint32_t cap, uint64_t est) {
  const unsigned long long *nDev = (const unsigned long long *)ctx->bCounters.p + T1K_TOTAL_BASE + arena;
  jobs = countingSort(ctx, jobs, cap, JobLenKey{(const unsigned long long *)a.memo}, nDev, est);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, (std::min<uint64_t>(cap, est) + WG - 1) / WG);
  hipLaunchKernelGGL(k_dp_dense, dim3(grid), dim3(WG), 0, ctx->stream, a, jobs, cap, nDev);
}

// expected entries of an arena in a range of nRe read-ends (a quarter to spare), never more than it can hold
uint64_t t1k_arena_estimate(const t1k_ctx *ctx, int arena, uint64_t cap, uint32_t nRe) {
  if (!ctx->estValid || !ctx->estTotal[arena]) return cap;
  return std::min<uint64_t>(cap, (ctx->estTotal[arena] * std::max(1u, nRe) >> 16) * 5 / 4 + 4096);
}
void t1k_arena_estimate_set(t1k_ctx *ctx, int arena, uint64_t total, uint32_t nRe) { ctx->estTotal[arena] = (total << 16) / std::max(1u, nRe) + 1; }

// ------------------------------------------------------------------------------------------------------------------
// Route report (t1k_route_report_enable): one record per multi-diagonal group of the pass that has just ended, classified from the words the
// kernels left in its record -- word 4 = hits (0xFFFFFFFF: k_gather_general handed the group to k_chain_big by size), word 5 ==
// REC_NEAR_DONE and word 6 == 1 (k_near_hits; in an xlong range it did not run and the words still hold mask bits) -- and from the
// big list (a group on it that has a hit count came from a lane or a wavefront that met a gap beyond the register band).  Host only: it
// reads what is there after the range's counter fetch (the stream is idle), before the records' memory is used again.
// ------------------------------------------------------------------------------------------------------------------
static int routeCollect(t1k_ctx *ctx, const ChainArgs &a, bool longReads, bool xlong, uint64_t nGen, uint64_t nBig) {
  auto &rr = ctx->route;
  rr.passRecs.clear();
  rr.passLong = longReads; rr.passXlong = xlong;
  if (!nGen) return 0;
  std::vector<uint32_t> gen(nGen), big(nBig);
  T1K_HIP(ctx, hipMemcpy(gen.data(), a.generalList, nGen * 4, hipMemcpyDeviceToHost));
  if (nBig) T1K_HIP(ctx, hipMemcpy(big.data(), a.bigList, nBig * 4, hipMemcpyDeviceToHost));
  std::sort(big.begin(), big.end());
  // the listed records: the group arena is dense inside each stripe, so the sorted ids fall into a few runs; each run is one copy
  std::vector<uint32_t> ids(gen);
  std::sort(ids.begin(), ids.end());
  if (ids.back() >= a.groupCap) return t1k_fail(ctx, T1K_ERR_INTERNAL, "route report: a listed group lies outside the group arena");
  const uint32_t stride = a.recStride;
  std::vector<uint32_t> words((size_t)nGen * 8);  // words 0 .. 7 of each listed record, in the order of `ids`
  std::vector<uint32_t> buf;
  for (size_t s = 0; s < ids.size();) {
    size_t e = s + 1;
    while (e < ids.size() && ids[e] - ids[e - 1] <= 4096u && (uint64_t)(ids[e] - ids[s] + 1) * stride <= (64u << 20)) ++e;
    const uint64_t span = (uint64_t)(ids[e - 1] - ids[s] + 1) * stride;
    buf.resize(span);
    T1K_HIP(ctx, hipMemcpy(buf.data(), a.recs + (uint64_t)ids[s] * stride, span * 4, hipMemcpyDeviceToHost));
    for (size_t i = s; i < e; ++i) std::copy_n(&buf[(uint64_t)(ids[i] - ids[s]) * stride], 8, &words[i * 8]);
    s = e;
  }
  const uint64_t first = (uint64_t)(a.reads.len - ctx->reads.len);  // the range's first read-end in the uploaded set
  rr.passRecs.reserve(nGen);
  for (uint64_t q = 0; q < nGen; ++q) {
    const size_t at = std::lower_bound(ids.begin(), ids.end(), gen[q]) - ids.begin();
    const uint32_t *r = &words[at * 8];
    t1k_route_rec o{};
    o.read_end = (uint32_t)(first + (r[0] & 0x7FFFFFFFu)); o.allele = r[1]; o.n = r[4];
    o.strand = (r[0] >> 31) ? 0 : 1;
    o.near_done = !xlong && r[5] == REC_NEAR_DONE;
    o.simple = o.near_done && r[6] == 1u;
    o.nw = longReads ? 10 : 5; o.xlong = xlong ? 1 : 0;
    if (r[4] == 0xFFFFFFFFu) o.route = T1K_ROUTE_BIG_BY_SIZE;
    else if (std::binary_search(big.begin(), big.end(), gen[q])) o.route = T1K_ROUTE_BIG_BY_SCRATCH;
    else if (o.n <= GENERAL_SMALL || (o.simple && o.n <= 3 * GENERAL_SMALL)) o.route = T1K_ROUTE_GENERAL_LANE;
    else o.route = o.n <= 512u ? T1K_ROUTE_WAVE_SMALL : T1K_ROUTE_WAVE_LARGE;
    rr.passRecs.push_back(o);
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Seed report (t1k_seed_report_enable): what the seeding kernels decided for every read-end of the pass that has just ended, copied
// from the buffers ChainArgs names -- usedCount, usedOut (read offset and list length of each used k-mer; the first usedCount[2 re]
// entries are the read-end as given) and usedMask.  k_seed_groups writes a read-end's masks only where it seeds it (k <= len <=
// T1K_MAX_READ_LEN, not linked to an earlier window): the others' words are whatever the block held and are reported as zero.  Host
// only, like the route report: the stream is idle, the buffers are not used again before the next range.
// ------------------------------------------------------------------------------------------------------------------
static_assert(T1K_SEED_MASK_WORDS == T1K_USED_MASK_WORDS, "the seed report hands the kernels' used-offset masks out as they are");
static int seedCollect(t1k_ctx *ctx, const ChainArgs &a) {
  auto &p = ctx->seedRep.pass;
  const uint32_t n = a.reads.nReadEnds;
  constexpr uint32_t MW = 2 * T1K_USED_MASK_WORDS;
  p.first = (uint64_t)(a.reads.len - ctx->reads.len); p.count = n;  // the range's first read-end in the uploaded set
  p.counts.assign((size_t)n * 2, 0); p.masks.assign((size_t)n * MW, 0); p.usedPtr.assign((size_t)n + 1, 0); p.used.clear();
  std::vector<uint32_t> masks((size_t)n * MW);
  std::vector<uint16_t> len(n);
  std::vector<uint8_t> skip(a.reads.skip ? n : 0);
  T1K_HIP(ctx, hipMemcpy(p.counts.data(), a.usedCount, (size_t)n * 2 * 4, hipMemcpyDeviceToHost));
  T1K_HIP(ctx, hipMemcpy(masks.data(), a.usedMask, (size_t)n * MW * 4, hipMemcpyDeviceToHost));
  T1K_HIP(ctx, hipMemcpy(len.data(), a.reads.len, (size_t)n * 2, hipMemcpyDeviceToHost));
  if (a.reads.skip) T1K_HIP(ctx, hipMemcpy(skip.data(), a.reads.skip, n, hipMemcpyDeviceToHost));
  const size_t stride = (size_t)a.maxK * 4;  // words of a read-end's used-list table
  const uint32_t slab = (uint32_t)std::max<size_t>(1, (size_t)(16u << 20) / std::max<size_t>(stride, 1));  // read-ends per copy (64 MB)
  std::vector<uint32_t> buf;
  for (uint32_t r0 = 0; r0 < n; r0 += slab) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(n, (uint64_t)r0 + slab);
    buf.resize((size_t)(r1 - r0) * stride);
    T1K_HIP(ctx, hipMemcpy(buf.data(), a.usedOut + (size_t)r0 * stride, buf.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t re = r0; re < r1; ++re) {
      const uint32_t plus = p.counts[2 * (size_t)re], all = plus + p.counts[2 * (size_t)re + 1];
      if (all > a.maxK) return t1k_fail(ctx, T1K_ERR_INTERNAL, "seed report: a read-end has more used k-mers than its table holds");
      const uint32_t *uo = &buf[(size_t)(re - r0) * stride];
      for (uint32_t u = 0; u < all; ++u) {
        t1k_seed_used e{};
        e.read_off = uo[4 * u]; e.list_len = uo[4 * u + 2]; e.strand = u < plus ? 0 : 1;
        p.used.push_back(e);
      }
      p.usedPtr[(size_t)re + 1] = (uint32_t)p.used.size();
      const bool seeded = (int)len[re] >= a.k && (int)len[re] <= T1K_MAX_READ_LEN && !(a.reads.skip && skip[re]);
      if (seeded) std::copy_n(&masks[(size_t)re * MW], MW, &p.masks[(size_t)re * MW]);
    }
  }
  ctx->seedRep.passValid = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// The chain of one range as ONE submission (round 5).  Rounds 1-4 fetched the counter block six times per range -- after seeding, after
// the closed-form pass, after the gap walk, twice inside the multi-diagonal path, at the end -- because every consumer's grid and item
// count were launch arguments.  Here every consumer reads its item count on the device (the total word k_arena_compact leaves where it
// makes a striped list dense, or the group arena's cursors) and strides over the items, so its grid only has to be roughly right: it is
// sized from what the context's previous range counted (per read-end; the first range of a context: from the arenas' capacities).  A full
// stripe raises ERR_GROUPCAP on the device; the kernels behind it work on the clamped lists (their results are thrown away: the caller
// runs the range again with the capacities the cursors ask for, as before).  One counter fetch is left, at the end.
// ------------------------------------------------------------------------------------------------------------------
// runs K1..K6; on return hc[T1K_CTR_CAND] = number of candidates, hc[T1K_CTR_ERR] = error flags, hc[T1K_CTR_JOB_TOTAL ..] the lists' totals
int t1k_run_chain(t1k_ctx *ctx, const ChainArgs &aIn, int nWg, int bigBlocks, bool longReads, unsigned long long *hc) {
  ChainArgs a = aIn;
  a.devDriven = 1;
  const bool xlong = a.maxK > a.maxKFast;  // the window holds read-ends beyond T1K_MAX_READ_LEN: k_seed_long takes those
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
  if (const int rc = t1k_launch_seed(ctx, a, longReads, xlong)) return rc;
  T1K_HIP(ctx, hipEventRecord(ctx->ev[8], ctx->stream));
  const unsigned long long *tot = (const unsigned long long *)ctx->bCounters.p + T1K_TOTAL_BASE;
  const uint32_t nRe = std::max<uint32_t>(1u, a.reads.nReadEnds);
  auto est = [&](int arena, uint64_t cap) -> uint64_t { return t1k_arena_estimate(ctx, arena, cap, nRe); };
  auto blocks = [](uint64_t items, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (items + per - 1) / per); };
  const uint64_t listCap = (uint64_t)a.listSegCap * T1K_NSTRIPE, rareCap = (uint64_t)a.rareSegCap * T1K_NSTRIPE, jobCap = (uint64_t)a.jobSegCap * T1K_NSTRIPE,
                 genJobCap = (uint64_t)a.genJobSegCap * T1K_NSTRIPE;
  {  // closed-form pass over all records: blockIdx.y = stripe.  The straight-line kernel (the striding form costs it a wavefront per SIMD) over a
     // grid that covers what a stripe CAN hold: the workgroups beyond the stripe's cursor end at once (a few hundred thousand empty
     // workgroups are tens of microseconds of dispatch)
    const dim3 grid(blocks(a.groupSegCap, WG), T1K_NSTRIPE);
    if (longReads) hipLaunchKernelGGL((k_chain_fast<10, 0>), grid, dim3(WG), 0, ctx->stream, a, (const uint32_t *)nullptr, 0u, tot);
    else hipLaunchKernelGGL((k_chain_fast<5, 0>), grid, dim3(WG), 0, ctx->stream, a, (const uint32_t *)nullptr, 0u, tot);
  }
  {  // gap walk over the groups the closed form left
    const uint64_t e = est(T1K_AR_SLOW, listCap);
    t1k_arena_compact_dev(ctx, T1K_AR_SLOW, a.slowStr, a.listSegCap, a.slowList, e);
    if (longReads) hipLaunchKernelGGL((k_chain_fast<10, 1>), dim3(blocks(e, WG)), dim3(WG), 0, ctx->stream, a, (const uint32_t *)a.slowList, 0u, tot + T1K_AR_SLOW);
    else hipLaunchKernelGGL((k_chain_fast<5, 1>), dim3(blocks(e, WG)), dim3(WG), 0, ctx->stream, a, (const uint32_t *)a.slowList, 0u, tot + T1K_AR_SLOW);
  }
  const uint64_t eJobs = est(T1K_AR_JOBS, jobCap), eRetry = est(T1K_AR_RETRY, listCap), eGen = est(T1K_AR_GENERAL, rareCap);
  t1k_arena_compact_dev(ctx, T1K_AR_JOBS, a.jobStr, a.jobSegCap, a.jobList, eJobs);
  t1k_arena_compact_dev(ctx, T1K_AR_RETRY, a.retryStr, a.listSegCap, a.retryList, eRetry);
  t1k_arena_compact_dev(ctx, T1K_AR_GENERAL, a.generalStr, a.rareSegCap, a.generalList, eGen);
  // (the finish list -- groups whose candidate waits for registered alignments -- is only a count here: k_collect adds the match counts itself;
  // a full stripe of it loses nothing, its entries are never read)
  t1k_launch_dp_dense_dev(ctx, a, a.jobList, T1K_AR_JOBS, (uint32_t)jobCap, eJobs);
  if (longReads) hipLaunchKernelGGL((k_chain_fast<10, 2>), dim3(blocks(eRetry, WG)), dim3(WG), 0, ctx->stream, a, (const uint32_t *)a.retryList, 0u, tot + T1K_AR_RETRY);
  else hipLaunchKernelGGL((k_chain_fast<5, 2>), dim3(blocks(eRetry, WG)), dim3(WG), 0, ctx->stream, a, (const uint32_t *)a.retryList, 0u, tot + T1K_AR_RETRY);
  {  // groups with hits on several diagonals
    const int skipDone = !xlong;  // k_near_hits writes the hit lists it can (its masks span T1K_MAX_READ_LEN), k_gather_general the rest
    const unsigned long long *nGen = tot + T1K_AR_GENERAL;
    if (skipDone) {
      if (longReads) hipLaunchKernelGGL(k_near_hits<10>, dim3(blocks(eGen, WG)), dim3(WG), 0, ctx->stream, a, 0u, nGen);
      else hipLaunchKernelGGL(k_near_hits<5>, dim3(blocks(eGen, WG)), dim3(WG), 0, ctx->stream, a, 0u, nGen);
    }
    const uint32_t gatherGrid = std::min<uint32_t>(blocks(eGen, 4), 8192u);
    if (xlong) hipLaunchKernelGGL(k_gather_general<(T1K_LONG_READ_LEN + 63) / 64>, dim3(gatherGrid), dim3(WG), 0, ctx->stream, a, 0u, skipDone, nGen);
    else hipLaunchKernelGGL(k_gather_general<GROUP_FAST_MAXLEN / 64>, dim3(gatherGrid), dim3(WG), 0, ctx->stream, a, 0u, skipDone, nGen);
    ChainArgs g = a;
    g.generalList = (uint32_t *)countingSort(ctx, a.generalList, (uint32_t)rareCap, GroupSizeKey{(const uint32_t *)a.recs, a.recStride, skipDone}, nGen, eGen);  // groups of similar size side by side
    hipLaunchKernelGGL(k_chain_general, dim3(blocks(eGen, 64)), dim3(64), 0, ctx->stream, g, 0u, skipDone, nGen);
    const uint64_t eWave = est(T1K_AR_WAVE, rareCap);
    t1k_arena_compact_dev(ctx, T1K_AR_WAVE, a.waveStr, a.rareSegCap, a.waveList, eWave);
    T1K_HIP(ctx, hipFuncSetAttribute((const void *)k_chain_wave, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * WAVE_CAP * 4));
    {
      const uint32_t wgrid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(eWave, 2048u));
      const uint32_t smallCap = 512;  // the list is run twice: the small LDS size class first, the groups beyond it with the full arrays
      hipLaunchKernelGGL(k_chain_wave, dim3(wgrid), dim3(64), 3 * smallCap * 4, ctx->stream, a, 0u, tot + T1K_AR_WAVE, smallCap, 0u);
      hipLaunchKernelGGL(k_chain_wave, dim3(wgrid), dim3(64), 3 * WAVE_CAP * 4, ctx->stream, a, 0u, tot + T1K_AR_WAVE, (uint32_t)WAVE_CAP, smallCap);
    }
    const uint64_t eGenJobs = est(T1K_AR_GENJOBS, genJobCap);
    t1k_arena_compact_dev(ctx, T1K_AR_GENJOBS, a.genJobStr, a.genJobSegCap, a.genJobList, eGenJobs);
    t1k_launch_dp_dense_dev(ctx, a, a.genJobList, T1K_AR_GENJOBS, (uint32_t)genJobCap, eGenJobs);
    hipLaunchKernelGGL(k_general_finish, dim3(blocks(eGen, WG)), dim3(WG), 0, ctx->stream, a, 0u, nGen);
    t1k_arena_compact_dev(ctx, T1K_AR_BIG, a.bigStr, a.rareSegCap, a.bigList, est(T1K_AR_BIG, rareCap));
    hipLaunchKernelGGL(k_chain_big, dim3(bigBlocks * 64), dim3(64), 0, ctx->stream, a, 0u, tot + T1K_AR_BIG);
  }
  if (xlong) hipLaunchKernelGGL(k_collect<T1K_LONG_READ_LEN>, dim3(nWg), dim3(WG), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_collect<T1K_MAX_READ_LEN>, dim3(nWg), dim3(WG), 0, ctx->stream, a);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
  if (const int rc = t1k_fetch_counters(ctx, hc)) return rc;
  // what the cursors say: overflow of a list whose compaction is the only place that could have seen it, the statistics, the next range's estimates
  const T1kArenaCounts groups = t1k_arena_counts(ctx, T1K_AR_GROUPS, a.groupSegCap), slow = t1k_arena_counts(ctx, T1K_AR_SLOW, a.listSegCap), jobs = t1k_arena_counts(ctx, T1K_AR_JOBS, a.jobSegCap),
                       retry = t1k_arena_counts(ctx, T1K_AR_RETRY, a.listSegCap), fin = t1k_arena_counts(ctx, T1K_AR_FINISH, a.listSegCap), gen = t1k_arena_counts(ctx, T1K_AR_GENERAL, a.rareSegCap),
                       wv = t1k_arena_counts(ctx, T1K_AR_WAVE, a.rareSegCap), gj = t1k_arena_counts(ctx, T1K_AR_GENJOBS, a.genJobSegCap), big = t1k_arena_counts(ctx, T1K_AR_BIG, a.rareSegCap);
  if (groups.overflow || slow.overflow || jobs.overflow || retry.overflow || gen.overflow || wv.overflow || gj.overflow || big.overflow) hc[T1K_CTR_ERR] |= ERR_GROUPCAP;
  // (the finish list: T1K_CTR_FINISH_TOTAL is a statistic; the list itself is not read -- see above -- so its overflow is not an error)
  // A full job list means memo claims were released while other lanes already waited on them: what ran behind it may have met a slot still
  // pending (ERR_MEMO).  That is a consequence of the overflow, not an internal error: the range runs again with lists that fit.
  if (hc[T1K_CTR_ERR] & ERR_GROUPCAP) hc[T1K_CTR_ERR] &= ~(unsigned long long)ERR_MEMO;
  ctx->lastSlowGroups = slow.total;
  hc[T1K_CTR_JOB_TOTAL] = jobs.total; hc[T1K_CTR_RETRY_TOTAL] = retry.total; hc[T1K_CTR_GENERAL_TOTAL] = gen.total; hc[T1K_CTR_BIG_TOTAL] = big.total; hc[T1K_CTR_FINISH_TOTAL] = fin.total;
  if (!hc[T1K_CTR_ERR]) {
    const T1kArenaCounts *cs[] = {&groups, &slow, &jobs, &retry, &gen, &wv, &gj, &big};
    const int ar[] = {T1K_AR_GROUPS, T1K_AR_SLOW, T1K_AR_JOBS, T1K_AR_RETRY, T1K_AR_GENERAL, T1K_AR_WAVE, T1K_AR_GENJOBS, T1K_AR_BIG};
    for (int i = 0; i < 8; ++i) t1k_arena_estimate_set(ctx, ar[i], cs[i]->total, nRe);
    ctx->estValid = true;
  }
  if (ctx->seedRep.on) {  // (opt-in, and whether or not the range has a multi-diagonal group)
    ctx->seedRep.passValid = false;
    if (!hc[T1K_CTR_ERR])
      if (const int rc = seedCollect(ctx, a)) return rc;
  }
  if (ctx->route.on) {  // (opt-in: nothing above depends on it)
    ctx->route.passRecs.clear();
    if (!hc[T1K_CTR_ERR])
      if (const int rc = routeCollect(ctx, a, longReads, xlong, gen.total, big.total)) return rc;
  }
  return 0;
}
