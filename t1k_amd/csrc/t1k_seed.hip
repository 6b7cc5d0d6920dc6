// t1k_amd/csrc/t1k_seed.hip -- seeding of SeqSet::AssignRead on gfx950: the read-ends' k-mers -> one group record per (read-end, strand,
// allele) with at least three hits (all integer, HBM/LDS-bound).  The records are read by the chain kernels (t1k_chain.hip); what both sides
// agree on is in t1k_chain_rec.h.
//
//   k_seed_groups   one 256-thread workgroup per read-end: rolling 11-mers + direct-address look-up with the >=100 skip
//                   rule (GetHitsFromRead, SeqSet.hpp:1071-1229); per (strand, 1024-allele chunk) the hits are folded into
//                   per-allele LDS accumulators (reference diagonal, bitmask of hit offsets, stray counts), i.e. grouped by
//                   (strand, allele) as SortHits 1558-1590 does, and one record per group leaves the chip; groups with fewer
//                   than 3 hits are never written (refMinHitRequired, 1253/1314)
//   k_seed_long     the same for the rare read-ends beyond the hit masks' span: counts only, every group marked "several diagonals"
#include <algorithm>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_chain_rec.h"

// ------------------------------------------------------------------------------------------------------------------
// K1: seeds -> one record per (strand, allele) group, built in LDS in a single pass over the posting lists
//
// Alleles are processed in chunks of CHUNK_A; each allele of the chunk owns an accumulator in LDS:
//   diag  reference diagonal = diagonal of the first hit that arrived (any choice is valid, see groupFastPath)
//   M     bitmask of the read offsets whose k-mer hits the allele on that diagonal
//   meta  number of hits on other diagonals (low 16 bits) and how many of those lie within `radius` (high 16 bits)
// Posting lists are sorted by allele, so the chunk's slice of every used list is found by binary search from a cursor.
// A group record leaves the chip once, coalesced; no hit list is ever written.
// ------------------------------------------------------------------------------------------------------------------
#ifndef T1K_SEED_WAVES
#define T1K_SEED_WAVES 7   // round 6: the kernel's 20.7 KB of LDS admit SEVEN workgroups a compute unit; held to 64 VGPRs for eight it spilled 41 registers for an occupancy it never had (72 VGPRs: 24 spilled; 3.11 -> 2.87 ms per range alone, profiles/r06_callE_seed_waves_suite.log)
#endif
// (the body stays a helper that is inlined into the kernel: written into the kernel itself the same text allocates differently -- 22 / 24
// spilled VGPRs instead of 24 / 27 -- and the form that was measured is the one that ships)
template <int NW>
__device__ __forceinline__ void seedGroupsBody(const ChainArgs &P) {
  constexpr int AW = NW == 5 ? 7 : 13;  // u32 per accumulator: diag, meta, M[NW]; odd stride = no LDS bank conflicts
  extern __shared__ uint32_t lds[];
  const int k = P.k;
  const int maxK = (int)P.maxKFast;                 // >= k-mers of a read-end this kernel seeds, both strands (LDS layout; the used-list table's stride is P.maxK)
  uint32_t *acc = lds;                              // [CHUNK_A][AW] per-allele accumulators of the current chunk
  // look-up phase only (overlaid on the accumulators, which are re-initialised afterwards):
  uint32_t *ukCode = acc;                           // [maxK]  code | valid << 31
  uint32_t *ukStart = ukCode + maxK;                // [maxK]
  uint32_t *ukLen = ukStart + maxK;                 // [maxK]
  uint32_t *ukDir = ukLen + maxK;                   // [maxK]  chunk-directory row of the list
  uint16_t *usedQ = (uint16_t *)(ukDir + maxK);     // [maxK]  k-mers whose lists are used, + strand first
  // chunk loop:
  uint32_t *sLo = acc + CHUNK_A * AW;               // [maxK]  slice of the current chunk
  uint32_t *pre = sLo + maxK;                       // [maxK + 1] exclusive prefix of the slice lengths
  uint32_t *lstStart = pre + maxK + 1;              // [maxK]  posting-list start / length of the used lists (both strands)
  uint32_t *lstLen = lstStart + maxK;               // [maxK]
  uint32_t *lstDir = lstLen + maxK;                 // [maxK]
  uint16_t *qOf = (uint16_t *)(lstDir + maxK);      // [maxK]  read offset of the used lists
  // two bitmaps over all alleles (chunk selection, before the chunk loop of each strand): over the accumulators when they fit there
  // (references of up to 57 344 / 106 496 sequences), else behind the list arrays (the launcher sizes the dynamic LDS for it)
  const uint32_t A = P.ref.nAlleles;
  const uint32_t nChunks = P.ref.kDirStride - 1;    // (the launcher refuses more than 256 chunks: sHot)
  uint32_t *bitmaps = 2 * ((A + 31) >> 5) <= (uint32_t)(CHUNK_A * AW) ? acc : (uint32_t *)(qOf + ((maxK + 1) & ~1));
  __shared__ uint32_t warpSums[4];
  __shared__ uint32_t sHot[8];                      // bit c: chunk c can hold an allele with three hits (this strand)
  __shared__ uint32_t sUsed[2], sGroupBase, sFallback, sPost;
  __shared__ int sWaveMax[4];
  const int tid = threadIdx.x;
  const uint32_t kmask = (1u << (2 * k)) - 1;
  const uint32_t stride = P.recStride;
  for (uint32_t i = tid; i < CHUNK_A * AW; i += WG) acc[i] = (i % AW) == 0 ? (uint32_t)DIAG_EMPTY : 0u;
  __syncthreads();
#ifdef T1K_SEED_PROFILE
  uint64_t tp_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl_ = __builtin_amdgcn_s_memtime();
#endif
  __shared__ uint32_t sUMask[2 * T1K_USED_MASK_WORDS];  // read offsets whose lists are used, per strand
  __shared__ unsigned long long sStat[3];             // lookups, postings, hits: thread 0 tallies them in LDS (three 64-bit counters in registers would be held by every lane), flushed once per workgroup
  if (tid == 0) { sStat[0] = 0; sStat[1] = 0; sStat[2] = 0; }
  for (uint32_t re = blockIdx.x; re < P.reads.nReadEnds; re += gridDim.x) {
    const int len = P.reads.len[re];
    const int S = P.reads.S;
    const uint64_t *rbase = P.reads.bases + (uint64_t)re * 2 * S;
    const uint64_t *rnm = P.reads.nmask + (uint64_t)re * 2 * S;
    for (int c = tid; c < P.maxChunks; c += WG) P.chunkCount[(uint64_t)re * P.maxChunks + c] = 0;
    if (tid == 0) { P.usedCount[2 * re] = 0; P.usedCount[2 * re + 1] = 0; }
    // (a read-end beyond the hit masks' span is seeded by k_seed_long, launched behind this kernel)
    // (... and one whose lists an earlier window of the job holds is not seeded at all: t1k_xwin_link)
    if (len < k || len > T1K_MAX_READ_LEN || (P.reads.skip && P.reads.skip[re])) { __syncthreads(); continue; }  // GetOverlapsFromRead returns -1 (SeqSet.hpp:1598-1599)
    const int nk = len - k + 1;
    if (tid < 2 * T1K_USED_MASK_WORDS) sUMask[tid] = 0;  // (read by the previous read-end before its chunk loop's barriers)
    for (int q = tid; q < 2 * nk; q += WG) {
      int pass = q / nk, p = q - pass * nk;
      const uint64_t *b = rbase + pass * S, *nm = rnm + pass * S;
      uint32_t code = (uint32_t)t1k_get32(b, p) & kmask;
      bool valid = ((uint32_t)t1k_get32(nm, p) & kmask) == 0;
      uint32_t st = 0, ln = 0, dr = T1K_NO_DIR;
      if (valid) { st = P.ref.kStart[code]; ln = P.ref.kStart[code + 1] - st; dr = P.ref.kDirIdx[code]; }
      ukCode[q] = code | (valid ? 0x80000000u : 0);
      ukStart[q] = st; ukLen[q] = ln; ukDir[q] = dr;
    }
    __syncthreads();

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[0] += tn_ - tl_; tl_ = tn_; }
#endif
    // The look-up rule (SeqSet.hpp:1098-1153, 1165-1226) is a sequential state machine (prevKmerCode, skipCnt).
    // Parallel form: if no two k-mers within k/2 + 1 consecutive positions of a strand are equal, `code != prev` holds at every
    // position (prev is the code of one of the previous k/2 + 1 positions), every position is a look-up, and only skipCnt is
    // left: in a maximal run of "big" positions (list >= 100, not the first / last k-mer) exactly every (k/2 + 1)-th one is
    // used, any other position resets the count.  Reads with such short repeats take the sequential replay below.
    const int W1 = k / 2 + 1;
    if (tid == 0) { sFallback = 0; sUsed[0] = 0; sUsed[1] = 0; sPost = 0; }
    __syncthreads();
    int qv[3], lastNonBig[3];
    uint32_t szv[3];
    bool bigv[3];
    {
      int localMax = -1;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const int q = 3 * tid + x;
        qv[x] = q; szv[x] = 0; bigv[x] = false; lastNonBig[x] = -1;
        if (q < 2 * nk) {
          const int pass = q >= nk ? 1 : 0, p = q - pass * nk;
          const uint32_t code = ukCode[q] & 0x7FFFFFFFu;
          for (int d = 1; d <= W1 && d <= p; ++d)
            if ((ukCode[q - d] & 0x7FFFFFFFu) == code) sFallback = 1;
          szv[x] = ukLen[q];
          bigv[x] = szv[x] >= 100 && p != 0 && p != nk - 1;
          if (!bigv[x]) localMax = q;
        }
        lastNonBig[x] = localMax;  // within this lane so far; the lanes before are merged in below
      }
      // inclusive max-scan of localMax over the lanes (three consecutive positions per lane, lanes in position order)
      int incl = localMax;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl = max(incl, y); }
      if ((tid & 63) == 63) sWaveMax[tid >> 6] = incl;
      __syncthreads();
      int before = __shfl_up(incl, 1, 64);
      if ((tid & 63) == 0) before = -1;
      for (int w = 0; w < (tid >> 6); ++w) before = max(before, sWaveMax[w]);
#pragma unroll
      for (int x = 0; x < 3; ++x) lastNonBig[x] = max(lastNonBig[x], before);
    }
    const bool fallback = sFallback != 0;  // (sWaveMax's barrier also published sFallback)
    if (!fallback) {
      uint32_t mine = 0, minePlus = 0, minePost = 0;
      bool usedv[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        usedv[x] = false;
        if (qv[x] < 2 * nk && szv[x]) usedv[x] = !bigv[x] || ((qv[x] - lastNonBig[x]) % W1 == 0);
        if (usedv[x]) { ++mine; minePost += szv[x]; if (qv[x] < nk) ++minePlus; }
      }
      uint32_t tot;
      uint32_t slot = t1k_block_scan_exclusive(mine, warpSums, &tot);
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (usedv[x]) usedQ[slot++] = (uint16_t)qv[x];
      for (int o = 32; o > 0; o >>= 1) { minePlus += __shfl_xor(minePlus, o, 64); minePost += __shfl_xor(minePost, o, 64); }
      if ((tid & 63) == 0) { atomicAdd(&sUsed[0], minePlus); atomicAdd(&sPost, minePost); }
      __syncthreads();
      if (tid == 0) {
        sUsed[1] = tot - sUsed[0];
        sStat[0] += 2 * nk; sStat[1] += sPost;
        P.usedCount[2 * re] = sUsed[0]; P.usedCount[2 * re + 1] = sUsed[1];
      }
    }
    // sequential replay (reads with short repeats): the first wavefront runs it as uniform (scalar) code: each lane holds one
    // k-mer's code and list length, the loop reads them with v_readlane.
    if (fallback && tid < 64) {
      uint32_t prev = 0;  // prevKmerCode starts at code 0 and is carried from the + strand into the - strand
      uint32_t nUsed = 0;
      uint32_t lookups = 0, postings = 0;
      for (int pass = 0; pass < 2; ++pass) {
        int skipCnt = 0;
        const uint32_t begin = nUsed;
        for (int seg = 0; seg < nk; seg += 64) {
          const int pl = seg + tid;
          const uint32_t vc = pl < nk ? (ukCode[pass * nk + pl] & 0x7FFFFFFFu) : 0u;
          const uint32_t vl = pl < nk ? ukLen[pass * nk + pl] : 0u;
          const int cnt = min(64, nk - seg);
          for (int j = 0; j < cnt; ++j) {
            const uint32_t code = (uint32_t)__builtin_amdgcn_readlane((int)vc, j);
            const uint32_t size = (uint32_t)__builtin_amdgcn_readlane((int)vl, j);
            const int p = seg + j;
            if (p == 0 || code != prev) {
              ++lookups;
              if (size >= 100 && p != 0 && p != nk - 1 && skipCnt < k / 2) { ++skipCnt; continue; }
              skipCnt = 0;
              if (size) {
                if (tid == 0) usedQ[nUsed] = (uint16_t)(pass * nk + p);
                ++nUsed;
                postings += size;
              }
            }
            prev = code;
          }
        }
        if (tid == 0) sUsed[pass] = nUsed - begin;
      }
      if (tid == 0) {
        sStat[0] += lookups; sStat[1] += postings;
        P.usedCount[2 * re] = sUsed[0]; P.usedCount[2 * re + 1] = sUsed[1];
      }
    }
    __syncthreads();
    const uint32_t nUsedPlus = sUsed[0], nUsedMinus = sUsed[1];
#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[1] += tn_ - tl_; tl_ = tn_; }
#endif

    // the used lists are kept for k_chain_general, which re-derives the hits of the few multi-diagonal groups; which read offsets have
    // their lists used goes out per strand as bit masks as well (k_near_hits rebuilds the hits on near diagonals from them; sUMask was
    // cleared at the top of this read-end, before the barriers of the look-up phase)
    {
      uint32_t *uo = P.usedOut + (uint64_t)re * P.maxK * 4;
      for (uint32_t u = tid; u < nUsedPlus + nUsedMinus; u += WG) {
        int q = usedQ[u];
        int pass = u < nUsedPlus ? 0 : 1;
        uo[4 * u] = (uint32_t)(q - pass * nk); uo[4 * u + 1] = ukStart[q]; uo[4 * u + 2] = ukLen[q]; uo[4 * u + 3] = ukDir[q];
        atomicOr(&sUMask[pass * T1K_USED_MASK_WORDS + ((q - pass * nk) >> 5)], 1u << ((q - pass * nk) & 31));
      }
    }
    // what the chunk loop needs of the used lists moves out of the overlay, then the accumulators under it are made clean again
    __syncthreads();
    if (tid < 2 * T1K_USED_MASK_WORDS) P.usedMask[(uint64_t)re * 2 * T1K_USED_MASK_WORDS + tid] = sUMask[tid];
    for (uint32_t u = tid; u < nUsedPlus + nUsedMinus; u += WG) {
      const int q = usedQ[u];
      const int pass = u < nUsedPlus ? 0 : 1;
      const uint32_t st = ukStart[q], ln = ukLen[q];
      lstStart[u] = st; lstLen[u] = ln; lstDir[u] = ukDir[q]; qOf[u] = (uint16_t)(q - pass * nk);
    }
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)((9 * maxK + 1) / 2); i += WG) acc[i] = (i % AW) == 0 ? (uint32_t)DIAG_EMPTY : 0u;
    __syncthreads();

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[2] += tn_ - tl_; tl_ = tn_; }
#endif
    int chunk = 0;
    for (int sp = 0; sp < 2; ++sp) {  // '-' strand first (SortHits 1577-1583)
      const int pass = sp == 0 ? 1 : 0;
      const uint32_t uBegin = pass == 0 ? 0 : nUsedPlus;
      const uint32_t uCount = pass == 0 ? nUsedPlus : nUsedMinus;
      if (uCount == 0) continue;
      // thread t owns the lists t and t + WG (uCount <= 2 * WG: reads are at most 320 bp)
      const bool has0 = (uint32_t)tid < uCount, has1 = (uint32_t)tid + WG < uCount;
      uint32_t cur0 = 0, cur1 = 0;
      // ---- which chunks can hold a group at all.  A group needs >= 3 hits on its allele.  The k-mers of a read that are not part of
      // a gene's conserved sequence have short lists (a handful of chance postings anywhere in the reference), and there are enough of
      // them to put a posting or two into EVERY chunk: stepping through all chunks for them was most of this kernel's time.  So: a
      // chunk is visited if a long list (one with a directory row: its per-chunk occupancy mask is part of the index) has a posting
      // in it, or if some allele of it collects three postings from the short lists alone -- counted exactly with two bitmaps over
      // all alleles (seen once / seen twice; the third sighting marks the chunk).  Every other chunk holds no allele with three hits
      // and cannot emit a record.  mk0 / mk1: chunk occupancy of this lane's own lists (chunks < 64; beyond that: "maybe").
      unsigned long long mk0 = 0, mk1 = 0;
      {
        const uint32_t BW = (A + 31) >> 5;
        uint32_t *b1 = bitmaps, *b2 = bitmaps + BW;
        for (uint32_t i = tid; i < 2 * BW; i += WG) bitmaps[i] = 0;
        if (tid < 8) sHot[tid] = 0;
        __syncthreads();
        auto mark = [&](bool has, uint32_t st, uint32_t ln, uint32_t row, unsigned long long &mk) {
          if (!has || !ln) return;
          if (row != T1K_NO_DIR) {
            const unsigned long long *m = P.ref.kDirMask + (uint64_t)row * P.ref.kDirMaskWords;
            for (uint32_t w = 0; w < P.ref.kDirMaskWords; ++w) {
              const unsigned long long v = m[w];
              if (w == 0) mk = v;
              if ((uint32_t)v) atomicOr(&sHot[2 * w], (uint32_t)v);
              if ((uint32_t)(v >> 32)) atomicOr(&sHot[2 * w + 1], (uint32_t)(v >> 32));
            }
            if (P.ref.kDirMaskWords > 1) mk = ~0ull;  // (more than 64 chunks: the directory itself answers)
          } else {
            for (uint32_t j0 = 0; j0 < ln; j0 += 8) {  // <= T1K_DIR_MINLEN postings; eight loads in flight
              uint32_t al[8];
#pragma unroll
              for (int x = 0; x < 8; ++x) al[x] = j0 + x < ln ? P.ref.kPostAllele[st + j0 + x] : 0xFFFFFFFFu;
#pragma unroll
              for (int x = 0; x < 8; ++x) {
                if (al[x] == 0xFFFFFFFFu) continue;
                const uint32_t ci = al[x] / CHUNK_A, bit = 1u << (al[x] & 31);
                mk |= ci < 64 ? 1ull << ci : 0ull;
                if (atomicOr(&b1[al[x] >> 5], bit) & bit)
                  if (atomicOr(&b2[al[x] >> 5], bit) & bit) atomicOr(&sHot[ci >> 5], 1u << (ci & 31));
              }
            }
            if (nChunks > 64) mk = ~0ull;
          }
        };
        mark(has0, has0 ? lstStart[uBegin + tid] : 0u, has0 ? lstLen[uBegin + tid] : 0u, has0 ? lstDir[uBegin + tid] : T1K_NO_DIR, mk0);
        mark(has1, has1 ? lstStart[uBegin + tid + WG] : 0u, has1 ? lstLen[uBegin + tid + WG] : 0u, has1 ? lstDir[uBegin + tid + WG] : T1K_NO_DIR, mk1);
        __syncthreads();
        if (bitmaps == acc) {  // the bitmaps lay over the accumulators: make those clean again
          for (uint32_t i = tid; i < 2 * BW; i += WG) acc[i] = (i % AW) == 0 ? (uint32_t)DIAG_EMPTY : 0u;
          __syncthreads();
        }
      }
      // first posting with allele >= bound in [lo, ln) of a short list (bisection over the allele column)
      auto lowerBound = [&](uint32_t st, uint32_t lo, uint32_t ln, uint32_t bound) -> uint32_t {
        uint32_t hi = ln;
        while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (P.ref.kPostAllele[st + m] < bound) lo = m + 1; else hi = m; }
        return lo;
      };
      for (uint32_t hw = 0; hw < 8; ++hw) {
       uint32_t hotBits = sHot[hw];
       while (hotBits) {
        const uint32_t ci = hw * 32 + (uint32_t)__ffs((int)hotBits) - 1;
        hotBits &= hotBits - 1;
        const uint32_t c0 = ci * CHUNK_A;
        const uint32_t c1 = min(c0 + CHUNK_A, A);
#ifdef T1K_SEED_PROFILE
        tp_[3] += 1;  // chunks visited (not a clock)
#endif
        // slice of every used list inside [c0, c1): long lists from their directory row, short ones by bisection from their cursor
        // (the chunks come in ascending order, so the cursor only moves forward); lists without a posting here are not touched
        // (a lane's list start / length / directory row are read back from LDS where they are needed: held in registers across the
        // chunk loop they were spilled to scratch under the 64-VGPR budget)
        uint32_t n0 = 0, n1 = 0;
        const bool may = ci >= 64;
        if (has0) {
          uint32_t lo = cur0, hi = cur0;
          if (may || ((mk0 >> ci) & 1ull)) {
            const uint32_t row = lstDir[uBegin + tid];
            if (row != T1K_NO_DIR) { const uint32_t *dir = P.ref.kDir + (uint64_t)row * P.ref.kDirStride; lo = dir[ci]; hi = dir[ci + 1]; }
            else { const uint32_t st = lstStart[uBegin + tid], ln = lstLen[uBegin + tid]; lo = lowerBound(st, cur0, ln, c0); hi = lowerBound(st, lo, ln, c1); }
          }
          n0 = hi - lo; sLo[tid] = lo; cur0 = hi;
        }
        if (has1) {
          uint32_t lo = cur1, hi = cur1;
          if (may || ((mk1 >> ci) & 1ull)) {
            const uint32_t row = lstDir[uBegin + tid + WG];
            if (row != T1K_NO_DIR) { const uint32_t *dir = P.ref.kDir + (uint64_t)row * P.ref.kDirStride; lo = dir[ci]; hi = dir[ci + 1]; }
            else { const uint32_t st = lstStart[uBegin + tid + WG], ln = lstLen[uBegin + tid + WG]; lo = lowerBound(st, cur1, ln, c0); hi = lowerBound(st, lo, ln, c1); }
          }
          n1 = hi - lo; sLo[tid + WG] = lo; cur1 = hi;
        }

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[4] += tn_ - tl_; tl_ = tn_; }
#endif
        uint32_t tot0, tot1 = 0;
        const uint32_t e0 = t1k_block_scan_exclusive(n0, warpSums, &tot0);
        if (has0) pre[tid] = e0;
        if (uCount > WG) {
          const uint32_t e1 = t1k_block_scan_exclusive(n1, warpSums, &tot1);
          if (has1) pre[tid + WG] = tot0 + e1;
        }
        const uint32_t T = tot0 + tot1;
        if (tid == 0) { pre[uCount] = T; sStat[2] += T; }
        __syncthreads();

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[5] += tn_ - tl_; tl_ = tn_; }
#endif
        // walk the chunk's postings.  The flat posting index [0, T) is cut into one contiguous range per wavefront; a lane finds the
        // list of its first posting by bisection over the prefix ONCE, and from there its list index only moves forward (its
        // positions grow by 64 a step), so the later postings cost a look at one or two prefix entries instead of a bisection each.
        // Four postings in flight per lane; 64 consecutive postings per wavefront load.
        {
          const uint32_t wv = (uint32_t)tid >> 6, ln = (uint32_t)tid & 63u;
          const uint32_t Rw = (((T + 3) >> 2) + 63u) & ~63u;
          const uint32_t jBeg = wv * Rw, jEnd = min(T, jBeg + Rw);
          uint32_t lo = 0;
          if (jBeg + ln < jEnd) {
            const uint32_t j = jBeg + ln;
            uint32_t hi = uCount;
            while (hi - lo > 1) { uint32_t m = (lo + hi) >> 1; if (pre[m] <= j) lo = m; else hi = m; }
          }
#ifndef T1K_SEED_INFLIGHT
#define T1K_SEED_INFLIGHT 4
#endif
          for (uint32_t j0 = jBeg + ln; j0 < jEnd; j0 += T1K_SEED_INFLIGHT * 64) {
            T1kPosting pst[T1K_SEED_INFLIGHT];
            int rr[T1K_SEED_INFLIGHT];
#pragma unroll
            for (int x = 0; x < T1K_SEED_INFLIGHT; ++x) {
              const uint32_t j = j0 + x * 64;
              if (j < jEnd) {
                while (pre[lo + 1] <= j) ++lo;  // pre[uCount] = T > j ends it
                pst[x] = P.ref.kPost[lstStart[uBegin + lo] + sLo[lo] + (j - pre[lo])];
                rr[x] = (int)qOf[uBegin + lo];
              }
            }
#pragma unroll
            for (int x = 0; x < T1K_SEED_INFLIGHT; ++x) {
              const uint32_t j = j0 + x * 64;
              if (j < jEnd) {
                const int r = rr[x];
                const int d = r - (int)pst[x].offset;
                uint32_t *a = acc + (pst[x].allele - c0) * AW;
                const uint32_t old = atomicCAS(&a[0], (uint32_t)DIAG_EMPTY, (uint32_t)d);
                if (old == (uint32_t)DIAG_EMPTY || old == (uint32_t)d) atomicOr(&a[2 + (r >> 5)], 1u << (r & 31));
                else {
                  int dd = d - (int)old; if (dd < 0) dd = -dd;
                  atomicAdd(&a[1], dd <= P.radius ? 0x10001u : 1u);
                }
              }
            }
          }
        }
        __syncthreads();

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[6] += tn_ - tl_; tl_ = tn_; }
#endif
        // emit the groups that can still produce a candidate: >= 3 hits in total, and either >= 3 on the reference diagonal
        // or some hit close enough to chain with it, or > 2 strays (which could form their own run).  Lane t looks at the
        // accumulators t, t + WG, ... (conflict-free with the odd accumulator stride); the records leave in allele order.
        constexpr int EPT = CHUNK_A / WG;
        uint32_t flags = 0;
        uint64_t packed = 0;  // EPT counters of 16 bits
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          const uint32_t *a = acc + (i * WG + tid) * AW;
          if (a[0] == (uint32_t)DIAG_EMPTY) continue;
          int onDiag = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) onDiag += __popc(a[2 + w]);
          const uint32_t strays = a[1] & 0xFFFFu, nearCnt = a[1] >> 16;
          const bool general = nearCnt > 0 || strays > 2;
          flags |= 2u << (2 * i);  // occupied
          if (onDiag + (int)strays >= 3 && (general || onDiag >= 3)) { flags |= 1u << (2 * i); packed += 1ull << (16 * i); }
        }
        uint32_t totLo, totHi = 0, exHi = 0;
        const uint32_t exLo = t1k_block_scan_exclusive((uint32_t)packed, warpSums, &totLo);
        exHi = t1k_block_scan_exclusive((uint32_t)(packed >> 32), warpSums, &totHi);  // (skipping it when CHUNK_A <= 512 -- the high word is empty then -- measured 4 % SLOWER)
        const uint64_t ex = (uint64_t)exLo | ((uint64_t)exHi << 32), tt = (uint64_t)totLo | ((uint64_t)totHi << 32);
        const uint32_t gTot = (uint32_t)((tt & 0xFFFF) + ((tt >> 16) & 0xFFFF) + ((tt >> 32) & 0xFFFF) + (tt >> 48));
        if (tid == 0) {
          const uint32_t gb = gTot ? t1k_arena_alloc(P.counters, T1K_AR_GROUPS, gTot, P.groupSegCap) : 0u;
          const bool ok = gb != T1K_ARENA_FULL && chunk < P.maxChunks;
          if (!ok) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_GROUPCAP);
          sGroupBase = ok ? gb : 0xFFFFFFFFu;
          if (ok && gTot) { P.chunkStart[(uint64_t)re * P.maxChunks + chunk] = gb; P.chunkCount[(uint64_t)re * P.maxChunks + chunk] = gTot; }
        }
        __syncthreads();
        const uint32_t groupBase = sGroupBase;

#ifdef T1K_SEED_PROFILE
    { const uint64_t tn_ = __builtin_amdgcn_s_memtime(); tp_[7] += tn_ - tl_; tl_ = tn_; }
#endif
        if (gTot) ++chunk;
        uint32_t before = 0;  // records of the lower accumulator rows
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          if ((flags >> (2 * i)) & 2u) {
            uint32_t *a = acc + (i * WG + tid) * AW;
            if (((flags >> (2 * i)) & 1u) && groupBase != 0xFFFFFFFFu) {
              const uint32_t slot = before + (uint32_t)((ex >> (16 * i)) & 0xFFFF);
              uint4 *rec = (uint4 *)(P.recs + (uint64_t)(groupBase + slot) * stride);
              constexpr int RW = NW == 5 ? 8 : 16;  // record words: re|strand, allele, diagonal + stray counts, M[NW]
              uint32_t v[RW];
              v[0] = re | (pass == 0 ? 0x80000000u : 0);  // bit31: '+' strand
              v[1] = c0 + i * WG + tid;
              v[2] = packDiagMeta((int)a[0], a[1]);
#pragma unroll
              for (int w = 0; w < NW; ++w) v[3 + w] = a[2 + w];
#pragma unroll
              for (int w = 3 + NW; w < RW; ++w) v[w] = 0;
#pragma unroll
              for (int w = 0; w < RW / 4; ++w) rec[w] = make_uint4(v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]);
            }
            a[0] = (uint32_t)DIAG_EMPTY; a[1] = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) a[2 + w] = 0;
          }
          before += (uint32_t)((tt >> (16 * i)) & 0xFFFF);
        }
        __syncthreads();
       }
      }
    }
  }
#ifdef T1K_SEED_PROFILE
  if (tid == 0) for (int i = 0; i < T1K_WIN_SEED_PROFILE_LEN; ++i) atomicAdd(&P.counters[T1K_WIN_SEED_PROFILE + i], (unsigned long long)tp_[i]);
#endif
  if (tid == 0) {  // statistics: one striped atomic per workgroup and counter
    unsigned long long *st = P.counters + T1K_STAT_BASE + (blockIdx.x & (T1K_STAT_STRIPES - 1)) * T1K_STAT_KINDS;
    atomicAdd(&st[T1K_STAT_LOOKUPS], sStat[0]); atomicAdd(&st[T1K_STAT_POSTINGS], sStat[1]); atomicAdd(&st[T1K_STAT_HITS], sStat[2]);
  }
}
template <int NW>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(T1K_SEED_WAVES, T1K_SEED_WAVES))) void k_seed_groups(ChainArgs P) { seedGroupsBody<NW>(P); }

// ------------------------------------------------------------------------------------------------------------------
// K1L: seeding of the read-ends beyond the hit masks' span (T1K_MAX_READ_LEN < len <= T1K_LONG_READ_LEN), one workgroup per such
// read-end; the others are k_seed_groups' and are skipped here.  No masks, no diagonals: the look-up rule (GetHitsFromRead,
// SeqSet.hpp:1071-1229) is replayed sequentially by the first wavefront, the used lists are kept for gatherHits as usual, and a
// (strand, allele) pair that collects >= 3 postings (minHitRequired, 1253 / 1314) becomes a group record flagged "several diagonals":
// k_chain_fast<*, 0> hands such records to k_gather_general -> k_chain_general / k_chain_wave / k_chain_big, which rebuild the hit
// list and run the reference's diagonal-run / LIS logic on it whatever the read's length.  Counts live in LDS for LONG_CH alleles at
// a time; a pass emits its records in allele order as one entry of the read-end's chunk table ('-' strand first, as SortHits
// 1577-1583 orders the groups).  Slow by design: such reads are the odd ones among millions.
// ------------------------------------------------------------------------------------------------------------------
#define LONG_CH 16384
__global__ __launch_bounds__(WG) void k_seed_long(ChainArgs P) {
  extern __shared__ uint32_t lds[];
  const int k = P.k;
  const int maxK = (int)P.maxK;
  uint32_t *ukCode = lds;                           // [maxK]  code | valid << 31
  uint32_t *ukStart = ukCode + maxK;                // [maxK]
  uint32_t *ukLen = ukStart + maxK;                 // [maxK]
  uint32_t *ukDir = ukLen + maxK;                   // [maxK]
  uint16_t *usedQ = (uint16_t *)(ukDir + maxK);     // [maxK]  used k-mers, + strand first
  uint32_t *cnt = (uint32_t *)(usedQ + ((maxK + 1) & ~1));  // [LONG_CH] postings per allele of the current pass
  __shared__ uint32_t warpSums[4];
  __shared__ uint32_t sUsed[2], sGroupBase;
  const int tid = threadIdx.x;
  const uint32_t kmask = (1u << (2 * k)) - 1;
  const uint32_t stride = P.recStride;
  const uint32_t A = P.ref.nAlleles;
  unsigned int hitsLocal = 0;
  for (uint32_t re = blockIdx.x; re < P.reads.nReadEnds; re += gridDim.x) {
    const int len = P.reads.len[re];
    if (len <= T1K_MAX_READ_LEN || (P.reads.skip && P.reads.skip[re])) continue;  // (uniform over the workgroup)
    const int S = P.reads.S;
    const uint64_t *rbase = P.reads.bases + (uint64_t)re * 2 * S;
    const uint64_t *rnm = P.reads.nmask + (uint64_t)re * 2 * S;
    const int nk = len - k + 1;
    __syncthreads();  // the previous read-end's tables are dead
    for (int q = tid; q < 2 * nk; q += WG) {
      const int pass = q / nk, p = q - pass * nk;
      const uint64_t *b = rbase + pass * S, *nm = rnm + pass * S;
      const uint32_t code = (uint32_t)t1k_get32(b, p) & kmask;
      const bool valid = ((uint32_t)t1k_get32(nm, p) & kmask) == 0;
      uint32_t st = 0, ln = 0, dr = T1K_NO_DIR;
      if (valid) { st = P.ref.kStart[code]; ln = P.ref.kStart[code + 1] - st; dr = P.ref.kDirIdx[code]; }
      ukCode[q] = code | (valid ? 0x80000000u : 0);
      ukStart[q] = st; ukLen[q] = ln; ukDir[q] = dr;
    }
    __syncthreads();
    // the look-up rule, sequentially (SeqSet.hpp:1098-1153, 1165-1226): lane j of the first wavefront holds one k-mer's code
    // and list length, the loop reads them with v_readlane (the same replay k_seed_groups runs for reads with short repeats)
    if (tid < 64) {
      uint32_t prev = 0, nUsed = 0, lookups = 0, postings = 0;
      for (int pass = 0; pass < 2; ++pass) {
        int skipCnt = 0;
        const uint32_t begin = nUsed;
        for (int seg = 0; seg < nk; seg += 64) {
          const int pl = seg + tid;
          const uint32_t vc = pl < nk ? (ukCode[pass * nk + pl] & 0x7FFFFFFFu) : 0u;
          const uint32_t vl = pl < nk ? ukLen[pass * nk + pl] : 0u;
          const int cntj = min(64, nk - seg);
          for (int j = 0; j < cntj; ++j) {
            const uint32_t code = (uint32_t)__builtin_amdgcn_readlane((int)vc, j);
            const uint32_t size = (uint32_t)__builtin_amdgcn_readlane((int)vl, j);
            const int p = seg + j;
            if (p == 0 || code != prev) {
              ++lookups;
              if (size >= 100 && p != 0 && p != nk - 1 && skipCnt < k / 2) { ++skipCnt; continue; }
              skipCnt = 0;
              if (size) {
                if (tid == 0) usedQ[nUsed] = (uint16_t)(pass * nk + p);
                ++nUsed;
                postings += size;
              }
            }
            prev = code;
          }
        }
        if (tid == 0) sUsed[pass] = nUsed - begin;
      }
      if (tid == 0) {
        P.usedCount[2 * re] = sUsed[0]; P.usedCount[2 * re + 1] = sUsed[1];
        unsigned long long *st = P.counters + T1K_STAT_BASE + (blockIdx.x & (T1K_STAT_STRIPES - 1)) * T1K_STAT_KINDS;
        atomicAdd(&st[T1K_STAT_LOOKUPS], (unsigned long long)lookups); atomicAdd(&st[T1K_STAT_POSTINGS], (unsigned long long)postings);
      }
    }
    __syncthreads();
    const uint32_t nUsedPlus = sUsed[0], nUsedMinus = sUsed[1];
    {
      uint32_t *uo = P.usedOut + (uint64_t)re * maxK * 4;
      for (uint32_t u = tid; u < nUsedPlus + nUsedMinus; u += WG) {
        const int q = usedQ[u];
        const int pass = u < nUsedPlus ? 0 : 1;
        uo[4 * u] = (uint32_t)(q - pass * nk); uo[4 * u + 1] = ukStart[q]; uo[4 * u + 2] = ukLen[q]; uo[4 * u + 3] = ukDir[q];
      }
    }
    int chunk = 0;
    for (int sp = 0; sp < 2; ++sp) {  // '-' strand first
      const int pass = sp == 0 ? 1 : 0;
      const uint32_t uBegin = pass == 0 ? 0 : nUsedPlus;
      const uint32_t uCount = pass == 0 ? nUsedPlus : nUsedMinus;
      if (uCount == 0) continue;
      for (uint32_t c0 = 0; c0 < A; c0 += LONG_CH) {
        const uint32_t c1 = min(c0 + (uint32_t)LONG_CH, A);
        for (uint32_t i = tid; i < LONG_CH; i += WG) cnt[i] = 0;
        __syncthreads();
        for (uint32_t u = tid; u < uCount; u += WG) {
          const int q = usedQ[uBegin + u];
          const uint32_t st = ukStart[q], ln = ukLen[q];
          uint32_t lo = 0, hi = ln;  // first posting with allele >= c0
          while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (P.ref.kPostAllele[st + m] < c0) lo = m + 1; else hi = m; }
          for (uint32_t j = lo; j < ln; ++j) {
            const uint32_t al = P.ref.kPostAllele[st + j];
            if (al >= c1) break;
            atomicAdd(&cnt[al - c0], 1u);
            ++hitsLocal;
          }
        }
        __syncthreads();
        constexpr uint32_t PER = LONG_CH / WG;  // thread t looks at the alleles [c0 + t * PER, + PER): the records leave in allele order
        uint32_t mine = 0;
        for (uint32_t i = 0; i < PER; ++i) mine += cnt[tid * PER + i] >= 3u ? 1u : 0u;
        uint32_t gTot;
        const uint32_t ex = t1k_block_scan_exclusive(mine, warpSums, &gTot);
        if (tid == 0) {
          const uint32_t gb = gTot ? t1k_arena_alloc(P.counters, T1K_AR_GROUPS, gTot, P.groupSegCap) : 0u;
          const bool ok = gb != T1K_ARENA_FULL && chunk < P.maxChunks;
          if (!ok) atomicOr(&P.counters[T1K_CTR_ERR], (unsigned long long)ERR_GROUPCAP);
          sGroupBase = ok ? gb : 0xFFFFFFFFu;
          if (ok && gTot) { P.chunkStart[(uint64_t)re * P.maxChunks + chunk] = gb; P.chunkCount[(uint64_t)re * P.maxChunks + chunk] = gTot; }
        }
        __syncthreads();
        const uint32_t groupBase = sGroupBase;
        if (gTot) ++chunk;
        if (mine && groupBase != 0xFFFFFFFFu) {
          uint32_t slot = ex;
          for (uint32_t i = 0; i < PER; ++i) {
            if (cnt[tid * PER + i] < 3u) continue;
            uint4 *rec = (uint4 *)(P.recs + (uint64_t)(groupBase + slot) * stride);
            // words 0..2: read-end | '+' strand, allele, "several diagonals" (recIsGeneral: near count 1, diagonal 0); the rest is the chain's
            rec[0] = make_uint4(re | (pass == 0 ? 0x80000000u : 0u), c0 + tid * PER + i, (uint32_t)REC_DIAG_BIAS | (31u << 25), 0u);  // near = 31: "count unknown", the hits come from the used lists
            for (uint32_t w = 1; w < stride / 4; ++w) rec[w] = make_uint4(0u, 0u, 0u, 0u);
            ++slot;
          }
        }
        __syncthreads();
      }
    }
  }
  t1k_stat_add(P.counters, T1K_STAT_HITS, hitsLocal);
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
// K1 (+ K1L when the window holds read-ends beyond T1K_MAX_READ_LEN) over the range; longReads: masks of 10 words (reads <= 320 bp) instead of 5
int t1k_launch_seed(t1k_ctx *ctx, const ChainArgs &a, bool longReads, bool xlong) {
  const int AW = longReads ? 13 : 7;
  const size_t maxK = a.maxKFast;
  size_t lds = (size_t)CHUNK_A * AW * 4 + maxK * (5 * 4 + 2) + 4 + 64;  // accumulators | sLo, pre, lstStart, lstLen, lstDir, qOf
  const size_t bitmapWords = 2 * (((size_t)a.ref.nAlleles + 31) / 32);        // chunk selection: two bitmaps over all alleles ...
  if (bitmapWords > (size_t)CHUNK_A * AW) lds += bitmapWords * 4 + 8;         // ... behind the list arrays when the accumulators cannot hold them
  if (a.ref.kDirStride - 1 > 256) return t1k_fail(ctx, T1K_ERR_ARG, "the reference holds more than 131 072 distinct sequences (256 seeding chunks)");
  if (lds > 160 * 1024) return t1k_fail(ctx, T1K_ERR_ARG, "the reference holds too many sequences for the seeding kernel's LDS bitmaps");
  // the seeding kernel keeps no per-workgroup HBM scratch: one workgroup per read-end (up to 32768) balances their uneven cost best
  const int seedWg = (int)std::min<uint32_t>(a.reads.nReadEnds, 32768u);
  if (longReads) {
    T1K_HIP(ctx, hipFuncSetAttribute((const void *)k_seed_groups<10>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_seed_groups<10>, dim3(seedWg), dim3(WG), lds, ctx->stream, a);
  } else {
    T1K_HIP(ctx, hipFuncSetAttribute((const void *)k_seed_groups<5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_seed_groups<5>, dim3(seedWg), dim3(WG), lds, ctx->stream, a);
  }
  if (xlong) {
    const size_t ldsLong = (size_t)a.maxK * (4 * 4 + 2) + 8 + (size_t)LONG_CH * 4;
    T1K_HIP(ctx, hipFuncSetAttribute((const void *)k_seed_long, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsLong));
    hipLaunchKernelGGL(k_seed_long, dim3(seedWg), dim3(WG), ldsLong, ctx->stream, a);
  }
  return 0;
}
