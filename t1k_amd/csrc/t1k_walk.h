// t1k_amd/csrc/t1k_walk.h -- internal: the edit-string walk of one alignment by one wave64, shared by k_pileup (t1k_pileup.hip) and
// k_sitepile (t1k_sitepile.hip).  64 edit columns per step.  A lane's allele coordinate is seq_start + the non-insert ops before it, its
// read coordinate the non-delete ops before it: a ballot, a population count below the lane, and wave-uniform running totals -- no lane
// walks the string.  The loop control is wave-uniform, so the per-column callback runs with all 64 lanes converged and may itself use
// cross-lane operations.
#pragma once
#include "t1k_dev.h"

enum { PILEUP_PLANES = 14, PILEUP_N = 4, PILEUP_DEL = 5, PILEUP_INS = 6, PILEUP_UNIQ = 7 };
enum { PILEUP_BAD_OP = 1, PILEUP_BAD_ALLELE_WALK = 2, PILEUP_BAD_TEXT_WALK = 4 };

__device__ __forceinline__ uint32_t pileupUniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long pileupUniform64(unsigned long long v) {
  return ((unsigned long long)pileupUniform((uint32_t)(v >> 32)) << 32) | pileupUniform((uint32_t)v);
}
__device__ __forceinline__ uint32_t pileupBelow(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the counter plane of a column that is no gap: the read base, anything but A/C/G/T as N
__device__ __forceinline__ uint32_t pileupBasePlane(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : (uint32_t)PILEUP_N; }

struct PileupWalkEnd {
  unsigned long long t, p;  // allele position behind the last column, read bases consumed
  uint32_t bad;             // CHECK: PILEUP_BAD_OP if some op lies outside 0 .. 3
};

// ops[opsAt .. opsAt + nOps) from allele position seqStart of an allele of `len` bases; nOps, seqStart and len are wave-uniform.
// COLUMNS: column(active, op, pos, readPos) once per step on every lane -- active: the lane has a column; pos: the allele position the
// column books at (an insert: the position consumed last, seq_start if none yet, clamped to the allele's last position; with len == 0
// or on a walk that leaves the allele pos may lie outside 0 .. len - 1, which the check reports); readPos: the read bases in front of it.
template <bool CHECK, bool COLUMNS, class F>
__device__ __forceinline__ PileupWalkEnd pileupWalk(const int8_t *ops, unsigned long long opsAt, uint32_t nOps, uint32_t seqStart, unsigned long long len, uint32_t lane, F &&column) {
  unsigned long long t = seqStart, p = 0;
  uint32_t bad = 0;
  for (uint32_t c0 = 0; c0 < nOps; c0 += 64u) {
    const uint32_t col = c0 + lane;
    const bool active = col < nOps;
    const int op = active ? (int)ops[opsAt + col] : -1;
    const bool isT = active && op != 2, isP = active && op != 3;
    const uint64_t mT = __ballot(isT ? 1 : 0), mP = __ballot(isP ? 1 : 0);
    if (COLUMNS) {
      const unsigned long long myT = t + pileupBelow(mT), myP = p + pileupBelow(mP);
      unsigned long long pos = myT;
      if (op == 2) {
        pos = myT > seqStart ? myT - 1 : myT;   // the allele position consumed last; none yet: seq_start
        if (pos >= len) pos = len - 1;            // (an all-insert window at the allele's end)
      }
      column(active, op, pos, myP);
    }
    if (CHECK) bad |= __ballot((active && (op < 0 || op > 3)) ? 1 : 0) ? (uint32_t)PILEUP_BAD_OP : 0u;
    t += (uint32_t)__popcll(mT);
    p += (uint32_t)__popcll(mP);
  }
  return PileupWalkEnd{t, p, bad};
}
