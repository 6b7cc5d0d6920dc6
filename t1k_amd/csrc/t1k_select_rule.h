// The selection's emit rule on a list in candidate order (k_select's CUT instantiations, t1k_assign.hip), as plain functions that the
// kernel and the host harness (tests/harness/select_emit_san.cpp) both compile.
//
// The selection orders a read-end's candidates by `<`: class on the seed coordinates and allele (the packed key above the candidate
// number), then candBeforeFull (read start, read end, allele start, allele end of the seed), then the candidate number.  What it emits
// needs no sort, only two order statistics of the list:
//   L     the `<`-smallest candidate without a separator in its seed whose extension failed (the latch: SeqSet.hpp:2170-2172); may not exist
//   good  the largest seed match count among the candidates without separator, with a passed extension, that lie before L (all of them
//         if there is no L; -1 if there are none)
//   candidate c is emitted iff it has no separator, its extension passed, and not (L < c and seed(c) < good and not KEEPCLIP)
// Candidates whose class and allele equal L's (rare: two candidates on one allele in one seed class) are settled exactly with the
// remaining fields: SelTie packs them into two words whose unsigned order is candBeforeFull's, then the candidate number's.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define T1K_SEL_FN __host__ __device__ __forceinline__
#else
#define T1K_SEL_FN inline
#endif

#define SEL_F_SEPSEED 1u
#define SEL_F_EXTOK 2u
#define SEL_F_KEEPCLIP 4u
// what the flags become once L is known (the same three bits of the key): the candidate can be emitted, it lies behind L, and KEEPCLIP;
// after the decision SEL_M_EMIT alone is read: the candidate is emitted
#define SEL_M_EMIT 1u
#define SEL_M_BEHIND 2u

struct SelTie { uint64_t hi, lo; };  // (read start, read end, allele start) | (allele end, candidate number)
T1K_SEL_FN SelTie selTieOf(uint32_t readSE, int32_t seqStart, int32_t seqEnd, uint32_t idx) {
  SelTie t;
  t.hi = (uint64_t)(readSE & 0xFFFFu) << 48 | (uint64_t)(readSE >> 16) << 32 | (uint64_t)((uint32_t)seqStart ^ 0x80000000u);  // (sign bit flipped: the signed order)
  t.lo = (uint64_t)((uint32_t)seqEnd ^ 0x80000000u) << 32 | (uint64_t)idx;
  return t;
}
T1K_SEL_FN bool selTieBefore(const SelTie &a, const SelTie &b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

T1K_SEL_FN bool selLatchCand(uint32_t fl) { return !(fl & SEL_F_SEPSEED) && !(fl & SEL_F_EXTOK); }
T1K_SEL_FN bool selEmitCand(uint32_t fl) { return !(fl & SEL_F_SEPSEED) && (fl & SEL_F_EXTOK); }
// does candidate c (class and allele `ca`) lie before L; `tie` is only read when the two classes and alleles are equal
template <class TieFn>
T1K_SEL_FN bool selBeforeLatch(uint64_t ca, uint64_t caL, const SelTie &tieL, TieFn tie) {
  if (ca != caL) return ca < caL;
  return selTieBefore(tie(), tieL);
}
// the three bits of a candidate once L is known
T1K_SEL_FN uint32_t selMarks(uint32_t fl, bool hasLatch, bool beforeLatch) {
  return (selEmitCand(fl) ? SEL_M_EMIT : 0u) | ((hasLatch && !beforeLatch) ? SEL_M_BEHIND : 0u) | (fl & SEL_F_KEEPCLIP);
}
// counts towards `good`
T1K_SEL_FN bool selCountsForGood(uint32_t marks) { return (marks & SEL_M_EMIT) && !(marks & SEL_M_BEHIND); }
T1K_SEL_FN bool selEmit(uint32_t marks, int seed, int good) {
  return (marks & SEL_M_EMIT) && !((marks & SEL_M_BEHIND) && seed < good && !(marks & SEL_F_KEEPCLIP));
}

// Compaction of the emitted candidates in candidate order: bits[w] holds the emit marks of candidates 64 w .. 64 w + 63, wordBase[w]
// the number of marks in the words before w (one exclusive prefix over the words); a marked candidate's place among the emitted:
T1K_SEL_FN uint32_t selBitPos(const uint64_t *bits, const uint32_t *wordBase, uint32_t i) {
  const uint64_t below = (i & 63u) ? (bits[i >> 6] & (~0ull >> (64 - (i & 63u)))) : 0ull;
  return wordBase[i >> 6] + (uint32_t)__builtin_popcountll(below);
}
