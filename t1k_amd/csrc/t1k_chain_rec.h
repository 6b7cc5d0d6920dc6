// t1k_amd/csrc/t1k_chain_rec.h -- internal: what the writer of a group record (seeding, t1k_seed.hip) and its readers (chaining and
// collection, t1k_chain.hip) have to agree on.
//
// A record is recStride u32 (8: reads <= 160 bp, 16: reads <= 320 bp), one per (read-end, strand, allele) group:
//   as seeded:      0 re | '+' strand << 31, 1 allele, 2 diagonal + stray counts (packDiagMeta), 3.. M (bitmask of the read offsets on the diagonal)
//   after chaining: 2 state (REC_DONE | number of candidates, or the number of memo slots still to be added: recPending), 3..5 packed candidate
//                   (3 = side-arena base for multi-diagonal groups), 6..7 memo slots still to be added
#pragma once
#include "t1k_dev.h"

#define WG 256
#define CHUNK_A T1K_SEED_CHUNK   // alleles per seeding chunk: one LDS accumulator each
#define DIAG_EMPTY 0x7FFFFFFF    // diagonal of an accumulator no hit has reached
#define GROUP_MAX_REFS 4         // two 32-bit words of 16-bit memo slots in a group record

// record word 2 before chaining: reference diagonal (22 bits, biased; alleles are shorter than 2^20 bases) and the counts of hits off
// it: FAR = beyond `radius` diagonals (bits 22..24, saturating at 7) and NEAR = within `radius` (bits 25..29, saturating at 31) -- the
// chain asks "near > 0" and "far > 2" (several diagonals: the general path), k_near_hits asks for "far == 0" and the exact near count
// (31 = unknown).  Bits 30 and 31 stay clear: after chaining the word holds the state, whose REC_DONE is bit 31.
#define REC_DIAG_BIAS (1 << 21)
#define REC_DIAG_MIN (-(1 << 20))  // diagonal = read offset - allele offset > -(allele length)
__device__ __forceinline__ uint32_t packDiagMeta(int diag, uint32_t meta) {
  const uint32_t strays = meta & 0xFFFFu, nearCnt = meta >> 16;  // (strays counts every hit off the reference diagonal, near ones included)
  return (uint32_t)(diag + REC_DIAG_BIAS) | (min(strays - nearCnt, 7u) << 22) | (min(nearCnt, 31u) << 25);
}
__device__ __forceinline__ int recDiag(uint32_t w2) { return (int)(w2 & 0x3FFFFFu) - REC_DIAG_BIAS; }
__device__ __forceinline__ uint32_t recFar(uint32_t w2) { return (w2 >> 22) & 7u; }
__device__ __forceinline__ uint32_t recNear(uint32_t w2) { return (w2 >> 25) & 31u; }
__device__ __forceinline__ bool recIsGeneral(uint32_t w2) { return recNear(w2) > 0 || recFar(w2) > 2; }
#define REC_NEAR_DONE 0x4E454152u  // record word 5 of a multi-diagonal group whose hit list k_near_hits wrote (k_gather_general leaves it alone)
enum { REC_DONE = 0x80000000u };  // word 2 after chaining: REC_DONE | number of candidates (general groups: bit 30 = candidates in the side arena)
__device__ __forceinline__ bool recPending(uint32_t state) { return !(state & REC_DONE) && state >= 1u && state <= (uint32_t)GROUP_MAX_REFS; }
// The closed-form pass leaves a group without a candidate as seeding wrote it, so a reader of word 2 tells three things apart by value alone:
// REC_DONE set = chained; 1..GROUP_MAX_REFS = a candidate waiting for that many memo slots; anything else = the diagonal word, no candidate.
// That holds as long as the diagonal word can be mistaken for neither:
static_assert(REC_DIAG_MIN + REC_DIAG_BIAS > GROUP_MAX_REFS, "the biased diagonal of an untouched record must not read as a pending count");
static_assert(REC_DIAG_BIAS + T1K_MAX_READ_LEN <= (1 << 22), "the largest diagonal (a read offset of k_seed_groups) must fit the 22 bits with its bias");
static_assert((0x3FFFFFu | (7u << 22) | (31u << 25)) < (1u << 30), "packDiagMeta must leave bits 30 (side arena) and 31 (REC_DONE) clear");
