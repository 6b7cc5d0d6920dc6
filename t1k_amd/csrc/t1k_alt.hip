// t1k_amd/csrc/t1k_alt.hip -- runner-up evidence per called allele (genotyper --alternatives).  Stateless: one call, nothing
// kept on the context.
//
// Input: the read groups as a CSR (groupPtr, the allele of every entry, ascending inside a group), the fixed-point weight q of every group,
// the gene of every allele and slotOf[a] = 2 * gene + k for the allele called in slot k of its gene (0xFFFFFFFF otherwise).  Output: four
// dense uint64 tables over the alleles -- total, both0, both1, neither (include/t1k_gpu.h has the definition).  Integers only: the sums are
// 64-bit global atomic adds and come out the same for every launch shape, piece size and arrival order.
//
// k_alt_groups: one wave64 per group, four waves per workgroup, grid-stride.  Every wave owns a bitset of 2 * nGenes bits in LDS, one bit
// per slot, all clear between two groups:
//   sweep 1  marks the slots of the called alleles the group holds (ds_or);
//   sweep 2  reads, for every entry, the two slot bits of its gene -- bits 2g and 2g + 1 share a word -- and adds q to total[a], to both0[a]
//            / both1[a] where the bit is set and to neither[a] where none is;
//   sweep 3  clears the words sweep 1 touched, so that the cost of a group is its entries and not the number of genes.
// A wave's LDS instructions are executed in program order, so a fence (lgkmcnt(0), and no reordering by the compiler) between the sweeps is
// all that is needed: no workgroup barrier inside the loop, and the waves of a workgroup never wait for one another.  Groups of up to 64
// entries keep the entry in registers and need no loop; longer ones stride the list three times (the second and third time from cache).
// Nothing is checked on the device: the host has been over every index before the first launch (t1k_alt_batch below).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "t1k_dev.h"
#include "t1k_launch.h"

namespace {
constexpr uint32_t kAltEmpty = 0xFFFFFFFFu;
constexpr uint32_t kAltWaves = 4;                     // wavefronts (= bitsets) per workgroup
constexpr uint64_t kAltPieceEntries = 1ull << 24;     // entries uploaded per piece (64 MB); env T1K_ALT_PIECE overrides it
constexpr uint32_t kAltMaxWords = (64u << 10) / (4u * kAltWaves);  // bitset words per wave that fit 64 KB of LDS: 2 * nGenes <= 131072

struct AltArgs {
  const unsigned long long *groupPtr;  // [nGroups + 1] of the piece, in entries of the whole call
  const uint32_t *ent;                 // the piece's entries; entry e of the call is ent[e - entBase]
  const unsigned long long *q;         // [nGroups]
  const uint32_t *alleleGene, *slotOf; // [nAlleles]
  unsigned long long *tables;          // [4 * nAlleles]: total, both0, both1, neither
  unsigned long long entBase;
  uint32_t nGroups, nAlleles, words;
};

__device__ __forceinline__ uint32_t altUniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long altUniform64(unsigned long long v) {
  return ((unsigned long long)altUniform((uint32_t)(v >> 32)) << 32) | altUniform((uint32_t)v);
}
__device__ __forceinline__ void altAdd(unsigned long long *p, unsigned long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return global_atomic_add_x2
}
// the wave's own LDS traffic so far is done and visible to all its lanes
__device__ __forceinline__ void altSeam() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup", "local");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void altBook(const AltArgs &P, const uint32_t *bits, uint32_t a, unsigned long long q) {
  const uint32_t gene = P.alleleGene[a];
  const uint32_t pair = (bits[gene >> 4] >> ((gene & 15u) * 2u)) & 3u;
  unsigned long long *t = P.tables + a;
  altAdd(t, q);
  if (pair & 1u) altAdd(t + P.nAlleles, q);
  if (pair & 2u) altAdd(t + 2ull * P.nAlleles, q);
  if (pair == 0u) altAdd(t + 3ull * P.nAlleles, q);
}

__global__ __launch_bounds__(64 * kAltWaves) void k_alt_groups(AltArgs P) {
  extern __shared__ uint32_t altBits[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t *bits = altBits + (size_t)wave * P.words;
  for (uint32_t w = lane; w < P.words; w += 64u) bits[w] = 0u;
  altSeam();
  const uint32_t nWaves = gridDim.x * kAltWaves;
  for (unsigned long long g = altUniform(blockIdx.x * kAltWaves + wave); g < P.nGroups; g += nWaves) {  // (64 bits: g + nWaves may pass 2^32)
    const unsigned long long b = altUniform64(P.groupPtr[g]) - P.entBase, n = altUniform64(P.groupPtr[g + 1]) - P.entBase - b;
    const unsigned long long q = altUniform64(P.q[g]);
    const uint32_t *e = P.ent + b;
    if (n <= 64ull) {
      const bool active = lane < (uint32_t)n;
      const uint32_t a = active ? e[lane] : 0u;
      const uint32_t slot = active ? P.slotOf[a] : kAltEmpty;
      if (slot != kAltEmpty) atomicOr(&bits[slot >> 5], 1u << (slot & 31u));
      altSeam();
      if (active) altBook(P, bits, a, q);
      altSeam();
      if (slot != kAltEmpty) bits[slot >> 5] = 0u;
    } else {
      for (unsigned long long i = lane; i < n; i += 64ull) {
        const uint32_t slot = P.slotOf[e[i]];
        if (slot != kAltEmpty) atomicOr(&bits[slot >> 5], 1u << (slot & 31u));
      }
      altSeam();
      for (unsigned long long i = lane; i < n; i += 64ull) altBook(P, bits, e[i], q);
      altSeam();
      for (unsigned long long i = lane; i < n; i += 64ull) {
        const uint32_t slot = P.slotOf[e[i]];
        if (slot != kAltEmpty) bits[slot >> 5] = 0u;
      }
    }
    altSeam();
  }
}

}  // namespace

extern "C" {

int t1k_alt_batch(t1k_ctx *ctx, uint64_t nGroups, const uint64_t *groupPtr, const uint32_t *entryAllele, const uint64_t *q, uint32_t nAlleles, const uint32_t *alleleGene,
                  uint32_t nGenes, const uint32_t *slotOf, uint64_t *tables, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if ((nAlleles && (!tables || !alleleGene || !slotOf)) || (nGroups && (!groupPtr || !q))) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: bad arguments (NULL arrays)");
  // ---- everything the kernel relies on, before anything is written ----
  {
    std::vector<uint8_t> claimed(2ull * nGenes, 0);
    for (uint32_t a = 0; a < nAlleles; ++a) {
      if (alleleGene[a] >= nGenes) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: allele " + std::to_string(a) + " names gene " + std::to_string(alleleGene[a]) + " of " + std::to_string(nGenes));
      const uint32_t s = slotOf[a];
      if (s == kAltEmpty) continue;
      if ((s >> 1) != alleleGene[a]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: slotOf of allele " + std::to_string(a) + " is neither empty nor a slot of its gene");
      if (claimed[s]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: two alleles claim slot " + std::to_string(s & 1u) + " of gene " + std::to_string(s >> 1));
      claimed[s] = 1;
    }
  }
  const uint32_t words = (uint32_t)std::max<uint64_t>(1, (2ull * nGenes + 31) / 32);
  if (words > kAltMaxWords) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_alt_batch: more than " + std::to_string(kAltMaxWords * 16u) + " genes (the slot bitsets of a workgroup exceed its LDS)");
  if (nGroups >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_alt_batch: 2^32 read groups or more");
  if (nGroups) {
    if (groupPtr[0] != 0) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: groupPtr does not start at 0");
    std::string bad = t1k_parallel_check(nGroups, [&](uint64_t g0, uint64_t g1) {
      for (uint64_t g = g0; g < g1; ++g)
        if (groupPtr[g + 1] < groupPtr[g]) return "groupPtr decreases at group " + std::to_string(g);
      return std::string();
    });
    if (!bad.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: " + bad);
    if (groupPtr[nGroups] && !entryAllele) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: bad arguments (NULL entryAllele)");
    bad = t1k_parallel_check(nGroups, [&](uint64_t g0, uint64_t g1) {
      for (uint64_t g = g0; g < g1; ++g)
        for (uint64_t p = groupPtr[g]; p < groupPtr[g + 1]; ++p) {
          if (entryAllele[p] >= nAlleles) return "entry " + std::to_string(p) + " names allele " + std::to_string(entryAllele[p]) + " of " + std::to_string(nAlleles);
          if (p > groupPtr[g] && entryAllele[p] <= entryAllele[p - 1]) return "the entries of group " + std::to_string(g) + " are not strictly ascending by allele";
        }
      return std::string();
    });
    if (!bad.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_alt_batch: " + bad);
    // no table cell can exceed the sum of q over all groups (an allele appears at most once per group)
    uint64_t sum = 0;
    for (uint64_t g = 0; g < nGroups; ++g) {
      if (q[g] >= (1ull << 63) || sum + q[g] >= (1ull << 63)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_alt_batch: the sum of q could pass 2^63");
      sum += q[g];
    }
  }
  if (nGroups == 0 || nAlleles == 0) {
    if (nAlleles) memset(tables, 0, 32ull * nAlleles);
    return T1K_OK;
  }
  const std::vector<uint64_t> cut = t1k_group_pieces(nGroups, groupPtr, kAltPieceEntries, "T1K_ALT_PIECE");
  uint64_t maxEnt = 0, maxGroups = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i) {
    maxEnt = std::max(maxEnt, groupPtr[cut[i + 1]] - groupPtr[cut[i]]);
    maxGroups = std::max(maxGroups, cut[i + 1] - cut[i]);
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  T1kCallBlock blk;  // (freed on every return, behind the stream's work)
  T1kCarve piece;
  const size_t oTab = piece(32ull * nAlleles), oGene = piece(4ull * nAlleles), oSlot = piece(4ull * nAlleles);
  const size_t oPtr = piece(8ull * (maxGroups + 1)), oQ = piece(8ull * maxGroups), oEnt = piece(4ull * maxEnt);
  int rc;
  if ((rc = blk.alloc(ctx, piece.off))) return rc;
  char *D = (char *)blk.buf.p;
  T1K_HIP(ctx, hipMemsetAsync(D + oTab, 0, 32ull * nAlleles, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oGene, alleleGene, 4ull * nAlleles, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oSlot, slotOf, 4ull * nAlleles, hipMemcpyHostToDevice, st));
  AltArgs a{};
  a.groupPtr = (const unsigned long long *)(D + oPtr); a.ent = (const uint32_t *)(D + oEnt); a.q = (const unsigned long long *)(D + oQ);
  a.alleleGene = (const uint32_t *)(D + oGene); a.slotOf = (const uint32_t *)(D + oSlot);
  a.tables = (unsigned long long *)(D + oTab);
  a.nAlleles = nAlleles; a.words = words;
  double ms = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i) {
    const uint64_t g0 = cut[i], g1 = cut[i + 1], e0 = groupPtr[g0], e1 = groupPtr[g1];
    T1K_HIP(ctx, hipMemcpyAsync(D + oPtr, groupPtr + g0, 8ull * (g1 - g0 + 1), hipMemcpyHostToDevice, st));
    T1K_HIP(ctx, hipMemcpyAsync(D + oQ, q + g0, 8ull * (g1 - g0), hipMemcpyHostToDevice, st));
    if (e1 > e0) T1K_HIP(ctx, hipMemcpyAsync(D + oEnt, entryAllele + e0, 4ull * (e1 - e0), hipMemcpyHostToDevice, st));
    a.entBase = e0; a.nGroups = (uint32_t)(g1 - g0);
    T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_alt_groups, dim3(t1k_grid(ctx, g1 - g0, kAltWaves)), dim3(64 * kAltWaves), (size_t)words * 4u * kAltWaves, st, a);
    T1K_HIP(ctx, hipGetLastError());
    T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    T1K_HIP(ctx, hipStreamSynchronize(st));  // the piece's staging arrays are free again
    float t = 0;
    if (hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]) == hipSuccess) ms += t;
  }
  // everything is sound: only now the caller's array
  std::vector<uint64_t> got(4ull * nAlleles);
  T1K_HIP(ctx, hipMemcpyAsync(got.data(), D + oTab, 32ull * nAlleles, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  memcpy(tables, got.data(), 32ull * nAlleles);
  if (kernelMs) *kernelMs = ms;
  return T1K_OK;
}

uint64_t t1k_alt_pieces(uint64_t nGroups, const uint64_t *groupPtr) {
  if (nGroups == 0 || !groupPtr) return 0;
  return (uint64_t)t1k_group_pieces(nGroups, groupPtr, kAltPieceEntries, "T1K_ALT_PIECE").size() - 1;
}

}  // extern "C"
