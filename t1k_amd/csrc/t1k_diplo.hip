// t1k_amd/csrc/t1k_diplo.hip -- weighted co-occurrence of the allele-pair candidates of every gene (genotyper --diplotypes).
// Stateless: one call, nothing kept on the context.
//
// Input: the read groups as a CSR over candidate ids (groupPtr, the id of every entry, strictly ascending inside a group), the fixed-point
// weight q of every group, and candPtr: gene x owns the ids candPtr[x] .. candPtr[x + 1).  Ids are gene-major and ascending, so the
// candidates of one gene are one contiguous segment of a group's list.  Output: per gene a dense n_x * n_x block of uint64 cells, cell
// (i, j), i <= j, the sum of q over the groups that hold both candidates (include/t1k_gpu.h has the definition).  Integers only: the sums
// are 64-bit global atomic adds and come out the same for every launch shape, piece size and arrival order.
//
// k_diplo_groups: one wave64 per group, four waves per workgroup, grid-stride, no LDS, no workgroup barrier.  The group's list is taken in
// chunks of 64: lane l of a chunk keeps its id, the end of its gene's id range and the address of its matrix row less the gene's first id
// in registers.  For every i of the chunk, in turn, the three values of lane i are made wave-uniform (readlane); the lanes j >= i whose
// id lies below the end of i's gene -- the rest of i's segment -- add q to row[id_j], one no-return global_atomic_add_x2 for a stretch
// of one matrix row.  Whether i's segment runs past the chunk is bit 63 of the ballot of those lanes; only then further tiles of 64 ids
// are read for this i, until a tile that the segment does not fill.  So a group costs the sum of its segments' squares / 64 instructions
// (at least one per id), not the square of its length.  A group of up to 64 ids is one chunk and never reads its list twice.
// Nothing is checked on the device: the host has been over every index before the first launch (t1k_diplo_batch below).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "t1k_dev.h"
#include "t1k_launch.h"

namespace {
constexpr uint32_t kDiploWaves = 4;                    // wavefronts per workgroup
constexpr uint64_t kDiploPieceEntries = 1ull << 24;    // entries uploaded per piece (64 MB); env T1K_DIPLO_PIECE overrides it
constexpr uint32_t kDiploMaxCand = 2048;               // candidates per gene
constexpr uint64_t kDiploMaxCells = 1ull << 29;        // cells of all blocks (4 GB)
constexpr uint32_t kDiploNone = 0xFFFFFFFFu;           // id of a lane behind the end of the list: below no gene's end

struct DiploArgs {
  const unsigned long long *groupPtr;  // [nGroups + 1] of the piece, in entries of the whole call
  const uint32_t *ent;                 // the piece's entries; entry e of the call is ent[e - entBase]
  const unsigned long long *q;         // [nGroups]
  const uint32_t *candEnd;             // [nCand]: candPtr[gene + 1] of the candidate's gene
  const unsigned long long *candRow;   // [nCand]: index of cell (local id, 0) of its gene's block, less candPtr[gene] (never negative: n^2 >= n)
  unsigned long long *matrix;
  unsigned long long entBase;
  uint32_t nGroups;
};

__device__ __forceinline__ uint32_t diploUniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long diploUniform64(unsigned long long v) {
  return ((unsigned long long)diploUniform((uint32_t)(v >> 32)) << 32) | diploUniform((uint32_t)v);
}
__device__ __forceinline__ uint32_t diploLane(uint32_t v, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i); }
__device__ __forceinline__ void diploAdd(unsigned long long *p, unsigned long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return global_atomic_add_x2
}

__global__ __launch_bounds__(64 * kDiploWaves) void k_diplo_groups(DiploArgs P) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nWaves = gridDim.x * kDiploWaves;
  for (unsigned long long g = diploUniform(blockIdx.x * kDiploWaves + wave); g < P.nGroups; g += nWaves) {  // (64 bits: g + nWaves may pass 2^32)
    const unsigned long long b = diploUniform64(P.groupPtr[g]) - P.entBase, n = diploUniform64(P.groupPtr[g + 1]) - P.entBase - b;
    const unsigned long long q = diploUniform64(P.q[g]);
    const uint32_t *e = P.ent + b;
    for (unsigned long long c0 = 0; c0 < n; c0 += 64ull) {
      const bool valid = c0 + lane < n;
      const uint32_t id = valid ? e[c0 + lane] : kDiploNone;
      const uint32_t end = valid ? P.candEnd[id] : 0u;
      const unsigned long long row = valid ? P.candRow[id] : 0ull;
      const uint32_t rowLo = (uint32_t)row, rowHi = (uint32_t)(row >> 32);
      const uint32_t m = (uint32_t)std::min<unsigned long long>(64ull, n - c0);
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t endI = diploLane(end, i);
        unsigned long long *rowI = P.matrix + (((unsigned long long)diploLane(rowHi, i) << 32) | diploLane(rowLo, i));
        const bool mine = lane >= i && id < endI;  // (a lane behind the list: kDiploNone is below no end)
        if (mine) diploAdd(rowI + id, q);
        if (!(__ballot(mine) >> 63)) continue;     // the segment ends inside the chunk
        for (unsigned long long t0 = c0 + 64ull; t0 < n; t0 += 64ull) {  // ... or runs on: tiles of 64 behind the chunk
          const uint32_t idT = t0 + lane < n ? e[t0 + lane] : kDiploNone;
          const bool more = idT < endI;
          if (more) diploAdd(rowI + idT, q);
          if (!(__ballot(more) >> 63)) break;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int t1k_diplo_batch(t1k_ctx *ctx, uint64_t nGroups, const uint64_t *groupPtr, const uint32_t *entryCand, const uint64_t *q, uint32_t nGenes, const uint32_t *candPtr, uint64_t *matrix,
                    double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if (!candPtr || (nGroups && (!groupPtr || !q))) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: bad arguments (NULL arrays)");
  // ---- everything the kernel relies on, before anything is written ----
  if (candPtr[0] != 0) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: candPtr does not start at 0");
  uint64_t cells = 0;
  for (uint32_t x = 0; x < nGenes; ++x) {
    if (candPtr[x + 1] < candPtr[x]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: candPtr decreases at gene " + std::to_string(x));
    const uint64_t nx = candPtr[x + 1] - candPtr[x];
    if (nx > kDiploMaxCand) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_diplo_batch: gene " + std::to_string(x) + " has " + std::to_string(nx) + " candidates (at most " + std::to_string(kDiploMaxCand) + ")");
    cells += nx * nx;
    if (cells > kDiploMaxCells) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_diplo_batch: more than 2^29 matrix cells");
  }
  const uint32_t nCand = candPtr[nGenes];
  if (cells && !matrix) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: bad arguments (NULL matrix)");
  if (nGroups >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_diplo_batch: 2^32 read groups or more");
  if (nGroups) {
    if (groupPtr[0] != 0) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: groupPtr does not start at 0");
    std::string bad = t1k_parallel_check(nGroups, [&](uint64_t g0, uint64_t g1) {
      for (uint64_t g = g0; g < g1; ++g)
        if (groupPtr[g + 1] < groupPtr[g]) return "groupPtr decreases at group " + std::to_string(g);
      return std::string();
    });
    if (!bad.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: " + bad);
    if (groupPtr[nGroups] && !entryCand) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: bad arguments (NULL entryCand)");
    bad = t1k_parallel_check(nGroups, [&](uint64_t g0, uint64_t g1) {
      for (uint64_t g = g0; g < g1; ++g)
        for (uint64_t p = groupPtr[g]; p < groupPtr[g + 1]; ++p) {
          if (entryCand[p] >= nCand) return "entry " + std::to_string(p) + " names candidate " + std::to_string(entryCand[p]) + " of " + std::to_string(nCand);
          if (p > groupPtr[g] && entryCand[p] <= entryCand[p - 1]) return "the entries of group " + std::to_string(g) + " are not strictly ascending by candidate";
        }
      return std::string();
    });
    if (!bad.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_diplo_batch: " + bad);
    // no cell can exceed the sum of q over all groups (a pair appears at most once per group)
    uint64_t sum = 0;
    for (uint64_t g = 0; g < nGroups; ++g) {
      if (q[g] >= (1ull << 63) || sum + q[g] >= (1ull << 63)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_diplo_batch: the sum of q could pass 2^63");
      sum += q[g];
    }
  }
  if (nGroups == 0 || cells == 0 || groupPtr[nGroups] == 0) {
    if (cells) memset(matrix, 0, 8ull * cells);
    return T1K_OK;
  }
  // per candidate: the end of its gene's ids, and where its matrix row begins less the gene's first id (so that cell = row + id)
  std::vector<uint32_t> candEnd(nCand);
  std::vector<uint64_t> candRow(nCand);
  {
    uint64_t base = 0;
    for (uint32_t x = 0; x < nGenes; ++x) {
      const uint64_t lo = candPtr[x], nx = candPtr[x + 1] - lo;
      for (uint64_t i = 0; i < nx; ++i) { candEnd[lo + i] = candPtr[x + 1]; candRow[lo + i] = base + i * nx - lo; }
      base += nx * nx;
    }
  }
  const std::vector<uint64_t> cut = t1k_group_pieces(nGroups, groupPtr, kDiploPieceEntries, "T1K_DIPLO_PIECE");
  uint64_t maxEnt = 0, maxGroups = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i) {
    maxEnt = std::max(maxEnt, groupPtr[cut[i + 1]] - groupPtr[cut[i]]);
    maxGroups = std::max(maxGroups, cut[i + 1] - cut[i]);
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  T1kCallBlock blk;  // (freed on every return, behind the stream's work)
  T1kCarve piece;
  const size_t oMat = piece(8ull * cells), oEnd = piece(4ull * nCand), oRow = piece(8ull * nCand);
  const size_t oPtr = piece(8ull * (maxGroups + 1)), oQ = piece(8ull * maxGroups), oEnt = piece(4ull * maxEnt);
  int rc;
  if ((rc = blk.alloc(ctx, piece.off))) return rc;
  char *D = (char *)blk.buf.p;
  T1K_HIP(ctx, hipMemsetAsync(D + oMat, 0, 8ull * cells, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oEnd, candEnd.data(), 4ull * nCand, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oRow, candRow.data(), 8ull * nCand, hipMemcpyHostToDevice, st));
  DiploArgs a{};
  a.groupPtr = (const unsigned long long *)(D + oPtr); a.ent = (const uint32_t *)(D + oEnt); a.q = (const unsigned long long *)(D + oQ);
  a.candEnd = (const uint32_t *)(D + oEnd); a.candRow = (const unsigned long long *)(D + oRow);
  a.matrix = (unsigned long long *)(D + oMat);
  double ms = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i) {  // the matrix stays on the device across the pieces
    const uint64_t g0 = cut[i], g1 = cut[i + 1], e0 = groupPtr[g0], e1 = groupPtr[g1];
    T1K_HIP(ctx, hipMemcpyAsync(D + oPtr, groupPtr + g0, 8ull * (g1 - g0 + 1), hipMemcpyHostToDevice, st));
    T1K_HIP(ctx, hipMemcpyAsync(D + oQ, q + g0, 8ull * (g1 - g0), hipMemcpyHostToDevice, st));
    if (e1 > e0) T1K_HIP(ctx, hipMemcpyAsync(D + oEnt, entryCand + e0, 4ull * (e1 - e0), hipMemcpyHostToDevice, st));
    a.entBase = e0; a.nGroups = (uint32_t)(g1 - g0);
    T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_diplo_groups, dim3(t1k_grid(ctx, g1 - g0, kDiploWaves)), dim3(64 * kDiploWaves), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
    T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    T1K_HIP(ctx, hipStreamSynchronize(st));  // the piece's staging arrays are free again
    float t = 0;
    if (hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]) == hipSuccess) ms += t;
  }
  // every check has passed and every piece has run: only now the caller's array, copied out once
  T1K_HIP(ctx, hipMemcpyAsync(matrix, D + oMat, 8ull * cells, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (kernelMs) *kernelMs = ms;
  return T1K_OK;
}

uint64_t t1k_diplo_pieces(uint64_t nGroups, const uint64_t *groupPtr) {
  if (nGroups == 0 || !groupPtr) return 0;
  return (uint64_t)t1k_group_pieces(nGroups, groupPtr, kDiploPieceEntries, "T1K_DIPLO_PIECE").size() - 1;
}

}  // extern "C"
