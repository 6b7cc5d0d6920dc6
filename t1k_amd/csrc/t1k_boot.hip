// t1k_amd/csrc/t1k_boot.hip -- genotyper --bootstrap: B Poisson-bootstrap replicates of the EM's read counts and one EM update
// for all of them in one pass over the structure t1k_em_setup left on the context (rowPtr, ecIdx, colPtr, rowOf: read, never copied).
//
// The replicates share the sparse structure and differ in the group counts and the abundance vectors only: B independent chains of
// double additions over the SAME entries.  So a lane is a replicate: a wavefront walks a row (a class) once, the entry index is
// wave-uniform, and every lane adds its own replicate's operand to its own chain -- the reference's order for every replicate, 64 chains
// at the price of one, no LDS.  The per-replicate arrays are replicate-minor and padded to whole blocks of 64 (stride Rpad):
//   count[g][Rpad]  psum[g][Rpad]  k[g][Rpad]  x[e][Rpad]  n[e][Rpad]
// so that what the 64 lanes of a wavefront load is one 512-byte line.
//   k_boot_resample : k and c' = c * k / n_g of every (group, replicate); the lanes of a wavefront share the draws of a large n_g
//   k_boot_rows     : one wavefront per (read group, block of 64 replicates): psum = sum_j x[ec_j] in row order (psum == 0 -> 1)
//   k_boot_cols     : one wavefront per (class, block): n[ec] = sum over its entries in group order of count[g] * (x[ec] / psum[g])
// A replicate's doubles are those of k_em_psum / k_em_cols on its counts.  The M-step runs on the host (t1k_boot_update), as
// t1k_em_update's does, over the same replicate-minor arrays.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"

namespace {

constexpr int BOOT_LANES = 64;        // replicates per block: one per lane
constexpr int BOOT_U = 8;             // entries whose operands are requested ahead of the additions (k_em_cols: EM_K pieces)
constexpr uint32_t BOOT_SHARE = 64;   // draws per (group, replicate) from which the lanes of a wavefront share them
constexpr uint32_t BOOT_MAX_N = 1u << 27;  // largest n_g: 20 n_g, the largest k there is, stays below 2^32
static_assert(BOOT_LANES == 64, "a block of replicates is one wavefront");

// T_k = floor(2^64 * e^-1 * sum_{j <= k} 1 / j!), k = 0 .. 19: the Poisson(1) draw of a uniform 64-bit u is the number of k with u >= T_k
#define BOOT_T(k) kBootT##k
constexpr unsigned long long kBootT0 = 0x5e2d58d8b3bcdf1aull, kBootT1 = 0xbc5ab1b16779be35ull, kBootT2 = 0xeb715e1dc1582dc2ull, kBootT3 = 0xfb23979734a252f1ull,
                             kBootT4 = 0xff1025f59174dc3dull, kBootT5 = 0xffd90f3ba4055e19ull, kBootT6 = 0xfffa8b71fc72c913ull, kBootT7 = 0xffff540c0914b3c9ull,
                             kBootT8 = 0xffffed1f4aa8f120ull, kBootT9 = 0xfffffe216e641462ull, kBootT10 = 0xffffffd4d85d3183ull, kBootT11 = 0xfffffffc6da262b4ull,
                             kBootT12 = 0xffffffffba12d178ull, kBootT13 = 0xfffffffffb07c64cull, kBootT14 = 0xffffffffffab8ea5ull, kBootT15 = 0xfffffffffffabe22ull,
                             kBootT16 = 0xffffffffffffb11aull, kBootT17 = 0xfffffffffffffba1ull, kBootT18 = 0xffffffffffffffc5ull, kBootT19 = 0xfffffffffffffffdull;

__host__ __device__ __forceinline__ unsigned long long bootMix(unsigned long long z) {  // (the finaliser of splitmix64)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the hash of (seed, replicate, group), before the draw index goes in
__host__ __device__ __forceinline__ unsigned long long bootKey(unsigned long long seed, unsigned long long r, unsigned long long g) {
  return bootMix(bootMix(seed ^ (r * 0xD1342543DE82EF95ull)) ^ g);
}
__host__ __device__ __forceinline__ uint32_t bootPoisson(unsigned long long u) {
  uint32_t c = (uint32_t)(u >= BOOT_T(0)) + (uint32_t)(u >= BOOT_T(1)) + (uint32_t)(u >= BOOT_T(2)) + (uint32_t)(u >= BOOT_T(3));
  if (u >= BOOT_T(3)) {  // 1.9 % of the draws
    c += (uint32_t)(u >= BOOT_T(4)) + (uint32_t)(u >= BOOT_T(5)) + (uint32_t)(u >= BOOT_T(6)) + (uint32_t)(u >= BOOT_T(7));
    if (u >= BOOT_T(7))
      c += (uint32_t)(u >= BOOT_T(8)) + (uint32_t)(u >= BOOT_T(9)) + (uint32_t)(u >= BOOT_T(10)) + (uint32_t)(u >= BOOT_T(11)) + (uint32_t)(u >= BOOT_T(12)) +
           (uint32_t)(u >= BOOT_T(13)) + (uint32_t)(u >= BOOT_T(14)) + (uint32_t)(u >= BOOT_T(15)) + (uint32_t)(u >= BOOT_T(16)) + (uint32_t)(u >= BOOT_T(17)) +
           (uint32_t)(u >= BOOT_T(18)) + (uint32_t)(u >= BOOT_T(19));
  }
  return c;
}

// the wavefront of a launch of 256-thread workgroups -> (item, block of replicates); blocks of one item are neighbours: they read the
// same structure entries
__device__ __forceinline__ bool bootWave(uint32_t nItems, uint32_t nBlk, uint32_t &item, uint32_t &blk) {
  const uint64_t w = (uint64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6));
  item = (uint32_t)(w / nBlk);
  blk = (uint32_t)(w - (uint64_t)item * nBlk);
  return item < nItems;
}

// k[g][r] and c'[g][r].  Replicate 0 is the data (k = n_g), a padding replicate (r >= nRep) is empty (k = 0).  k is an integer sum: for
// n_g >= BOOT_SHARE the wavefront takes the block's replicates one after the other, lane l draws i = l, l + 64, ...
__global__ __launch_bounds__(256) void k_boot_resample(const double *count, const uint32_t *nOf, uint32_t nGroups, uint32_t nRep, uint32_t Rpad, unsigned long long seed,
                                                       int identity, uint32_t *kOut, double *cOut, uint32_t *nonEmpty) {
  uint32_t g, blk;
  if (!bootWave(nGroups, Rpad >> 6, g, blk)) return;
  const int lane = threadIdx.x & 63;
  const uint32_t r = blk * BOOT_LANES + lane;
  const uint32_t n = nOf[g];
  const double c = count[g];
  uint32_t k = 0;
  if (identity) k = r < nRep ? n : 0u;
  else if (n < BOOT_SHARE) {
    if (r == 0) k = n;
    else if (r < nRep) {
      const unsigned long long h = bootKey(seed, r, g);
      for (uint32_t i = 0; i < n; ++i) k += bootPoisson(bootMix(h ^ i));
    }
  } else {
    for (uint32_t j = 0; j < BOOT_LANES; ++j) {
      const uint32_t rr = blk * BOOT_LANES + j;  // (wave-uniform)
      if (rr == 0 || rr >= nRep) continue;
      const unsigned long long h = bootKey(seed, rr, g);
      uint32_t part = 0;
      for (uint32_t i = lane; i < n; i += BOOT_LANES) part += bootPoisson(bootMix(h ^ i));
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) part += (uint32_t)__shfl_xor((int)part, d, 64);
      if (lane == (int)j) k = part;
    }
    if (r == 0) k = n;
  }
  const double cr = c * (double)k / (double)n;  // one multiplication, then one division
  const size_t at = (size_t)g * Rpad + r;
  kOut[at] = k;
  cOut[at] = cr;
  if (r < nRep && cr != 0) nonEmpty[r] = 1u;  // (every writer writes 1)
}

// one wavefront per (read group, block): lane = replicate, the class index of an entry is wave-uniform, x[ec][lane] one line
__global__ __launch_bounds__(256) void k_boot_rows(const uint64_t *rowPtr, const uint32_t *ecIdx, const double *x, double *psumOut, const uint8_t *active, uint32_t nGroups,
                                                   uint32_t Rpad) {
  uint32_t g, blk;
  if (!bootWave(nGroups, Rpad >> 6, g, blk)) return;
  const uint32_t r = blk * BOOT_LANES + (threadIdx.x & 63);
  const bool act = active[r] != 0;
  if (__ballot(act) == 0) return;
  const uint64_t b = rowPtr[g], e = rowPtr[g + 1];
  const double *xr = x + r;
  double psum = 0;
  uint64_t p = b;
  for (; p + BOOT_U <= e; p += BOOT_U) {
    double v[BOOT_U];
#pragma unroll
    for (int u = 0; u < BOOT_U; ++u) v[u] = xr[(size_t)ecIdx[p + u] * Rpad];
#pragma unroll
    for (int u = 0; u < BOOT_U; ++u) psum += v[u];
  }
  for (; p < e; ++p) psum += xr[(size_t)ecIdx[p] * Rpad];
  if (psum == 0) psum = 1;
  if (act) psumOut[(size_t)g * Rpad + r] = psum;
}

// one wavefront per (class, block): the class's entries in group order; the group index is wave-uniform.  The chain of additions is the
// critical path: count / psum of the next BOOT_U entries are requested before the additions of these BOOT_U start, their contributions
// (a division each) are formed before the chain needs them.
__global__ __launch_bounds__(256) void k_boot_cols(const uint64_t *colPtr, const uint32_t *rowOf, const double *count, const double *psum, const double *x, double *n,
                                                   const uint8_t *active, uint32_t nEc, uint32_t Rpad) {
  constexpr int U = BOOT_U;
  uint32_t ec, blk;
  if (!bootWave(nEc, Rpad >> 6, ec, blk)) return;
  const uint32_t r = blk * BOOT_LANES + (threadIdx.x & 63);
  const bool act = active[r] != 0;
  if (__ballot(act) == 0) return;
  const uint64_t b = colPtr[ec], e = colPtr[ec + 1];
  const double xe = x[(size_t)ec * Rpad + r];
  const double *cr = count + r, *pr = psum + r;
  double c[U], ps[U];
  auto values = [&](uint64_t start) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t p = start + u;
      const bool ok = p < e;  // (wave-uniform)
      const size_t at = ok ? (size_t)rowOf[p] * Rpad : 0;
      c[u] = ok ? cr[at] : 0.0;
      ps[u] = ok ? pr[at] : 1.0;
    }
  };
  double s = 0;
  if (b < e) values(b);
  for (uint64_t base = b; base < e; base += U) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = c[u] * (xe / ps[u]);
    values(base + U);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u < e) s += v[u];
  }
  if (act) n[(size_t)ec * Rpad + r] = s;
}

uint32_t bootStride(uint32_t nReplicates) { return (nReplicates + 1 + BOOT_LANES - 1) / BOOT_LANES * BOOT_LANES; }

void bootRelease(t1k_ctx *ctx) {
  T1kBoot &B = ctx->boot;
  if (B.pinned) (void)hipHostFree(B.pinned);
  if (ctx->bBoot.p) (void)t1k_dev_free(ctx->bBoot.p);
  ctx->bBoot.p = nullptr; ctx->bBoot.bytes = 0;
  B = T1kBoot();
}

}  // namespace

extern "C" {

int t1k_boot_begin(t1k_ctx *ctx, uint32_t nReplicates, uint64_t seed, int identity) {
  if (!ctx) return T1K_ERR_ARG;
  if (nReplicates < 1 || nReplicates > 1000) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_boot_begin: 1 .. 1000 replicates");
  if (!ctx->bEmColPtr.p) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_boot_begin: t1k_em_setup has not run on this context");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  bootRelease(ctx);
  T1kBoot &B = ctx->boot;
  const uint32_t G = ctx->emGroups, E = ctx->emEc, Rpad = bootStride(nReplicates);
  // n_g = max(1, llrint(c_g)) on the host (round to nearest, ties to even)
  std::vector<double> count(G);
  if (G) T1K_HIP(ctx, hipMemcpy(count.data(), ctx->bEmCount.p, (size_t)G * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> nOf(G);
  for (uint32_t g = 0; g < G; ++g) {
    if (!std::isfinite(count[g]) || count[g] < 0 || count[g] > (double)BOOT_MAX_N)
      return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_boot_begin: the count of read group " + std::to_string(g) + " is not in 0 .. 2^27");
    nOf[g] = (uint32_t)std::max<long long>(1, llrint(count[g]));
  }
  T1kCarve piece;
  B.oCount = piece((size_t)G * Rpad * 8); B.oPsum = piece((size_t)G * Rpad * 8); B.oK = piece((size_t)G * Rpad * 4);
  B.oX = piece((size_t)E * Rpad * 8); B.oN = piece((size_t)E * Rpad * 8); B.oNOf = piece((size_t)G * 4); B.oActive = piece(Rpad); B.oNonEmpty = piece((size_t)Rpad * 4);
  int rc;
  if ((rc = t1k_ensure(ctx, ctx->bBoot, piece.off))) return rc;
  char *D = (char *)ctx->bBoot.p;
  hipStream_t st = ctx->stream;
  T1K_HIP(ctx, hipMemsetAsync(D, 0, piece.off, st));  // (psum, x and n of a lane are read before that lane was ever active: defined values)
  if (G) T1K_HIP(ctx, hipMemcpyAsync(D + B.oNOf, nOf.data(), (size_t)G * 4, hipMemcpyHostToDevice, st));
  if (G) {
    const uint64_t waves = (uint64_t)G * (Rpad >> 6);
    hipLaunchKernelGGL(k_boot_resample, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, (const double *)ctx->bEmCount.p, (const uint32_t *)(D + B.oNOf), G, nReplicates + 1,
                       Rpad, (unsigned long long)seed, identity ? 1 : 0, (uint32_t *)(D + B.oK), (double *)(D + B.oCount), (uint32_t *)(D + B.oNonEmpty));
    T1K_HIP(ctx, hipGetLastError());
  }
  std::vector<uint32_t> ne(Rpad);
  T1K_HIP(ctx, hipMemcpyAsync(ne.data(), D + B.oNonEmpty, (size_t)Rpad * 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  B.nonEmpty.assign(Rpad, 0);
  for (uint32_t r = 0; r < Rpad; ++r) B.nonEmpty[r] = ne[r] ? 1 : 0;
  if (E) T1K_HIP(ctx, hipHostMalloc((void **)&B.pinned, (size_t)E * Rpad * 16, hipHostMallocDefault));
  B.open = true; B.nRep = nReplicates + 1; B.Rpad = Rpad;
  return T1K_OK;
}

uint32_t t1k_boot_stride(uint32_t nReplicates) { return bootStride(nReplicates); }

int t1k_boot_nonempty(t1k_ctx *ctx, uint8_t *nonEmpty) {
  if (!ctx || !nonEmpty) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_boot_nonempty: bad arguments");
  if (!ctx->boot.open) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_boot_nonempty: no bootstrap is open");
  memcpy(nonEmpty, ctx->boot.nonEmpty.data(), ctx->boot.Rpad);
  return T1K_OK;
}

int t1k_boot_counts(t1k_ctx *ctx, uint32_t *k, double *count) {
  if (!ctx) return T1K_ERR_ARG;
  const T1kBoot &B = ctx->boot;
  if (!B.open) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_boot_counts: no bootstrap is open");
  const size_t cells = (size_t)ctx->emGroups * B.Rpad;
  if (!cells) return T1K_OK;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  const char *D = (const char *)ctx->bBoot.p;
  if (k) T1K_HIP(ctx, hipMemcpyAsync(k, D + B.oK, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (count) T1K_HIP(ctx, hipMemcpyAsync(count, D + B.oCount, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return T1K_OK;
}

int t1k_boot_update(t1k_ctx *ctx, const uint8_t *active, const double *x0, double *x1, double *n, double *diff) {
  if (!ctx || !active || !x0 || !x1 || !n || !diff) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_boot_update: bad arguments");
  T1kBoot &B = ctx->boot;
  if (!B.open) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_boot_update: no bootstrap is open");
  const uint32_t E = ctx->emEc, G = ctx->emGroups, Rpad = B.Rpad;
  bool any = false;
  for (uint32_t r = 0; r < Rpad; ++r) {
    if (active[r] && r >= B.nRep) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_boot_update: a padding replicate is marked active");
    any = any || active[r];
  }
  if (!any) return T1K_OK;
  if (E == 0) {
    for (uint32_t r = 0; r < Rpad; ++r) if (active[r]) diff[r] = 0;
    return T1K_OK;
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  char *D = (char *)ctx->bBoot.p;
  const size_t vec = (size_t)E * Rpad;
  double *px = B.pinned, *pn = B.pinned + vec;
  memcpy(px, x0, vec * 8);
  T1K_HIP(ctx, hipMemcpyAsync(D + B.oX, px, vec * 8, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + B.oActive, active, Rpad, hipMemcpyHostToDevice, st));
  const uint32_t nBlk = Rpad >> 6;
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  if (G) hipLaunchKernelGGL(k_boot_rows, dim3((unsigned)(((uint64_t)G * nBlk + 3) / 4)), dim3(256), 0, st, (const uint64_t *)ctx->bEmRowPtr.p, (const uint32_t *)ctx->bEmEc.p,
                            (const double *)(D + B.oX), (double *)(D + B.oPsum), (const uint8_t *)(D + B.oActive), G, Rpad);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  hipLaunchKernelGGL(k_boot_cols, dim3((unsigned)(((uint64_t)E * nBlk + 3) / 4)), dim3(256), 0, st, (const uint64_t *)ctx->bEmColPtr.p, (const uint32_t *)ctx->bEmRowOf.p,
                     (const double *)(D + B.oCount), (const double *)(D + B.oPsum), (const double *)(D + B.oX), (double *)(D + B.oN), (const uint8_t *)(D + B.oActive), E, Rpad);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  T1K_HIP(ctx, hipMemcpyAsync(pn, D + B.oN, vec * 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  float t = 0;
  if (hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]) == hipSuccess) B.ms[0] += t;
  if (hipEventElapsedTime(&t, ctx->ev[1], ctx->ev[2]) == hipSuccess) B.ms[1] += t;
  B.ms[2] += 1;
  // M-step (Genotyper.hpp:406-420) of every active replicate: per replicate the sums run over the classes in class order, as t1k_em_update's
  const std::vector<int32_t> &len = ctx->hEmLen;
  std::vector<double> norm(Rpad, 0.0), d(Rpad, 0.0);
  for (uint32_t e = 0; e < E; ++e) {
    const double *src = pn + (size_t)e * Rpad;
    double *dst = n + (size_t)e * Rpad;
    const double l = len[e];
    for (uint32_t r = 0; r < Rpad; ++r)
      if (active[r]) { dst[r] = src[r]; norm[r] += src[r] / l; }
  }
  for (uint32_t e = 0; e < E; ++e) {
    const double *nn = n + (size_t)e * Rpad, *from = x0 + (size_t)e * Rpad;
    double *to = x1 + (size_t)e * Rpad;
    const double l = len[e];
    for (uint32_t r = 0; r < Rpad; ++r)
      if (active[r]) {
        const double v = nn[r] / l / norm[r];
        d[r] += std::fabs(v - from[r]);
        to[r] = v;
      }
  }
  for (uint32_t r = 0; r < Rpad; ++r) if (active[r]) diff[r] = d[r];
  return T1K_OK;
}

void t1k_boot_end(t1k_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  bootRelease(ctx);
}

void t1k_boot_limits(uint32_t out[3]) { out[0] = BOOT_U; out[1] = BOOT_SHARE; out[2] = BOOT_LANES; }
void t1k_boot_times(const t1k_ctx *ctx, double ms3[3]) { for (int i = 0; i < 3; ++i) ms3[i] = ctx ? ctx->boot.ms[i] : 0; }

int t1k_em_set_count(t1k_ctx *ctx, const double *count) {
  if (!ctx || (!count && ctx->emGroups)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_em_set_count: bad arguments");
  if (!ctx->bEmColPtr.p) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_em_set_count: t1k_em_setup has not run on this context");
  if (!ctx->emGroups) return T1K_OK;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  T1K_HIP(ctx, hipMemcpyAsync(ctx->bEmCount.p, count, (size_t)ctx->emGroups * 8, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return T1K_OK;
}

}  // extern "C"
