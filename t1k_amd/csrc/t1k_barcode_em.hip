// t1k_amd/csrc/t1k_barcode_em.hip -- per-barcode allele EM (analyzer --barcodeEM): every barcode's EM over its own fragment
// groups, the whole iteration loop on the device in one launch.
//
// One wave64 per barcode, four barcodes per 256-thread workgroup, waves taking barcodes through an atomic cursor over a largest-first
// order (barcode sizes are Zipf-like: the biggest ones start first instead of ending the launch).  One update, in the order DESIGN §11
// fixes (so the doubles equal a sequential restatement bit for bit; -ffp-contract=off keeps every product and sum a separate rounding):
//   psum : a lane per group, psum_g = sum of theta over S_g in ascending allele order
//   n    : a lane per local allele, walking the allele's column list (its groups, in group order): n_a += c_g * (theta_a / psum_g)
//   M    : theta'_a = (n_a + alpha*rho_a) / (N_b + alpha) on the same lane, in place (no other lane reads theta_a in this phase)
//   d    : sum |theta' - theta| in ascending allele order through the wave's ordered sum; every lane runs the same chain, so the
//          stop decision is wave-uniform.
// Shapes: a barcode whose state fits the per-wave LDS arena (kArenaWords 4-byte words; T1K_BARCODE_EM_LDS lowers it) is staged there
// whole; a larger one runs the same code on a global scratch block (theta, psum) and the input arrays in place.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include "t1k_dev.h"
#include "t1k_launch.h"

static constexpr int kWaves = 4;              // barcodes (waves) per workgroup
static constexpr uint32_t kArenaWords = 2048; // LDS per wave: 8 KiB -> 4 x 8.5 KiB per workgroup, four workgroups per CU

// words of the LDS arena a barcode needs: theta, n, psum, count (doubles), group starts, column starts (G + 1, L + 1), entries, column list
__host__ __device__ __forceinline__ uint64_t bcWords(uint64_t L, uint64_t G, uint64_t E) { return 4 * L + 4 * G + (G + 1) + (L + 1) + 2 * E; }

struct BcArgs {
  const uint32_t *order;                 // barcodes, largest first
  const uint64_t *bcAllelePtr, *bcGroupPtr, *groupEntryPtr, *colPtr;  // rebased to the slice
  const uint32_t *entryLocal, *colGroup;  // colGroup: per allele column, local group indices in group order (same index space as entries)
  const double *groupCount, *prior;      // prior: alpha * rho per local allele (NULL: alpha == 0)
  double alpha, tol;
  int32_t maxIter;
  uint32_t nBarcodes, budget;
  double *theta, *psum, *n;              // theta / psum: scratch of the global shape; n: the result, laid out as the local alleles
  int32_t *iters;
  unsigned *cursor;
};

__device__ __forceinline__ void waveSync() {
  // the barcode state is written by one lane and read by another of the same wave: LDS in the arena shape, global memory (one CU,
  // one L1) in the other
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// acc + v(lane 0) + ... + v(lane cnt-1) in that order (t1k_em.hip's waveOrderedSum)
__device__ __forceinline__ double orderedSum(double v, int cnt, double acc, double *slot, int lane) {
  slot[lane] = v;
  waveSync();
  for (int j = 0; j < cnt; ++j) acc += slot[j];
  waveSync();
  return acc;
}

// the barcode's arrays: in LDS (32-bit starts relative to the barcode) or the inputs in place (64-bit starts of the slice)
struct View {
  double *theta, *n, *psum;
  const double *cnt;
  const uint32_t *eLocal, *cGroup;
  const uint32_t *gS32, *cS32;
  const uint64_t *gS64, *cS64;
  uint64_t e0;
};

template <bool LDS>
__device__ __forceinline__ uint32_t startAt(const uint32_t *s32, const uint64_t *s64, uint32_t i, uint64_t e0) {
  if constexpr (LDS) return s32[i]; else return (uint32_t)(s64[i] - e0);
}

template <bool LDS>
__device__ void runBarcode(const BcArgs &P, const View &V, uint32_t L, uint32_t G, uint64_t a0, double N, double *slot, int lane, int32_t *itersOut) {
  // start: theta0_a = f_a / N, f_a = sum over a's groups (group order) of c_g / |S_g|
  for (uint32_t a = lane; a < L; a += 64) {
    double f = 0;
    const uint32_t cb = startAt<LDS>(V.cS32, V.cS64, a, V.e0), ce = startAt<LDS>(V.cS32, V.cS64, a + 1, V.e0);
    for (uint32_t j = cb; j < ce; ++j) {
      const uint32_t g = V.cGroup[j];
      f += V.cnt[g] / (double)(startAt<LDS>(V.gS32, V.gS64, g + 1, V.e0) - startAt<LDS>(V.gS32, V.gS64, g, V.e0));
    }
    V.theta[a] = f / N;
  }
  waveSync();
  const double denom = N + P.alpha;
  int32_t it = 0;
  while (it < P.maxIter) {
    for (uint32_t g = lane; g < G; g += 64) {
      double s = 0;
      const uint32_t b = startAt<LDS>(V.gS32, V.gS64, g, V.e0), e = startAt<LDS>(V.gS32, V.gS64, g + 1, V.e0);
      for (uint32_t j = b; j < e; ++j) s += V.theta[V.eLocal[j]];
      V.psum[g] = s;
    }
    waveSync();
    double d = 0;
    for (uint32_t base = 0; base < L; base += 64) {
      const uint32_t a = base + lane;
      double v = 0;
      if (a < L) {
        const double th = V.theta[a];
        double s = 0;
        const uint32_t cb = startAt<LDS>(V.cS32, V.cS64, a, V.e0), ce = startAt<LDS>(V.cS32, V.cS64, a + 1, V.e0);
        for (uint32_t j = cb; j < ce; ++j) {
          const uint32_t g = V.cGroup[j];
          s += V.cnt[g] * (th / V.psum[g]);
        }
        V.n[a] = s;
        const double t = (s + (P.prior ? P.prior[a0 + a] : 0.0)) / denom;
        v = fabs(t - th);
        V.theta[a] = t;
      }
      d = orderedSum(v, (int)min(64u, L - base), d, slot, lane);
    }
    ++it;
    waveSync();
    if (__builtin_amdgcn_readfirstlane(d < P.tol ? 1 : 0)) break;
  }
  if (lane == 0) *itersOut = it;
}

// the next barcode of the largest-first order: lane 0 takes it from the cursor, v_readlane hands it to the wave as a scalar (wave-uniform
// to the compiler, so the loop over barcodes is a scalar loop and no cross-lane read happens under divergence)
__device__ __forceinline__ unsigned nextBarcode(unsigned *cursor, int lane) {
  unsigned got = 0;
  if (lane == 0) got = atomicAdd(cursor, 1u);
  return (unsigned)__builtin_amdgcn_readlane((int)got, 0);
}

__device__ __forceinline__ void oneBarcode(const BcArgs &P, uint32_t b, double *ar, double *slot, int lane) {
  const uint64_t a0 = P.bcAllelePtr[b], g0 = P.bcGroupPtr[b];
  const uint32_t L = (uint32_t)(P.bcAllelePtr[b + 1] - a0), G = (uint32_t)(P.bcGroupPtr[b + 1] - g0);
  const uint64_t e0 = P.groupEntryPtr[g0];
  const uint32_t E = (uint32_t)(P.groupEntryPtr[g0 + G] - e0);
  // N_b = sum of c_g in group order
  double N = 0;
  for (uint32_t base = 0; base < G; base += 64) N = orderedSum(base + lane < G ? P.groupCount[g0 + base + lane] : 0.0, (int)min(64u, G - base), N, slot, lane);
  if (__builtin_amdgcn_readfirstlane(N == 0 ? 1 : 0)) {
    for (uint32_t a = lane; a < L; a += 64) P.n[a0 + a] = 0.0;
    if (lane == 0) P.iters[b] = 0;
  } else if (bcWords(L, G, E) <= P.budget) {
    // stage the barcode in the wave's arena: doubles first (theta, n, psum, count), then the 32-bit tables
    View V;
    V.theta = ar; V.n = ar + L; V.psum = ar + 2 * L;
    double *cnt = ar + 2 * L + G;
    uint32_t *u = (uint32_t *)(ar + 2 * L + 2 * G);
    uint32_t *gS = u, *cS = u + G + 1, *eL = u + G + 1 + L + 1, *cG = eL + E;
    for (uint32_t g = lane; g < G; g += 64) cnt[g] = P.groupCount[g0 + g];
    for (uint32_t g = lane; g <= G; g += 64) gS[g] = (uint32_t)(P.groupEntryPtr[g0 + g] - e0);
    for (uint32_t a = lane; a <= L; a += 64) cS[a] = (uint32_t)(P.colPtr[a0 + a] - e0);
    for (uint32_t j = lane; j < E; j += 64) { eL[j] = P.entryLocal[e0 + j]; cG[j] = P.colGroup[e0 + j]; }
    V.cnt = cnt; V.eLocal = eL; V.cGroup = cG; V.gS32 = gS; V.cS32 = cS; V.gS64 = nullptr; V.cS64 = nullptr; V.e0 = 0;
    waveSync();
    runBarcode<true>(P, V, L, G, a0, N, slot, lane, P.iters + b);
    for (uint32_t a = lane; a < L; a += 64) P.n[a0 + a] = V.n[a];
    waveSync();  // the arena is free before the next barcode is staged
  } else {
    View V;
    V.theta = P.theta + a0; V.n = P.n + a0; V.psum = P.psum + g0;
    V.cnt = P.groupCount + g0; V.eLocal = P.entryLocal + e0; V.cGroup = P.colGroup + e0;
    V.gS32 = nullptr; V.cS32 = nullptr; V.gS64 = P.groupEntryPtr + g0; V.cS64 = P.colPtr + a0; V.e0 = e0;
    runBarcode<false>(P, V, L, G, a0, N, slot, lane, P.iters + b);
  }
}

__global__ __launch_bounds__(256) void k_barcode_em(BcArgs P) {
  __shared__ __attribute__((aligned(16))) double sArena[kWaves][kArenaWords / 2];
  __shared__ __attribute__((aligned(16))) double sOrd[kWaves][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (unsigned idx = nextBarcode(P.cursor, lane); idx < P.nBarcodes; idx = nextBarcode(P.cursor, lane)) oneBarcode(P, P.order[idx], sArena[w], sOrd[w], lane);
}

extern "C" {

int t1k_barcode_em(t1k_ctx *ctx, uint32_t nBarcodes, const uint64_t *bcAllelePtr, const uint32_t *bcAllele, const uint64_t *bcGroupPtr, const double *groupCount,
                   const uint64_t *groupEntryPtr, const uint32_t *entryLocal, const double *rho, uint32_t nAlleles, double alpha, double tol, int32_t maxIter,
                   double *nOut, int32_t *itersOut, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if (!bcAllelePtr || !bcGroupPtr) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: bad arguments (NULL offsets)");
  if (!(alpha >= 0) || !std::isfinite(alpha) || (alpha > 0 && !rho) || !(tol >= 0) || maxIter < 1)
    return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: bad arguments (alpha >= 0, rho when alpha > 0, tol >= 0, maxIter >= 1)");
  if (nBarcodes == 0) return T1K_OK;
  if (!itersOut || !nOut) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: bad arguments (NULL outputs)");
  // the slice: barcodes [0, nBarcodes) of the offsets given; alleles, groups and entries are rebased to its first ones
  const uint64_t aB = bcAllelePtr[0], gB = bcGroupPtr[0];
  for (uint32_t b = 0; b < nBarcodes; ++b)
    if (bcAllelePtr[b + 1] < bcAllelePtr[b] || bcGroupPtr[b + 1] < bcGroupPtr[b] || bcAllelePtr[b + 1] - bcAllelePtr[b] >= (1ull << 31))
      return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: barcode offsets decrease");
  const uint64_t nL = bcAllelePtr[nBarcodes] - aB, nG = bcGroupPtr[nBarcodes] - gB;
  if ((nL && !bcAllele) || (nG && (!groupCount || !groupEntryPtr))) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: bad arguments (NULL tables)");
  const uint64_t eB = nG ? groupEntryPtr[gB] : 0;
  for (uint64_t g = gB; g < gB + nG; ++g)
    if (groupEntryPtr[g + 1] <= groupEntryPtr[g]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: a group has no entry (or the entry offsets decrease)");
  const uint64_t nE = nG ? groupEntryPtr[gB + nG] - eB : 0;
  if (nE && !entryLocal) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: bad arguments (NULL entries)");
  if (nE >= (1ull << 32) || nG >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_barcode_em: more than 2^32 groups or entries in one call");
  // per barcode: alleles strictly ascending and known, counts positive, every group's entries strictly ascending local indices; the
  // column lists (per local allele, its groups in group order) and the work estimate of the largest-first order
  std::vector<uint64_t> colPtr(nL + 1, 0);
  std::vector<uint32_t> colGroup(nE), order(nBarcodes);
  std::vector<uint64_t> work(nBarcodes);
  std::vector<double> prior(alpha > 0 ? nL : 0);
  for (uint32_t b = 0; b < nBarcodes; ++b) {
    const uint64_t a0 = bcAllelePtr[b] - aB, L = bcAllelePtr[b + 1] - bcAllelePtr[b];
    const uint64_t g0 = bcGroupPtr[b] - gB, G = bcGroupPtr[b + 1] - bcGroupPtr[b];
    for (uint64_t i = 0; i < L; ++i) {
      const uint32_t al = bcAllele[aB + a0 + i];
      if (al >= nAlleles || (i && al <= bcAllele[aB + a0 + i - 1])) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: barcode alleles not ascending, or out of range");
      if (alpha > 0) {
        if (!(rho[al] >= 0) || !std::isfinite(rho[al])) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: rho must be finite and >= 0");
        prior[a0 + i] = alpha * rho[al];
      }
    }
    for (uint64_t g = g0; g < g0 + G; ++g) {
      const double c = groupCount[gB + g];
      if (!(c > 0) || !std::isfinite(c)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: group counts must be finite and > 0");
      for (uint64_t j = groupEntryPtr[gB + g]; j < groupEntryPtr[gB + g + 1]; ++j) {
        const uint32_t l = entryLocal[j];
        if (l >= L || (j > groupEntryPtr[gB + g] && l <= entryLocal[j - 1])) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_barcode_em: group entries not ascending, or outside the barcode's alleles");
        ++colPtr[a0 + l + 1];
      }
    }
    const uint64_t E = G ? groupEntryPtr[gB + g0 + G] - groupEntryPtr[gB + g0] : 0;
    work[b] = E + G + L;
  }
  for (uint64_t i = 0; i < nL; ++i) colPtr[i + 1] += colPtr[i];
  {
    std::vector<uint64_t> fill(colPtr.begin(), colPtr.end() - 1);
    for (uint32_t b = 0; b < nBarcodes; ++b) {
      const uint64_t a0 = bcAllelePtr[b] - aB, g0 = bcGroupPtr[b] - gB, G = bcGroupPtr[b + 1] - bcGroupPtr[b];
      for (uint64_t g = 0; g < G; ++g)
        for (uint64_t j = groupEntryPtr[gB + g0 + g]; j < groupEntryPtr[gB + g0 + g + 1]; ++j) colGroup[fill[a0 + entryLocal[j]]++] = (uint32_t)g;
    }
  }
  // (the column lists of a barcode fill exactly its entries' index range: colPtr is an offset into the entry space, as the kernel reads it)
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return work[x] > work[y]; });
  uint32_t budget = kArenaWords;
  if (const char *s = getenv("T1K_BARCODE_EM_LDS")) budget = (uint32_t)std::min<long long>(kArenaWords, std::max(0LL, atoll(s)));
  // device: one block, 256-byte aligned pieces
  std::vector<uint64_t> bAP(bcAllelePtr, bcAllelePtr + nBarcodes + 1), bGP(bcGroupPtr, bcGroupPtr + nBarcodes + 1), gEP(nG + 1);
  for (auto &x : bAP) x -= aB;
  for (auto &x : bGP) x -= gB;
  if (nG) for (uint64_t g = 0; g <= nG; ++g) gEP[g] = groupEntryPtr[gB + g] - eB;
  T1kCarve piece;
  const size_t oOrder = piece(4ull * nBarcodes), oAP = piece(8 * bAP.size()), oGP = piece(8 * bGP.size()), oEP = piece(8 * gEP.size()), oCP = piece(8 * colPtr.size()),
               oEL = piece(4 * nE), oCG = piece(4 * nE), oCnt = piece(8 * nG), oPri = piece(8 * prior.size()), oTh = piece(8 * nL), oPs = piece(8 * nG),
               oN = piece(8 * nL), oIt = piece(4ull * nBarcodes), oCur = piece(16);
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  T1kCallBlock blk;  // (freed on every return, behind the stream's work)
  int rc;
  if ((rc = blk.alloc(ctx, piece.off))) return rc;
  hipStream_t st = ctx->stream;
  char *D = (char *)blk.buf.p;
  auto put = [&](size_t o, const void *src, size_t bytes) -> hipError_t { return bytes ? hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
  T1K_HIP(ctx, put(oOrder, order.data(), 4ull * nBarcodes));
  T1K_HIP(ctx, put(oAP, bAP.data(), 8 * bAP.size()));
  T1K_HIP(ctx, put(oGP, bGP.data(), 8 * bGP.size()));
  T1K_HIP(ctx, put(oEP, gEP.data(), 8 * gEP.size()));
  T1K_HIP(ctx, put(oCP, colPtr.data(), 8 * colPtr.size()));
  T1K_HIP(ctx, put(oEL, entryLocal + eB, 4 * nE));
  T1K_HIP(ctx, put(oCG, colGroup.data(), 4 * nE));
  T1K_HIP(ctx, put(oCnt, groupCount + gB, 8 * nG));
  T1K_HIP(ctx, put(oPri, prior.data(), 8 * prior.size()));
  T1K_HIP(ctx, hipMemsetAsync(D + oCur, 0, 16, st));
  BcArgs a{};
  a.order = (const uint32_t *)(D + oOrder);
  a.bcAllelePtr = (const uint64_t *)(D + oAP); a.bcGroupPtr = (const uint64_t *)(D + oGP); a.groupEntryPtr = (const uint64_t *)(D + oEP); a.colPtr = (const uint64_t *)(D + oCP);
  a.entryLocal = (const uint32_t *)(D + oEL); a.colGroup = (const uint32_t *)(D + oCG);
  a.groupCount = (const double *)(D + oCnt); a.prior = alpha > 0 ? (const double *)(D + oPri) : nullptr;
  a.alpha = alpha; a.tol = tol; a.maxIter = maxIter; a.nBarcodes = nBarcodes; a.budget = budget;
  a.theta = (double *)(D + oTh); a.psum = (double *)(D + oPs); a.n = (double *)(D + oN); a.iters = (int32_t *)(D + oIt); a.cursor = (unsigned *)(D + oCur);
  // persistent waves: at most four workgroups per CU (the LDS arena's occupancy), fewer when there are fewer barcodes
  const unsigned blocks = t1k_grid(ctx, nBarcodes, kWaves, 4);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_barcode_em, dim3(blocks), dim3(64 * kWaves), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  if (nL) T1K_HIP(ctx, hipMemcpyAsync(nOut + aB, D + oN, 8 * nL, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(itersOut, D + oIt, 4ull * nBarcodes, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  float ms = 0;
  if (kernelMs && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms;
  return T1K_OK;
}

}  // extern "C"
