// t1k_amd/csrc/t1k_table.hip -- the host side of t1k_table.h: the site map's builder, the sparse count table's reserve / fold / read and
// the session around them (T1kStage), shared by t1k_sitepile.hip, t1k_support.hip, t1k_phase.hip and t1k_indel.hip.
#include <algorithm>
#include <cstdlib>
#include <vector>
#include "t1k_table.h"

// count of run r = the inclusive sum of the sorted counts at its last element minus that at the previous run's, modulo 2^32 (exact: see
// t1k_table.h); beyond 2^31 - 1 sets *over
__global__ __launch_bounds__(256) void k_table_counts(const uint32_t *incl, const uint32_t *runStart, uint32_t nRuns, uint32_t *runCount, uint32_t *over) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nRuns; r += gridDim.x * 256u) {
    const uint32_t c = incl[runStart[r + 1] - 1] - (r ? incl[runStart[r] - 1] : 0u);
    runCount[r] = c;
    if (c > 0x7FFFFFFFu) atomicOr(over, 1u);
  }
}

// (what t1k_stage_open_sites says of the sites; who: the _begin's name)
static int sitesBuild(t1k_ctx *ctx, const char *who, T1kSiteMap &m, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos) {
  const std::string W(who);
  const uint64_t words = alleleOff[nAlleles] / 64 + 1;
  std::vector<uint64_t> bits(words, 0);
  std::vector<uint32_t> rank(words, 0);
  for (uint64_t s = 0; s < nSites; ++s) {
    const uint32_t a = siteAllele[s], p = sitePos[s];
    if (a >= nAlleles || p >= alleleOff[a + 1] - alleleOff[a]) return t1k_fail(ctx, T1K_ERR_ARG, W + ": site " + std::to_string(s) + " lies outside the alleles");
    if (s && (siteAllele[s - 1] > a || (siteAllele[s - 1] == a && sitePos[s - 1] >= p)))
      return t1k_fail(ctx, T1K_ERR_ARG, W + ": the sites are not strictly ascending by (allele, pos) at site " + std::to_string(s));
    const uint64_t g = alleleOff[a] + p;
    bits[g >> 6] |= 1ull << (g & 63);
  }
  for (uint64_t w = 1; w < words; ++w) rank[w] = rank[w - 1] + (uint32_t)__builtin_popcountll(bits[w - 1]);
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  // [bits | rank | alleleOff]
  T1kCarve piece;
  const size_t oBits = piece(8 * words), oRank = piece(4 * words), oOff = piece(8ull * (nAlleles + 1));
  int rc;
  if ((rc = t1k_ensure(ctx, m.buf, piece.off))) return rc;
  char *D = (char *)m.buf.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oBits, bits.data(), 8 * words, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(D + oRank, rank.data(), 4 * words, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(D + oOff, alleleOff, 8ull * (nAlleles + 1), hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  m.at[0] = oBits; m.at[1] = oRank; m.at[2] = oOff;
  m.nSites = nSites;
  return T1K_OK;
}

static void tableFree(T1kDevBuf &b) {
  if (b.p) { (void)t1k_dev_free(b.p); b.p = nullptr; b.bytes = 0; }
}

// an empty table whose keys are all <= largestKey; boundEnv: the environment variable that overrides the pending bound of 2^28
static void tableOpen(T1kCountTable &t, unsigned long long largestKey, const char *boundEnv) {
  t.endBit = t1k_bits(largestKey);
  t.runs = t.pending = t.emitted = t.folds = 0;
  t.foldMs = 0;
  t.bound = 1ull << 28;
  if (const char *e = getenv(boundEnv)) t.bound = std::min<uint64_t>(1ull << 30, (uint64_t)std::max(1ll, atoll(e)));
}

// room for `want` (key, count) pairs in the table; what it holds is kept
static int tableReserve(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t want) {
  if (want <= t.cap) return T1K_OK;
  const uint64_t cap = std::max<uint64_t>(want + want / 4, 1024);
  void *k = nullptr, *v = nullptr;
  if (t1k_dev_malloc(&k, cap * 8) != hipSuccess || t1k_dev_malloc(&v, cap * 4) != hipSuccess) {
    if (k) (void)t1k_dev_free(k);
    return t1k_fail(ctx, T1K_ERR_DEVICE, std::string(who) + ": out of device memory for " + std::to_string(cap) + " keys");
  }
  const uint64_t n = t.runs + t.pending;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(k, t.keys.p, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v, t.vals.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)t1k_dev_free(k); (void)t1k_dev_free(v); return t1k_fail(ctx, T1K_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e)); }
  tableFree(t.keys);
  tableFree(t.vals);
  t.keys.p = k; t.keys.bytes = cap * 8;
  t.vals.p = v; t.vals.bytes = cap * 4;
  t.cap = cap;
  return T1K_OK;
}

// (key, count) pairs [0, runs) + pending keys behind them -> (key, count) pairs, ascending.  On an error the table is as before.
static int tableFold(t1k_ctx *ctx, const char *who, T1kCountTable &t) {
  const uint64_t n64 = t.runs + t.pending;
  if (t.pending == 0 || n64 == 0) return T1K_OK;
  const uint32_t n = (uint32_t)n64;  // (< 2^31: t1k_table_room)
  hipStream_t st = ctx->stream;
  T1kCarve piece;
  const size_t oKey = piece(8ull * n), oVal = piece(4ull * n), oFlag = piece(4ull * (n + 1ull)), oScan = piece(4ull * (n + 1ull)), oIncl = piece(4ull * n),
               oRunKey = piece(8ull * n), oRunStart = piece(4ull * (n + 1ull)), oRunCount = piece(4ull * n), oOver = piece(8);
  int rc;
  if ((rc = t1k_ensure(ctx, t.work, piece.off))) return rc;
  char *D = (char *)t.work.p;
  unsigned long long *keyB = (unsigned long long *)(D + oKey), *runKey = (unsigned long long *)(D + oRunKey);
  uint32_t *valB = (uint32_t *)(D + oVal), *flag = (uint32_t *)(D + oFlag), *scan = (uint32_t *)(D + oScan), *incl = (uint32_t *)(D + oIncl), *runStart = (uint32_t *)(D + oRunStart),
           *runCount = (uint32_t *)(D + oRunCount), *over = (uint32_t *)(D + oOver);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  T1K_HIP(ctx, hipMemsetAsync(over, 0, 8, st));
  if ((rc = t1k_sort_pairs(ctx, (const unsigned long long *)t.keys.p, keyB, (const uint32_t *)t.vals.p, valB, n, t.endBit))) return rc;
  uint32_t nRuns = 0;
  if ((rc = t1k_run_table(ctx, keyB, n, nullptr, flag, scan, runStart, runKey, &nRuns))) return rc;
  if (nRuns == 0 || nRuns > n) return t1k_fail(ctx, T1K_ERR_INTERNAL, std::string(who) + ": the runs of the fold do not add up");
  if ((rc = t1k_inclusive_sum(ctx, valB, incl, n))) return rc;
  hipLaunchKernelGGL(k_table_counts, dim3(t1k_grid(ctx, nRuns, 256)), dim3(256), 0, st, (const uint32_t *)incl, (const uint32_t *)runStart, nRuns, runCount, over);
  T1K_HIP(ctx, hipGetLastError());
  uint32_t hOver = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&hOver, over, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (hOver) return t1k_fail(ctx, T1K_ERR_CAPACITY, std::string(who) + ": a counter would pass 2^31 - 1");
  T1K_HIP(ctx, hipMemcpyAsync(t.keys.p, runKey, 8ull * nRuns, hipMemcpyDeviceToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(t.vals.p, runCount, 4ull * nRuns, hipMemcpyDeviceToDevice, st));
  T1K_HIP(ctx, hipEventRecord(ctx->ev[3], st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  t.runs = nRuns;
  t.pending = 0;
  ++t.folds;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) t.foldMs += ms;
  return T1K_OK;
}

int t1k_table_room(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit, const char *hint, unsigned long long **keys, uint32_t **vals) {
  // the sort takes 32-bit item counts, and the run sums of a fold stay below 2^32 with fewer than 2^31 pending keys
  if (t.runs + t.pending + emit >= (1ull << 31))
    return t1k_fail(ctx, T1K_ERR_CAPACITY, std::string(who) + "_add: the table and this call's keys exceed 2^31 entries (" + hint + ")");
  int rc;
  if ((rc = tableReserve(ctx, who, t, t.runs + t.pending + emit))) return rc;
  *keys = (unsigned long long *)t.keys.p + t.runs + t.pending;
  *vals = (uint32_t *)t.vals.p + t.runs + t.pending;
  return T1K_OK;
}

int t1k_table_commit(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit) {
  const uint64_t pending0 = t.pending;
  t.pending += emit;
  int rc;
  if (t.pending >= t.bound && (rc = tableFold(ctx, who, t)) != T1K_OK) {
    t.pending = pending0;  // the fold left the table alone: this call's keys are dropped again
    return rc;
  }
  t.emitted += emit;
  return T1K_OK;
}

// ---- the session ----
static int stageState(t1k_ctx *ctx, const T1kStage &s, const char *fn, const std::string &what) { return t1k_fail(ctx, T1K_ERR_STATE, std::string(s.who) + fn + ": " + what); }

int t1k_stage_closed(t1k_ctx *ctx, const T1kStage &s) {
  return s.open ? stageState(ctx, s, "_begin", std::string("a table is open already (") + s.who + "_end first)") : T1K_OK;
}

int t1k_stage_opened(t1k_ctx *ctx, const T1kStage &s, const char *fn, const char *hint) {
  if (s.open) return T1K_OK;
  return stageState(ctx, s, fn, hint ? std::string("no table is open (") + s.who + hint + " first)" : std::string("no table is open"));
}

int t1k_stage_site_args(t1k_ctx *ctx, const T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos) {
  const std::string begin = std::string(s.who) + "_begin";
  if (nSites && (!siteAllele || !sitePos)) return t1k_fail(ctx, T1K_ERR_ARG, begin + ": bad arguments (NULL arrays, or alleleOff not starting at 0)");
  int rc;
  if ((rc = pileupCheckOffsets(ctx, begin.c_str(), "NULL arrays, or alleleOff not starting at 0", nAlleles, alleleOff))) return rc;
  if (nSites > alleleOff[nAlleles]) return t1k_fail(ctx, T1K_ERR_ARG, begin + ": more sites than allele positions (the sites are not strictly ascending)");
  return T1K_OK;
}

void t1k_stage_open(T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, unsigned long long largestKey) {
  s.off.assign(alleleOff, alleleOff + nAlleles + 1);
  tableOpen(s.tab, largestKey, s.boundEnv);
  s.open = true;
}

int t1k_stage_open_sites(t1k_ctx *ctx, T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos,
                         unsigned long long largestKey) {
  int rc;
  if ((rc = sitesBuild(ctx, (std::string(s.who) + "_begin").c_str(), s.map, nAlleles, alleleOff, nSites, siteAllele, sitePos))) return rc;
  t1k_stage_open(s, nAlleles, alleleOff, largestKey);
  return T1K_OK;
}

int t1k_stage_get(t1k_ctx *ctx, T1kStage t1k_ctx::*which, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) {
  if (!ctx) return T1K_ERR_ARG;
  if (nRuns) *nRuns = 0;
  T1kStage &s = ctx->*which;
  T1kCountTable &t = s.tab;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_get"))) return rc;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = tableFold(ctx, s.who, t)) != T1K_OK) return rc;
  if (nRuns) *nRuns = t.runs;
  if (!keys || !counts || !t.runs) return T1K_OK;  // the size query
  if (cap < t.runs) return t1k_fail(ctx, T1K_ERR_ARG, std::string(s.who) + "_get: the buffers are too small");
  T1K_HIP(ctx, hipMemcpyAsync(keys, t.keys.p, 8 * t.runs, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(counts, t.vals.p, 4 * t.runs, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return T1K_OK;
}

int t1k_stage_stats(t1k_ctx *ctx, T1kStage t1k_ctx::*which, uint64_t *keysEmitted, uint64_t *folds, double *foldMs) {
  if (!ctx) return T1K_ERR_ARG;
  const T1kStage &s = ctx->*which;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_stats"))) return rc;
  if (keysEmitted) *keysEmitted = s.tab.emitted;
  if (folds) *folds = s.tab.folds;
  if (foldMs) *foldMs = s.tab.foldMs;
  return T1K_OK;
}

int t1k_stage_end(t1k_ctx *ctx, T1kStage t1k_ctx::*which) {
  if (!ctx) return T1K_ERR_ARG;
  T1kStage &s = ctx->*which;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_end"))) return rc;
  s.open = false;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  s.off.clear();
  s.map.nSites = 0;
  s.tab.runs = s.tab.pending = s.tab.cap = 0;
  t1k_stage_blocks(s, [](const std::string &, T1kDevBuf &b) { tableFree(b); });
  return T1K_OK;
}

int t1k_stage_done(t1k_ctx *ctx, double *kernelMs) {
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0;
  if (kernelMs && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms;
  return T1K_OK;
}
