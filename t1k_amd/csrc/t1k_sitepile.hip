// t1k_amd/csrc/t1k_sitepile.hip -- per-barcode pileup at chosen sites (analyzer --barcodePileup): what t1k_pileup.hip counts,
// split by barcode and restricted to a list of (allele, position) sites.  Sparse in both directions: the result is the list of
// (barcode, site, plane, uniq) cells that received a booking, with their counts, kept on the context from t1k_sitepile_begin to _end.
//
// Sites: a bitmap over the allele-offset space (bit alleleOff[a] + p) and a rank directory (sites in front of each 64-bit word): a lane
// maps its allele position to a site index with one bit test and one population count.
// One kernel, two instantiations, one wave64 per record; the record header, the walk and its verdict are k_pileup's, and so is the host's
// front end of a batch (all in t1k_walk.h):
//   k_sitepile<false>  check and count: the walk's checks (an op outside 0 .. 3, a walk that leaves its allele or the text) and per record
//                      hits x bookings, hits = its columns that book at a site.  Only when the flag word comes back clear does the host
//                      take the exclusive sum of the counts and launch
//   k_sitepile<true>   emit: one 64-bit key per (hit, booking) at its precomputed slot -- no atomics.  Inside a 64-column step the keys of
//                      booking b are consecutive over the lanes with a hit (slot + b * hits + hits below the lane): coalesced stores.
// Key = ((barcode * nSites + site) * 7 + plane) * 2 + (1 - uniq).  A uniq booking is emitted ONCE, under uniq = 1 (the even key); it
// counts in the plain counter as well as in the _uniq one where the runs are read: the reader of t1k_sitepile_get adds the even run of a
// cell to its plain counter (plain = even + odd, _uniq = even).  So no booking is ever stored twice.
// Fold: the table is (key, count) pairs followed by the pending keys (count 1).  t1k_sort_pairs over the bits of the largest possible
// key, t1k_run_table (t1k_sort.hip) numbers the runs, an inclusive scan of the counts (uint32, exact modulo 2^32) gives every run's sum as
// the difference of the scan at its last element and at the previous run's last element: a run's sum is at most (2^31 - 1) + the pending
// keys < 2^32, so the difference is exact, and no lane ever walks a run.  A sum beyond 2^31 - 1 refuses the fold (T1K_ERR_CAPACITY) and
// leaves the table as it was.  The table is folded whenever the pending keys reach a bound (2^28, env T1K_SITEPILE_PENDING) and at _get.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_walk.h"

enum { SITEPILE_BASE_PLANES = 7 };

struct SitepileArgs {
  PileupBatch in;
  const unsigned long long *bits;       // [total / 64 + 1] bit alleleOff[a] + p = (a, p) is a site
  const uint32_t *rank;                 // [total / 64 + 1] sites in front of the word
  unsigned long long nSites;
  const unsigned long long *bookPtr;    // [n + 1] into book
  const uint32_t *book;                 // barcode << 1 | uniq
  unsigned long long *count;            // [n + 1]: <false> writes hits x bookings, <true> reads their exclusive sums
  unsigned long long *keys;             // <true>: the pending keys of this call
  uint32_t *vals;                       //         and their counts (1 each)
};

template <bool EMIT>
__global__ __launch_bounds__(256) void k_sitepile(SitepileArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) {
    const unsigned long long bookAt = pileupUniform64(P.bookPtr[r]);
    const uint32_t nBook = (uint32_t)(pileupUniform64(P.bookPtr[r + 1]) - bookAt);
    if (EMIT && nBook == 0) continue;
    const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);  // (its weights are not read here)
    const unsigned long long base = R.base, len = R.len, readAt = R.readAt;
    unsigned long long slot = EMIT ? pileupUniform64(P.count[r]) : 0ull;  // wave-uniform: the next free key of this record
    unsigned long long hits = 0;
    const PileupWalkEnd end = pileupWalk<!EMIT, true>(P.in.ops, R.opsAt, R.nOps, R.seqStart, len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long myP) {
      bool hit = false;
      uint32_t site = 0;
      if (active && pos < len) {  // (pos >= len: only in the check pass, on a walk it is about to refuse)
        const unsigned long long g = base + pos, w = P.bits[g >> 6];
        hit = (w >> (g & 63u)) & 1ull;
        site = P.rank[g >> 6] + (uint32_t)__popcll(w & ((1ull << (g & 63u)) - 1ull));
      }
      const uint64_t mH = __ballot(hit ? 1 : 0);
      const uint32_t h = (uint32_t)__popcll(mH);
      if (!EMIT) { hits += h; return; }
      if (h == 0) return;  // wave-uniform
      unsigned long long cell = 0;
      if (hit) cell = (unsigned long long)site * SITEPILE_BASE_PLANES + (op == 2 ? (uint32_t)PILEUP_INS : op == 3 ? (uint32_t)PILEUP_DEL : pileupBasePlane(P.in.text[readAt + myP]));
      const unsigned long long mine = slot + pileupBelow(mH);
      for (uint32_t b = 0; b < nBook; ++b) {
        const uint32_t e = pileupUniform(P.book[bookAt + b]);
        if (hit) {
          const unsigned long long at = mine + (unsigned long long)b * h;
          P.keys[at] = (((unsigned long long)(e >> 1) * P.nSites * SITEPILE_BASE_PLANES + cell) << 1) | (1u - (e & 1u));
          P.vals[at] = 1u;
        }
      }
      slot += (unsigned long long)h * nBook;
    });
    if (!EMIT) {
      const uint32_t bad = pileupWalkVerdict(end, len, readAt, P.in.textBytes);
      if (lane == 0) {
        if (bad) atomicOr(P.in.flag, bad);
        P.count[r] = hits * nBook;
      }
    }
  }
}

// count of run r = the inclusive sum of the sorted counts at its last element minus that at the previous run's, modulo 2^32 (exact: see
// the header); beyond 2^31 - 1 sets *over
__global__ __launch_bounds__(256) void k_sitepile_counts(const uint32_t *incl, const uint32_t *runStart, uint32_t nRuns, uint32_t *runCount, uint32_t *over) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nRuns; r += gridDim.x * 256u) {
    const uint32_t c = incl[runStart[r + 1] - 1] - (r ? incl[runStart[r] - 1] : 0u);
    runCount[r] = c;
    if (c > 0x7FFFFFFFu) atomicOr(over, 1u);
  }
}

// room for `want` (key, count) pairs in the table; what it holds is kept
static int sitepileReserve(t1k_ctx *ctx, uint64_t want) {
  if (want <= ctx->spCap) return T1K_OK;
  const uint64_t cap = std::max<uint64_t>(want + want / 4, 1024);
  void *k = nullptr, *v = nullptr;
  if (t1k_dev_malloc(&k, cap * 8) != hipSuccess || t1k_dev_malloc(&v, cap * 4) != hipSuccess) {
    if (k) (void)t1k_dev_free(k);
    return t1k_fail(ctx, T1K_ERR_DEVICE, "t1k_sitepile: out of device memory for " + std::to_string(cap) + " keys");
  }
  const uint64_t n = ctx->spRuns + ctx->spPending;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(k, ctx->bSpKeys.p, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v, ctx->bSpVals.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)t1k_dev_free(k); (void)t1k_dev_free(v); return t1k_fail(ctx, T1K_ERR_DEVICE, std::string("t1k_sitepile: ") + hipGetErrorString(e)); }
  if (ctx->bSpKeys.p) (void)t1k_dev_free(ctx->bSpKeys.p);
  if (ctx->bSpVals.p) (void)t1k_dev_free(ctx->bSpVals.p);
  ctx->bSpKeys.p = k; ctx->bSpKeys.bytes = cap * 8;
  ctx->bSpVals.p = v; ctx->bSpVals.bytes = cap * 4;
  ctx->spCap = cap;
  return T1K_OK;
}

// (key, count) pairs [0, spRuns) + pending keys behind them -> (key, count) pairs, ascending.  On an error the table is as before.
static int sitepileFold(t1k_ctx *ctx) {
  const uint64_t n64 = ctx->spRuns + ctx->spPending;
  if (ctx->spPending == 0 || n64 == 0) return T1K_OK;
  const uint32_t n = (uint32_t)n64;  // (< 2^31: t1k_sitepile_add)
  hipStream_t st = ctx->stream;
  T1kCarve piece;
  const size_t oKey = piece(8ull * n), oVal = piece(4ull * n), oFlag = piece(4ull * (n + 1ull)), oScan = piece(4ull * (n + 1ull)), oIncl = piece(4ull * n),
               oRunKey = piece(8ull * n), oRunStart = piece(4ull * (n + 1ull)), oRunCount = piece(4ull * n), oOver = piece(8);
  int rc;
  if ((rc = t1k_ensure(ctx, ctx->bSpWork, piece.off))) return rc;
  char *D = (char *)ctx->bSpWork.p;
  unsigned long long *keyB = (unsigned long long *)(D + oKey), *runKey = (unsigned long long *)(D + oRunKey);
  uint32_t *valB = (uint32_t *)(D + oVal), *flag = (uint32_t *)(D + oFlag), *scan = (uint32_t *)(D + oScan), *incl = (uint32_t *)(D + oIncl), *runStart = (uint32_t *)(D + oRunStart),
           *runCount = (uint32_t *)(D + oRunCount), *over = (uint32_t *)(D + oOver);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  T1K_HIP(ctx, hipMemsetAsync(over, 0, 8, st));
  if ((rc = t1k_sort_pairs(ctx, (const unsigned long long *)ctx->bSpKeys.p, keyB, (const uint32_t *)ctx->bSpVals.p, valB, n, ctx->spEndBit))) return rc;
  uint32_t nRuns = 0;
  if ((rc = t1k_run_table(ctx, keyB, n, nullptr, flag, scan, runStart, runKey, &nRuns))) return rc;
  if (nRuns == 0 || nRuns > n) return t1k_fail(ctx, T1K_ERR_INTERNAL, "t1k_sitepile: the runs of the fold do not add up");
  if ((rc = t1k_inclusive_sum(ctx, valB, incl, n))) return rc;
  hipLaunchKernelGGL(k_sitepile_counts, dim3(t1k_grid(ctx, nRuns, 256)), dim3(256), 0, st, (const uint32_t *)incl, (const uint32_t *)runStart, nRuns, runCount, over);
  T1K_HIP(ctx, hipGetLastError());
  uint32_t hOver = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&hOver, over, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (hOver) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile: a counter would pass 2^31 - 1");
  T1K_HIP(ctx, hipMemcpyAsync(ctx->bSpKeys.p, runKey, 8ull * nRuns, hipMemcpyDeviceToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(ctx->bSpVals.p, runCount, 4ull * nRuns, hipMemcpyDeviceToDevice, st));
  T1K_HIP(ctx, hipEventRecord(ctx->ev[3], st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  ctx->spRuns = nRuns;
  ctx->spPending = 0;
  ++ctx->spFolds;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->spFoldMs += ms;
  return T1K_OK;
}

extern "C" {

int t1k_sitepile_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos, uint64_t nBarcodes) {
  if (!ctx) return T1K_ERR_ARG;
  if (ctx->spOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_sitepile_begin: a table is open already (t1k_sitepile_end first)");
  if (nSites && (!siteAllele || !sitePos)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_begin: bad arguments (NULL arrays, or alleleOff not starting at 0)");
  int rc;
  if ((rc = pileupCheckOffsets(ctx, "t1k_sitepile_begin", "NULL arrays, or alleleOff not starting at 0", nAlleles, alleleOff))) return rc;
  const uint64_t total = alleleOff[nAlleles];
  if (nSites > total) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_begin: more sites than allele positions (the sites are not strictly ascending)");
  // a booking names its barcode in 31 bits; the largest key, nBarcodes * nSites * 14 - 1, must leave the top bit of the 64 alone
  if (nBarcodes > (1ull << 31)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_begin: more than 2^31 barcodes");
  const unsigned __int128 space = (unsigned __int128)nBarcodes * nSites * (2 * SITEPILE_BASE_PLANES);
  if (space >= ((unsigned __int128)1 << 63)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_begin: nBarcodes * nSites * 14 does not fit the key (2^63)");
  const uint64_t words = total / 64 + 1;
  std::vector<uint64_t> bits(words, 0);
  std::vector<uint32_t> rank(words, 0);
  for (uint64_t s = 0; s < nSites; ++s) {
    const uint32_t a = siteAllele[s], p = sitePos[s];
    if (a >= nAlleles || p >= alleleOff[a + 1] - alleleOff[a]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_begin: site " + std::to_string(s) + " lies outside the alleles");
    if (s && (siteAllele[s - 1] > a || (siteAllele[s - 1] == a && sitePos[s - 1] >= p)))
      return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_begin: the sites are not strictly ascending by (allele, pos) at site " + std::to_string(s));
    const uint64_t g = alleleOff[a] + p;
    bits[g >> 6] |= 1ull << (g & 63);
  }
  for (uint64_t w = 1; w < words; ++w) rank[w] = rank[w - 1] + (uint32_t)__builtin_popcountll(bits[w - 1]);
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  // [bits | rank | alleleOff]
  T1kCarve piece;
  const size_t oBits = piece(8 * words), oRank = piece(4 * words), oOff = piece(8ull * (nAlleles + 1));
  if ((rc = t1k_ensure(ctx, ctx->bSpSites, piece.off))) return rc;
  char *D = (char *)ctx->bSpSites.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oBits, bits.data(), 8 * words, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(D + oRank, rank.data(), 4 * words, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(D + oOff, alleleOff, 8ull * (nAlleles + 1), hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->spOff.assign(alleleOff, alleleOff + nAlleles + 1);
  ctx->spSiteAt[0] = oBits; ctx->spSiteAt[1] = oRank; ctx->spSiteAt[2] = oOff;
  ctx->spSites = nSites;
  ctx->spBarcodes = nBarcodes;
  ctx->spEndBit = t1k_bits(space ? (unsigned long long)(space - 1) : 0ull);
  ctx->spRuns = ctx->spPending = ctx->spEmitted = ctx->spFolds = 0;
  ctx->spFoldMs = 0;
  ctx->spBound = 1ull << 28;
  if (const char *e = getenv("T1K_SITEPILE_PENDING")) ctx->spBound = std::min<uint64_t>(1ull << 30, (uint64_t)std::max(1ll, atoll(e)));
  ctx->spOpen = true;
  return T1K_OK;
}

int t1k_sitepile_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint64_t *bookPtr, const uint32_t *book, const char *text, uint64_t textBytes, const int8_t *ops,
                     uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if (!ctx->spOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_sitepile_add: no table is open (t1k_sitepile_begin first)");
  if (n == 0) return T1K_OK;
  if (!aln || !bookPtr || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: bad arguments (NULL arrays)");
  // what the host can tell from the records and the booking lists alone; the strings themselves are walked on the device before anything is emitted
  for (uint32_t i = 0; i < n; ++i) {
    if (bookPtr[i + 1] < bookPtr[i]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: bookPtr decreases at record " + std::to_string(i));
    if (bookPtr[i + 1] - bookPtr[i] >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_add: record " + std::to_string(i) + " has 2^32 bookings or more");
    const std::string fault = pileupRecordFault(aln[i], i, ctx->spOff, textBytes, opsBytes);
    if (!fault.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: " + fault);
  }
  const uint64_t book0 = bookPtr[0], nBook = bookPtr[n] - book0;
  if (nBook && !book) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: bad arguments (NULL book)");
  for (uint64_t j = 0; j < nBook; ++j)
    if ((book[book0 + j] >> 1) >= ctx->spBarcodes) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: booking " + std::to_string(book0 + j) + " names an unknown barcode");
  std::vector<uint64_t> bp(n + 1);
  for (uint32_t i = 0; i <= n; ++i) bp[i] = bookPtr[i] - book0;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const char *S = (const char *)ctx->bSpSites.p;
  SitepileArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, (const unsigned long long *)(S + ctx->spSiteAt[2]), nullptr};
  size_t oBp = 0, oBook = 0, oCount = 0;
  int rc;
  if ((rc = pileupStage(ctx, ctx->bSpIn, opsBytes, [&](T1kCarve &piece) { oBp = piece(8ull * (n + 1ull)); oBook = piece(4 * nBook); oCount = piece(8ull * (n + 1ull)); }, a.in))) return rc;
  char *D = (char *)ctx->bSpIn.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oBp, bp.data(), 8ull * (n + 1ull), hipMemcpyHostToDevice, st));
  if (nBook) T1K_HIP(ctx, hipMemcpyAsync(D + oBook, book + book0, 4 * nBook, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oCount, 0, 8ull * (n + 1ull), st));
  a.bits = (const unsigned long long *)(S + ctx->spSiteAt[0]); a.rank = (const uint32_t *)(S + ctx->spSiteAt[1]);
  a.nSites = ctx->spSites;
  a.bookPtr = (const unsigned long long *)(D + oBp); a.book = (const uint32_t *)(D + oBook);
  a.count = (unsigned long long *)(D + oCount);
  const unsigned grid = t1k_grid(ctx, n, 4);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_sitepile<false>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_exclusive_sum_u64(ctx, a.count, a.count, (uint64_t)n + 1))) return rc;  // (in place: every tile is read before it is written)
  uint32_t flag = 0;
  unsigned long long emit = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.in.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&emit, a.count + n, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal("t1k_sitepile_add", "nothing emitted", flag));
  if (emit == 0) {
    T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    T1K_HIP(ctx, hipStreamSynchronize(st));
    float ms0 = 0;
    if (kernelMs && hipEventElapsedTime(&ms0, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms0;
    return T1K_OK;
  }
  // the sort takes 32-bit item counts, and the run sums of a fold stay below 2^32 with fewer than 2^31 pending keys
  if (ctx->spRuns + ctx->spPending + emit >= (1ull << 31))
    return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_add: the table and this call's keys exceed 2^31 entries (lower T1K_SITEPILE_PENDING, or add fewer records per call)");
  const uint64_t runs0 = ctx->spRuns, pending0 = ctx->spPending;
  if ((rc = sitepileReserve(ctx, runs0 + pending0 + emit))) return rc;
  a.keys = (unsigned long long *)ctx->bSpKeys.p + runs0 + pending0;
  a.vals = (uint32_t *)ctx->bSpVals.p + runs0 + pending0;
  hipLaunchKernelGGL(k_sitepile<true>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  T1K_HIP(ctx, hipStreamSynchronize(st));  // text / ops / book are the caller's again, the staging block the next call's
  float ms = 0;
  if (kernelMs && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms;
  ctx->spPending += emit;
  if (ctx->spPending >= ctx->spBound && (rc = sitepileFold(ctx)) != T1K_OK) {
    ctx->spPending = pending0;  // the fold left the table alone: this call's keys are dropped again
    return rc;
  }
  ctx->spEmitted += emit;
  return T1K_OK;
}

int t1k_sitepile_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) {
  if (!ctx) return T1K_ERR_ARG;
  if (nRuns) *nRuns = 0;
  if (!ctx->spOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_sitepile_get: no table is open");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = sitepileFold(ctx)) != T1K_OK) return rc;
  if (nRuns) *nRuns = ctx->spRuns;
  if (!keys || !counts || !ctx->spRuns) return T1K_OK;  // the size query
  if (cap < ctx->spRuns) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_get: the buffers are too small");
  T1K_HIP(ctx, hipMemcpyAsync(keys, ctx->bSpKeys.p, 8 * ctx->spRuns, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync(counts, ctx->bSpVals.p, 4 * ctx->spRuns, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return T1K_OK;
}

int t1k_sitepile_stats(t1k_ctx *ctx, uint64_t *keysEmitted, uint64_t *folds, double *foldMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (!ctx->spOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_sitepile_stats: no table is open");
  if (keysEmitted) *keysEmitted = ctx->spEmitted;
  if (folds) *folds = ctx->spFolds;
  if (foldMs) *foldMs = ctx->spFoldMs;
  return T1K_OK;
}

int t1k_sitepile_end(t1k_ctx *ctx) {
  if (!ctx) return T1K_ERR_ARG;
  if (!ctx->spOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_sitepile_end: no table is open");
  ctx->spOpen = false;
  ctx->spOff.clear();
  ctx->spRuns = ctx->spPending = ctx->spCap = 0;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (T1kDevBuf *b : {&ctx->bSpKeys, &ctx->bSpVals, &ctx->bSpWork, &ctx->bSpIn, &ctx->bSpSites})
    if (b->p) { (void)t1k_dev_free(b->p); b->p = nullptr; b->bytes = 0; }
  return T1K_OK;
}

}  // extern "C"
