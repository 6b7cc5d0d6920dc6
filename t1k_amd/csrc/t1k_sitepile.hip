// t1k_amd/csrc/t1k_sitepile.hip -- per-barcode pileup at chosen sites (analyzer --barcodePileup): what t1k_pileup.hip counts,
// split by barcode and restricted to a list of (allele, position) sites.  Sparse in both directions: the result is the list of
// (barcode, site, plane, uniq) cells that received a booking, with their counts, kept on the context from t1k_sitepile_begin to _end.
//
// Sites: a T1kSiteMap (t1k_table.h): a lane maps its allele position to a site index with one bit test and one population count.
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
// The table and its fold are a T1kCountTable (t1k_table.h): (key, count) pairs followed by the pending keys (count 1), folded whenever the
// pending keys reach a bound (2^28, env T1K_SITEPILE_PENDING) and at _get.
// Shared with the other sparse stages, and not written out here: the session (ctx->sp, a T1kStage: state checks, _get, _stats, _end, the
// site arguments of _begin) and the check / sum / emit sequence of _add (t1k_stage_two_pass) in t1k_table.h; the checks of records and
// booking lists (pileupBookLists) and the staging (pileupStage) in t1k_walk.h.  Here: the kernel, the key's bounds, the barcode checks.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_table.h"
#include "t1k_walk.h"

enum { SITEPILE_BASE_PLANES = 7 };

struct SitepileArgs {
  PileupBatch in;
  T1kSiteView sites;
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
      if (active && pos < len) hit = t1kSiteAt(P.sites, base + pos, site);  // (pos >= len: only in the check pass, on a walk it is about to refuse)
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

extern "C" {

int t1k_sitepile_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos, uint64_t nBarcodes) {
  if (!ctx) return T1K_ERR_ARG;
  T1kStage &s = ctx->sp;
  int rc;
  if ((rc = t1k_stage_closed(ctx, s))) return rc;
  if ((rc = t1k_stage_site_args(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos))) return rc;
  // a booking names its barcode in 31 bits; the largest key, nBarcodes * nSites * 14 - 1, must leave the top bit of the 64 alone
  if (nBarcodes > (1ull << 31)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_begin: more than 2^31 barcodes");
  const unsigned __int128 space = (unsigned __int128)nBarcodes * nSites * (2 * SITEPILE_BASE_PLANES);
  if (space >= ((unsigned __int128)1 << 63)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_sitepile_begin: nBarcodes * nSites * 14 does not fit the key (2^63)");
  ctx->spBarcodes = nBarcodes;
  return t1k_stage_open_sites(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos, space ? (unsigned long long)(space - 1) : 0ull);
}

int t1k_sitepile_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint64_t *bookPtr, const uint32_t *book, const char *text, uint64_t textBytes, const int8_t *ops,
                     uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  T1kStage &s = ctx->sp;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_add", "_begin"))) return rc;
  if (n == 0) return T1K_OK;
  if (!aln || !bookPtr || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: bad arguments (NULL arrays)");
  // what the host can tell from the records and the booking lists alone; the strings themselves are walked on the device before anything is emitted
  std::vector<uint64_t> bp;
  if ((rc = pileupBookLists(ctx, "t1k_sitepile_add", aln, n, s.off, textBytes, opsBytes, bookPtr, 32, book, "book", [](uint32_t) { return std::string(); }, bp))) return rc;
  const uint64_t book0 = bookPtr[0], nBook = bp[n];
  for (uint64_t j = 0; j < nBook; ++j)
    if ((book[book0 + j] >> 1) >= ctx->spBarcodes) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_sitepile_add: booking " + std::to_string(book0 + j) + " names an unknown barcode");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SitepileArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, t1k_sites_offsets(s.map), nullptr};
  size_t oBp = 0, oBook = 0, oCount = 0;
  if ((rc = pileupStage(ctx, s.in, opsBytes, [&](T1kCarve &piece) { oBp = piece(8ull * (n + 1ull)); oBook = piece(4 * nBook); oCount = piece(8ull * (n + 1ull)); }, a.in))) return rc;
  char *D = (char *)s.in.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oBp, bp.data(), 8ull * (n + 1ull), hipMemcpyHostToDevice, st));
  if (nBook) T1K_HIP(ctx, hipMemcpyAsync(D + oBook, book + book0, 4 * nBook, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oCount, 0, 8ull * (n + 1ull), st));
  a.sites = t1k_sites_view(s.map);
  a.nSites = s.map.nSites;
  a.bookPtr = (const unsigned long long *)(D + oBp); a.book = (const uint32_t *)(D + oBook);
  a.count = (unsigned long long *)(D + oCount);
  const unsigned grid = t1k_grid(ctx, n, 4);
  return t1k_stage_two_pass(ctx, s, n, a.in.flag, a.count, kernelMs, [&] { hipLaunchKernelGGL(k_sitepile<false>, dim3(grid), dim3(256), 0, st, a); },
                            [&](unsigned long long *keys, uint32_t *vals) { a.keys = keys; a.vals = vals; hipLaunchKernelGGL(k_sitepile<true>, dim3(grid), dim3(256), 0, st, a); });
}

int t1k_sitepile_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) { return t1k_stage_get(ctx, &t1k_ctx::sp, keys, counts, cap, nRuns); }

int t1k_sitepile_stats(t1k_ctx *ctx, uint64_t *keysEmitted, uint64_t *folds, double *foldMs) { return t1k_stage_stats(ctx, &t1k_ctx::sp, keysEmitted, folds, foldMs); }

int t1k_sitepile_end(t1k_ctx *ctx) { return t1k_stage_end(ctx, &t1k_ctx::sp); }

}  // extern "C"
