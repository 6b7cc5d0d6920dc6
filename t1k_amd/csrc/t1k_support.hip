// t1k_amd/csrc/t1k_support.hip -- strand, mate, read-end distance and template support at chosen sites (analyzer --siteSupport):
// what t1k_pileup.hip counts, restricted to a list of (allele, position) sites and split by the evidence behind each booking.  The result
// is ONE sparse T1kCountTable of two key families, kept on the context from t1k_support_begin to _end.
//
// A record (one t1k_pileup_aln) is a window of a read-end; its t1k_support_rec says how long that read-end is (read_len), how many of its
// bases lie in front of the window (clip_front, in the strand-corrected read-end) and on which strand of the allele it lies (strand 0 / 1).
// A booking (one t1k_support_book of the record's list) is an assignment overlap that points at the record: flags bit 0 uniq, bit 1 mate
// (the read-end comes from file 2), bit 2 orient, and the template's extent t_start .. t_end on the allele.
// A column of state 0 .. 6 (A C G T N del ins, the plane order of t1k_walk.h) that books at site s, at allele position pos:
//   c = clip_front + the read bases of the window in front of the column;
//   d = min(c, read_len - 1 - c) for ops 0, 1, 2 (the column consumes base c), min(c, read_len - c) for op 3 (it lies between bases c - 1
//       and c), saturated at 511.  The check pass has made sure that clip_front + the read bases the walk consumes <= read_len, so neither
//       difference wraps: a consuming column has c < read_len, a deletion column c <= read_len.
// Per (hit, booking) two keys, count 1 each:
//   family A  ((((s * 7 + state) * 2 + strand) * 2 + mate) * 512 + d) * 2 + (1 - uniq)                     < 2^28 * 7 * 2^12 < 2^57
//             a uniq booking is stored ONCE, under the even key, as in t1k_sitepile.hip: plain = even + odd, _uniq = even
//   family B  2^57 | (((s * 7 + state) * 2 + orient) << 24) | (dStart << 12) | dEnd                        < 2^58
//             dStart = pos - t_start, dEnd = t_end - pos, each clamped to 0 .. 4095.  The reader counts the RUNS of a (site, state) -- its
//             distinct templates -- and ignores their counts.
// nSites <= 2^28 (else T1K_ERR_CAPACITY) keeps s * 7 + state below 2^31: family A's keys stay below 2^31 * 2^12 = 2^43, under bit 57, which
// family B sets on every one of its keys, and family B's below 2^57 + 2^31 * 2^25 < 2^58.  The sort runs over 58 bits.
// One kernel, two instantiations, one wave64 per record, shaped like k_sitepile; header, walk and verdict are t1k_walk.h's:
//   k_support<false>  check and count: the walk's checks, its own (the read window stays inside the read-end: PILEUP_BAD_READ_WINDOW) and per
//                     record 2 x hits x bookings.  Only when the flag word comes back clear does the host take the exclusive sum and launch
//   k_support<true>   emit at precomputed slots -- no atomics.  Inside a 64-column step with h hits, booking b owns the 2h slots from
//                     slot + 2 b h: its family-A keys are consecutive over the lanes with a hit, its family-B keys follow them the same way
//                     (coalesced stores).  The three words of a booking are wave-uniform loads; the record's t1k_support_rec is loaded once,
//                     beside the header.
// No LDS, no atomics on data (the flag word of the check excepted).  The table and its fold are a T1kCountTable (t1k_table.h), folded
// whenever the pending keys reach a bound (2^28, env T1K_SUPPORT_PENDING) and at _get.  One table for both families keeps a call atomic:
// one t1k_table_room, one t1k_table_commit, one fold.
// Shared with the other sparse stages, and not written out here: the session (ctx->sup, a T1kStage: state checks, _get, _stats, _end, the
// site arguments of _begin) and the check / sum / emit sequence of _add (t1k_stage_two_pass) in t1k_table.h; the checks of records and
// booking lists (pileupBookLists) and the staging (pileupStage) in t1k_walk.h.  Here: the kernel, the key families' bounds, the checks of
// a record's t1k_support_rec and of a booking's template.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_table.h"
#include "t1k_walk.h"

enum { SUPPORT_STATES = 7, SUPPORT_D_MAX = 511, SUPPORT_T_MAX = 4095, SUPPORT_MAX_READ = 65535 };
static const unsigned long long SUPPORT_FAMILY_B = 1ull << 57;

struct SupportArgs {
  PileupBatch in;
  T1kSiteView sites;
  const t1k_support_rec *rec;           // [n]
  const unsigned long long *bookPtr;    // [n + 1] into book
  const t1k_support_book *book;
  unsigned long long *count;            // [n + 1]: <false> writes 2 x hits x bookings, <true> reads their exclusive sums
  unsigned long long *keys;             // <true>: the pending keys of this call
  uint32_t *vals;                       //         and their counts (1 each)
};

template <bool EMIT>
__global__ __launch_bounds__(256) void k_support(SupportArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) {
    const unsigned long long bookAt = pileupUniform64(P.bookPtr[r]);
    const uint32_t nBook = (uint32_t)(pileupUniform64(P.bookPtr[r + 1]) - bookAt);
    if (EMIT && nBook == 0) continue;
    const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);  // (its weights are not read here)
    const uint32_t readLen = pileupUniform(P.rec[r].read_len), clip = pileupUniform(P.rec[r].clip_front), strand = pileupUniform(P.rec[r].strand);
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
      unsigned long long cell = 0, partA = 0;
      if (hit) {
        cell = (unsigned long long)site * SUPPORT_STATES + (op == 2 ? (uint32_t)PILEUP_INS : op == 3 ? (uint32_t)PILEUP_DEL : pileupBasePlane(P.in.text[readAt + myP]));
        const uint32_t c = clip + (uint32_t)myP;                            // (<= read_len <= 65535: the check pass)
        const uint32_t back = op == 3 ? readLen - c : readLen - 1u - c;
        const uint32_t d = min(min(c, back), (uint32_t)SUPPORT_D_MAX);
        partA = (((cell << 1) | strand) << 11) | (d << 1);                  // mate (bit 10) and 1 - uniq (bit 0) come with the booking
      }
      const unsigned long long mine = slot + pileupBelow(mH);
      for (uint32_t b = 0; b < nBook; ++b) {
        const t1k_support_book *e = P.book + bookAt + b;
        const uint32_t flags = pileupUniform(e->flags), tStart = pileupUniform(e->t_start), tEnd = pileupUniform(e->t_end);
        if (hit) {
          const unsigned long long at = mine + 2ull * b * h;
          const uint32_t dStart = pos > tStart ? (uint32_t)min(pos - tStart, (unsigned long long)SUPPORT_T_MAX) : 0u;
          const uint32_t dEnd = tEnd > pos ? (uint32_t)min(tEnd - pos, (unsigned long long)SUPPORT_T_MAX) : 0u;
          P.keys[at] = partA | ((unsigned long long)((flags >> 1) & 1u) << 10) | (1u - (flags & 1u));
          P.vals[at] = 1u;
          P.keys[at + h] = SUPPORT_FAMILY_B | (((cell << 1) | ((flags >> 2) & 1u)) << 24) | ((unsigned long long)dStart << 12) | dEnd;
          P.vals[at + h] = 1u;
        }
      }
      slot += 2ull * h * nBook;
    });
    if (!EMIT) {
      uint32_t bad = pileupWalkVerdict(end, len, readAt, P.in.textBytes);
      if ((unsigned long long)clip + end.p > readLen) bad |= PILEUP_BAD_READ_WINDOW;
      if (lane == 0) {
        if (bad) atomicOr(P.in.flag, bad);
        P.count[r] = 2ull * hits * nBook;
      }
    }
  }
}

extern "C" {

int t1k_support_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos) {
  if (!ctx) return T1K_ERR_ARG;
  T1kStage &s = ctx->sup;
  int rc;
  if ((rc = t1k_stage_closed(ctx, s))) return rc;
  // (site * 7 + state) takes 31 bits at most: family A stays below 2^57, family B below 2^58
  if (nSites > (1ull << 28)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_support_begin: more than 2^28 sites");
  if ((rc = t1k_stage_site_args(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos))) return rc;
  return t1k_stage_open_sites(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos, (SUPPORT_FAMILY_B << 1) - 1ull);
}

int t1k_support_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const t1k_support_rec *rec, const uint64_t *bookPtr, const t1k_support_book *book, const char *text,
                    uint64_t textBytes, const int8_t *ops, uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  T1kStage &s = ctx->sup;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_add", "_begin"))) return rc;
  if (n == 0) return T1K_OK;
  if (!aln || !rec || !bookPtr || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_support_add: bad arguments (NULL arrays)");
  // what the host can tell from the records and the booking lists alone; the strings themselves are walked on the device before anything is emitted
  const std::vector<uint64_t> &off = s.off;
  std::vector<uint64_t> bp;
  if ((rc = pileupBookLists(ctx, "t1k_support_add", aln, n, off, textBytes, opsBytes, bookPtr, 31, book, "book", [&](uint32_t i) -> std::string {
        if (rec[i].strand > 1) return "record " + std::to_string(i) + " has a strand other than 0 or 1";
        if (rec[i].read_len == 0 || rec[i].read_len > SUPPORT_MAX_READ) return "the read length of record " + std::to_string(i) + " lies outside 1 .. 65535";
        if (rec[i].clip_front > rec[i].read_len) return "the read window of record " + std::to_string(i) + " starts behind its read";
        return std::string();
      }, bp))) return rc;
  const uint64_t book0 = bookPtr[0], nBook = bp[n];
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t alleleLen = off[aln[i].allele + 1] - off[aln[i].allele];
    for (uint64_t j = bookPtr[i]; j < bookPtr[i + 1]; ++j) {
      const t1k_support_book &e = book[j];
      if (e.flags >= 8) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_support_add: booking " + std::to_string(j) + " has flags outside 0 .. 7");
      if (e.t_start > e.t_end) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_support_add: the template of booking " + std::to_string(j) + " ends in front of its start");
      if (e.t_end >= alleleLen) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_support_add: the template of booking " + std::to_string(j) + " leaves its allele");
    }
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SupportArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, t1k_sites_offsets(s.map), nullptr};
  size_t oRec = 0, oBp = 0, oBook = 0, oCount = 0;
  if ((rc = pileupStage(ctx, s.in, opsBytes, [&](T1kCarve &piece) {
        oRec = piece(sizeof(t1k_support_rec) * (size_t)n); oBp = piece(8ull * (n + 1ull)); oBook = piece(sizeof(t1k_support_book) * nBook); oCount = piece(8ull * (n + 1ull));
      }, a.in))) return rc;
  char *D = (char *)s.in.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oRec, rec, sizeof(t1k_support_rec) * (size_t)n, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oBp, bp.data(), 8ull * (n + 1ull), hipMemcpyHostToDevice, st));
  if (nBook) T1K_HIP(ctx, hipMemcpyAsync(D + oBook, book + book0, sizeof(t1k_support_book) * nBook, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oCount, 0, 8ull * (n + 1ull), st));
  a.sites = t1k_sites_view(s.map);
  a.rec = (const t1k_support_rec *)(D + oRec);
  a.bookPtr = (const unsigned long long *)(D + oBp); a.book = (const t1k_support_book *)(D + oBook);
  a.count = (unsigned long long *)(D + oCount);
  const unsigned grid = t1k_grid(ctx, n, 4);
  return t1k_stage_two_pass(ctx, s, n, a.in.flag, a.count, kernelMs, [&] { hipLaunchKernelGGL(k_support<false>, dim3(grid), dim3(256), 0, st, a); },
                            [&](unsigned long long *keys, uint32_t *vals) { a.keys = keys; a.vals = vals; hipLaunchKernelGGL(k_support<true>, dim3(grid), dim3(256), 0, st, a); });
}

int t1k_support_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) { return t1k_stage_get(ctx, &t1k_ctx::sup, keys, counts, cap, nRuns); }

int t1k_support_stats(t1k_ctx *ctx, uint64_t *keysEmitted, uint64_t *folds, double *foldMs) { return t1k_stage_stats(ctx, &t1k_ctx::sup, keysEmitted, folds, foldMs); }

int t1k_support_end(t1k_ctx *ctx) { return t1k_stage_end(ctx, &t1k_ctx::sup); }

}  // extern "C"
