// t1k_amd/csrc/t1k_phase.hip -- read-backed phasing of site pairs (analyzer --phase): which states two sites show on one
// fragment.  The result is the list of (site s, site t > s, state at s, state at t) cells that received a booking, with their counts
// over all bookings and over those of fragments with one assignment (_uniq), kept on the context from t1k_phase_begin to _end.
//
// Observation of a record (one t1k_pileup_aln) at a site: the column of its edit string that consumes that allele position -- ops 0 and
// 1 give the read base as A/C/G/T, anything else as N, op 3 gives del: six states 0 .. 5, the plane order of t1k_walk.h.  Insert columns
// observe nothing, so a record observes a site at most once and its observations come out ascending in site index.
// A booking is a fragment-assignment: rec1, an optional rec2 (its mate, on the same allele) and a uniq flag.  Its observations are the
// union of its records': a site both mates show in the same state counts once, a site they show in different states is dropped for
// this booking (and counted as discordant).  rec1 == rec2 gives that record's own list.  A booking with observed sites s < t in states
// x, y adds 1 to cell (s, t, x, y), for every unordered pair of its observed sites.
// Key = (((s * nSites + t) * 36 + x * 6 + y) << 1) | (1 - uniq), below 2^63 for nSites <= 2^28.  As in t1k_sitepile.hip a uniq booking is
// emitted once, under the even key: the reader of t1k_phase_get forms plain = even + odd, _uniq = even.
// Kernels of one _add call, none with atomics on data (the flag word of the check excepted):
//   k_phase_obs<false>  one wave64 per record on pileupWalk: the walk's checks into the flag word and the record's observations h(r).
//                       Only when the flag word comes back clear does the host take the exclusive sum of the counts (obsPtr) and launch
//   k_phase_obs<true>   the record's observation words site << 3 | state at obsPtr[r] + running total: the running totals are wave-uniform,
//                       the stores ballot-compacted.
//   k_phase_need        one lane per booking: u = h(rec1) + h(rec2) (rec2 only if present and another record than rec1), 0 when u < 2 --
//                       such a booking makes no pair.  The exclusive sum gives each booking its slice of the merge arena.
//   k_phase_merge       one wave64 per booking with u >= 2, 64 elements a step: each element of one list looks for its site in the other
//                       list by binary search (both ascending, L2-resident): unique, same state (list 1's copy survives) or discordant
//                       (neither survives).  Survivors are compacted by ballot into the slice, list 1's first, then list 2's -- the set
//                       need not be sorted, a pair orders itself when its key is built.  Writes m, the pair count m (m - 1) / 2 and the
//                       discordant sites.
//   k_phase_pairs       after the exclusive sum of the pair counts: one wave64 per booking with m >= 2.  Row i is wave-uniform, j = i + 1 +
//                       lane strides by 64; row i starts at i (2m - i - 1) / 2 and the key of (i, j) goes to slot + row start + (j - i - 1):
//                       the lanes of a row write consecutive keys.  No LDS, and nothing bounds a list's length.
// The table and its fold are a T1kCountTable (t1k_table.h), folded whenever the pending keys reach a bound (2^28, env T1K_PHASE_PENDING)
// and at _get.  Pairs grow with the square of a booking's observed sites; the table refuses what would pass 2^31 entries (T1K_ERR_CAPACITY).
// Shared with the other sparse stages, and not written out here: the session (ctx->ph, a T1kStage: state checks, _get, the table part of
// _stats, _end, the site arguments of _begin) and the end of an _add call (t1k_stage_done) in t1k_table.h; the record checks and the
// staging (pileupStage) in t1k_walk.h.  _add is this stage's own: its bookings name records instead of hanging off them, and its pipeline
// is five kernels with three sums between them.
#include <algorithm>
#include <cstdlib>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_table.h"
#include "t1k_walk.h"

enum { PHASE_STATES = 6 };
enum { PHASE_OBS = 0, PHASE_ARENA = 1 };  // of ctx->ph.more: one _add call's observation words and its merge arena
static const uint32_t PHASE_NO_MATE = 0xFFFFFFFFu;

struct PhaseArgs {
  PileupBatch in;
  T1kSiteView sites;
  unsigned long long nSites;
  unsigned long long *obsPtr;            // [n + 1]: obs<false> writes h(r), the later kernels read the exclusive sums
  uint32_t *obs;                         // observation words of the call, record by record
  uint32_t nBook;
  const uint32_t *bookRec;               // [2 * nBook] rec1, rec2 or PHASE_NO_MATE
  const uint8_t *bookUniq;               // [nBook]
  unsigned long long *need;              // [nBook + 1]: need writes u or 0, merge and pairs read the exclusive sums (arena slices)
  uint32_t *arena;                       // the bookings' merged observation words
  uint32_t *m;                           // [nBook] merged observations of a booking
  unsigned long long *pairs;             // [nBook + 1]: need / merge write m (m - 1) / 2, pairs reads the exclusive sums (key slots)
  unsigned long long *stat;              // [nBook + 1]: (m >= 2) << 32 | discordant sites, summed on the device for _stats
  unsigned long long *keys;              // pairs: the pending keys of this call
  uint32_t *vals;                        //        and their counts (1 each)
};

template <bool EMIT>
__global__ __launch_bounds__(256) void k_phase_obs(PhaseArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) {
    unsigned long long slot = 0;
    if (EMIT) {
      slot = pileupUniform64(P.obsPtr[r]);
      if (pileupUniform64(P.obsPtr[r + 1]) == slot) continue;
    }
    const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);  // (its weights are not read here)
    const unsigned long long base = R.base, len = R.len, readAt = R.readAt;
    unsigned long long hits = 0;
    const PileupWalkEnd end = pileupWalk<!EMIT, true>(P.in.ops, R.opsAt, R.nOps, R.seqStart, len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long myP) {
      bool hit = false;
      uint32_t site = 0;
      if (active && op != 2 && pos < len) hit = t1kSiteAt(P.sites, base + pos, site);  // (pos >= len: only in the check pass, on a walk it is about to refuse)
      const uint64_t mH = __ballot(hit ? 1 : 0);
      const uint32_t h = (uint32_t)__popcll(mH);
      if (!EMIT) { hits += h; return; }
      if (hit) P.obs[slot + pileupBelow(mH)] = (site << 3) | (op == 3 ? (uint32_t)PILEUP_DEL : pileupBasePlane(P.in.text[readAt + myP]));
      slot += h;
    });
    if (!EMIT) {
      const uint32_t bad = pileupWalkVerdict(end, len, readAt, P.in.textBytes);
      if (lane == 0) {
        if (bad) atomicOr(P.in.flag, bad);
        P.obsPtr[r] = hits;
      }
    }
  }
}

// the observation list of record r
struct PhaseList {
  const uint32_t *p;
  uint32_t n;
};
__device__ __forceinline__ PhaseList phaseList(const PhaseArgs &P, uint32_t r) {
  const unsigned long long at = P.obsPtr[r];
  return PhaseList{P.obs + at, (uint32_t)(P.obsPtr[r + 1] - at)};
}

__global__ __launch_bounds__(256) void k_phase_need(PhaseArgs P) {
  for (uint32_t b = blockIdx.x * 256u + threadIdx.x; b < P.nBook; b += gridDim.x * 256u) {
    const uint32_t r1 = P.bookRec[2ull * b], r2 = P.bookRec[2ull * b + 1ull];
    unsigned long long u = P.obsPtr[r1 + 1] - P.obsPtr[r1];
    if (r2 != PHASE_NO_MATE && r2 != r1) u += P.obsPtr[r2 + 1] - P.obsPtr[r2];
    P.need[b] = u < 2 ? 0ull : u;
    P.m[b] = (uint32_t)u;    // (k_phase_merge overwrites the three of a booking with u >= 2)
    P.pairs[b] = 0;
    P.stat[b] = 0;
  }
}

// the word of `list` at site `site`, or 0xFFFFFFFF (no observation word is: a site index has 28 bits)
__device__ __forceinline__ uint32_t phaseFind(const PhaseList &list, uint32_t site) {
  uint32_t lo = 0, hi = list.n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((list.p[mid] >> 3) < site) lo = mid + 1; else hi = mid;
  }
  if (lo < list.n) {
    const uint32_t w = list.p[lo];
    if ((w >> 3) == site) return w;
  }
  return 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_phase_merge(PhaseArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t b = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); b < P.nBook; b += nWaves) {
    const unsigned long long at = pileupUniform64(P.need[b]);
    if (pileupUniform64(P.need[b + 1]) == at) continue;  // u < 2
    const uint32_t r1 = pileupUniform(P.bookRec[2ull * b]), r2 = pileupUniform(P.bookRec[2ull * b + 1ull]);
    const PhaseList one = phaseList(P, r1);
    PhaseList two{nullptr, 0};
    if (r2 != PHASE_NO_MATE && r2 != r1) two = phaseList(P, r2);
    uint32_t *out = P.arena + at;
    uint32_t m = 0, discordant = 0;  // wave-uniform
    for (uint32_t i0 = 0; i0 < one.n; i0 += 64u) {
      const uint32_t i = i0 + lane;
      bool keep = false, clash = false;
      uint32_t w = 0;
      if (i < one.n) {
        w = one.p[i];
        const uint32_t other = phaseFind(two, w >> 3);
        clash = other != 0xFFFFFFFFu && other != w;
        keep = !clash;
      }
      const uint64_t mK = __ballot(keep ? 1 : 0);
      if (keep) out[m + pileupBelow(mK)] = w;
      m += (uint32_t)__popcll(mK);
      discordant += (uint32_t)__popcll(__ballot(clash ? 1 : 0));
    }
    for (uint32_t i0 = 0; i0 < two.n; i0 += 64u) {
      const uint32_t i = i0 + lane;
      bool keep = false;
      uint32_t w = 0;
      if (i < two.n) {
        w = two.p[i];
        keep = phaseFind(one, w >> 3) == 0xFFFFFFFFu;  // seen by list 1 as well: its copy survived, or neither does
      }
      const uint64_t mK = __ballot(keep ? 1 : 0);
      if (keep) out[m + pileupBelow(mK)] = w;
      m += (uint32_t)__popcll(mK);
    }
    if (lane == 0) {
      P.m[b] = m;
      P.pairs[b] = (unsigned long long)m * (m - (m ? 1u : 0u)) / 2ull;
      P.stat[b] = ((unsigned long long)(m >= 2u ? 1u : 0u) << 32) | discordant;
    }
  }
}

__global__ __launch_bounds__(256) void k_phase_pairs(PhaseArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t b = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); b < P.nBook; b += nWaves) {
    const unsigned long long slot = pileupUniform64(P.pairs[b]);
    if (pileupUniform64(P.pairs[b + 1]) == slot) continue;  // m < 2
    const uint32_t m = pileupUniform(P.m[b]);
    const uint32_t odd = P.bookUniq[b] ? 0u : 1u;
    const uint32_t *set = P.arena + pileupUniform64(P.need[b]);
    for (uint32_t i = 0; i + 1u < m; ++i) {
      const uint32_t wi = pileupUniform(set[i]);
      const unsigned long long row = slot + (unsigned long long)i * (2ull * m - i - 1ull) / 2ull;
      for (uint32_t j = i + 1u + lane; j < m; j += 64u) {
        const uint32_t wj = set[j];
        const uint32_t lo = (wi >> 3) < (wj >> 3) ? wi : wj, hi = lo == wi ? wj : wi;  // (two survivors never share a site)
        const unsigned long long cell = ((unsigned long long)(lo >> 3) * P.nSites + (hi >> 3)) * (PHASE_STATES * PHASE_STATES) + (lo & 7u) * PHASE_STATES + (hi & 7u);
        P.keys[row + (j - i - 1u)] = (cell << 1) | odd;
        P.vals[row + (j - i - 1u)] = 1u;
      }
    }
  }
}

extern "C" {

int t1k_phase_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos) {
  if (!ctx) return T1K_ERR_ARG;
  T1kStage &s = ctx->ph;
  int rc;
  if ((rc = t1k_stage_closed(ctx, s))) return rc;
  // a site index takes 28 bits of an observation word, and the largest key, nSites^2 * 72 - 1, stays below 2^63
  if (nSites > (1ull << 28)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_phase_begin: more than 2^28 sites");
  if ((rc = t1k_stage_site_args(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos))) return rc;
  const unsigned long long space = nSites * nSites * (2ull * PHASE_STATES * PHASE_STATES);
  ctx->phObs = ctx->phBookings = ctx->phDiscordant = 0;
  return t1k_stage_open_sites(ctx, s, nAlleles, alleleOff, nSites, siteAllele, sitePos, space ? space - 1 : 0ull);
}

int t1k_phase_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, uint32_t nBook, const uint32_t *bookRec, const uint8_t *bookUniq, const char *text, uint64_t textBytes,
                  const int8_t *ops, uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  T1kStage &s = ctx->ph;
  T1kDevBuf &bObs = s.more[PHASE_OBS].b, &bArena = s.more[PHASE_ARENA].b;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_add", "_begin"))) return rc;
  if ((n && !aln) || (nBook && (!bookRec || !bookUniq)) || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_phase_add: bad arguments (NULL arrays)");
  // what the host can tell from the records and the bookings alone; the strings themselves are walked on the device before anything is emitted
  for (uint32_t i = 0; i < n; ++i) {
    const std::string fault = pileupRecordFault(aln[i], i, s.off, textBytes, opsBytes);
    if (!fault.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_phase_add: " + fault);
  }
  for (uint32_t b = 0; b < nBook; ++b) {
    const uint32_t r1 = bookRec[2ull * b], r2 = bookRec[2ull * b + 1];
    if (r1 >= n || (r2 != PHASE_NO_MATE && r2 >= n)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_phase_add: booking " + std::to_string(b) + " names a record outside the call");
    if (r2 != PHASE_NO_MATE && aln[r1].allele != aln[r2].allele) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_phase_add: the mates of booking " + std::to_string(b) + " lie on different alleles");
  }
  if (n == 0) return T1K_OK;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PhaseArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, t1k_sites_offsets(s.map), nullptr};
  size_t oRec = 0, oUniq = 0, oObsPtr = 0, oNeed = 0, oM = 0, oPairs = 0, oStat = 0;
  if ((rc = pileupStage(ctx, s.in, opsBytes, [&](T1kCarve &piece) {
        oRec = piece(8ull * nBook); oUniq = piece(nBook); oObsPtr = piece(8ull * (n + 1ull)); oNeed = piece(8ull * (nBook + 1ull)); oM = piece(4ull * nBook);
        oPairs = piece(8ull * (nBook + 1ull)); oStat = piece(8ull * (nBook + 1ull));
      }, a.in))) return rc;
  char *D = (char *)s.in.p;
  if (nBook) {
    T1K_HIP(ctx, hipMemcpyAsync(D + oRec, bookRec, 8ull * nBook, hipMemcpyHostToDevice, st));
    T1K_HIP(ctx, hipMemcpyAsync(D + oUniq, bookUniq, nBook, hipMemcpyHostToDevice, st));
  }
  T1K_HIP(ctx, hipMemsetAsync(D + oObsPtr, 0, 8ull * (n + 1ull), st));
  a.sites = t1k_sites_view(s.map);
  a.nSites = s.map.nSites;
  a.obsPtr = (unsigned long long *)(D + oObsPtr);
  a.nBook = nBook;
  a.bookRec = (const uint32_t *)(D + oRec); a.bookUniq = (const uint8_t *)(D + oUniq);
  a.need = (unsigned long long *)(D + oNeed); a.m = (uint32_t *)(D + oM); a.pairs = (unsigned long long *)(D + oPairs); a.stat = (unsigned long long *)(D + oStat);
  const unsigned gridRec = t1k_grid(ctx, n, 4), gridBook = t1k_grid(ctx, nBook, 4);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_phase_obs<false>, dim3(gridRec), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_exclusive_sum_u64(ctx, a.obsPtr, a.obsPtr, (uint64_t)n + 1))) return rc;  // (in place: every tile is read before it is written)
  uint32_t flag = 0;
  unsigned long long nObs = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.in.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&nObs, a.obsPtr + n, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal("t1k_phase_add", "nothing emitted", flag));
  if (nObs >= (1ull << 31)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_phase_add: 2^31 observations or more in one call (add fewer records per call)");
  unsigned long long nArena = 0, emit = 0, stat = 0;
  if (nObs && nBook) {
    if ((rc = t1k_ensure(ctx, bObs, 4ull * nObs))) return rc;
    a.obs = (uint32_t *)bObs.p;
    hipLaunchKernelGGL(k_phase_obs<true>, dim3(gridRec), dim3(256), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
    T1K_HIP(ctx, hipMemsetAsync(a.need + nBook, 0, 8, st));
    T1K_HIP(ctx, hipMemsetAsync(a.pairs + nBook, 0, 8, st));
    T1K_HIP(ctx, hipMemsetAsync(a.stat + nBook, 0, 8, st));
    hipLaunchKernelGGL(k_phase_need, dim3(t1k_grid(ctx, nBook, 256)), dim3(256), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
    if ((rc = t1k_exclusive_sum_u64(ctx, a.need, a.need, (uint64_t)nBook + 1))) return rc;
    T1K_HIP(ctx, hipMemcpyAsync(&nArena, a.need + nBook, 8, hipMemcpyDeviceToHost, st));
    T1K_HIP(ctx, hipStreamSynchronize(st));
  }
  if (nArena >= (1ull << 31))
    return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_phase_add: the bookings of one call observe 2^31 sites or more (fewer sites, or add fewer records per call)");
  if (nArena) {
    if ((rc = t1k_ensure(ctx, bArena, 4ull * nArena))) return rc;
    a.arena = (uint32_t *)bArena.p;
    hipLaunchKernelGGL(k_phase_merge, dim3(gridBook), dim3(256), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
    if ((rc = t1k_exclusive_sum_u64(ctx, a.pairs, a.pairs, (uint64_t)nBook + 1))) return rc;
    if ((rc = t1k_exclusive_sum_u64(ctx, a.stat, a.stat, (uint64_t)nBook + 1))) return rc;  // (fewer than 2^32 discordant sites: no carry into the bookings)
    T1K_HIP(ctx, hipMemcpyAsync(&emit, a.pairs + nBook, 8, hipMemcpyDeviceToHost, st));
    T1K_HIP(ctx, hipMemcpyAsync(&stat, a.stat + nBook, 8, hipMemcpyDeviceToHost, st));
    T1K_HIP(ctx, hipStreamSynchronize(st));
  }
  if (emit) {
    // (the bookings' observed sites add up to less than 2^31, so the sum of their m (m - 1) / 2 is far from wrapping)
    if ((rc = t1k_table_room(ctx, s.who, s.tab, emit,
                             "pairs grow with the square of a booking's observed sites: fewer sites, a lower T1K_PHASE_PENDING, or fewer records per call", &a.keys, &a.vals)))
      return rc;
    hipLaunchKernelGGL(k_phase_pairs, dim3(gridBook), dim3(256), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
  }
  if ((rc = t1k_stage_done(ctx, kernelMs))) return rc;
  if (emit && (rc = t1k_table_commit(ctx, s.who, s.tab, emit))) return rc;
  ctx->phObs += nObs;
  ctx->phBookings += stat >> 32;
  ctx->phDiscordant += stat & 0xFFFFFFFFull;
  return T1K_OK;
}

int t1k_phase_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) { return t1k_stage_get(ctx, &t1k_ctx::ph, keys, counts, cap, nRuns); }

int t1k_phase_stats(t1k_ctx *ctx, uint64_t *observations, uint64_t *bookings, uint64_t *keysEmitted, uint64_t *discordant, uint64_t *folds, double *foldMs) {
  int rc;
  if ((rc = t1k_stage_stats(ctx, &t1k_ctx::ph, keysEmitted, folds, foldMs))) return rc;
  if (observations) *observations = ctx->phObs;
  if (bookings) *bookings = ctx->phBookings;
  if (discordant) *discordant = ctx->phDiscordant;
  return T1K_OK;
}

int t1k_phase_end(t1k_ctx *ctx) { return t1k_stage_end(ctx, &t1k_ctx::ph); }

}  // extern "C"
