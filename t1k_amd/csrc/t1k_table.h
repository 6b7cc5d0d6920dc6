// t1k_amd/csrc/t1k_table.h -- internal: what the four sparse analyzer stages share beyond the walk (t1k_sitepile.hip; t1k_phase.hip,
// §11.5; t1k_support.hip, §11.7; t1k_indel.hip, §11.8); the types live in t1k_dev.h (the context holds them), the host side in t1k_table.hip.
// T1kSiteMap: a set of (allele, position) sites as a bitmap over the allele-offset space (bit alleleOff[a] + p) and a rank directory (sites
// in front of each 64-bit word): a lane maps its allele position to a site index with one bit test and one population count.
// T1kCountTable: a sparse table of counts under 64-bit keys.  It is (key, count) pairs, ascending, followed by pending keys of count 1.
// A stage asks for room behind the pending keys (t1k_table_room), has a kernel write its keys there (count 1 each, no atomics) and commits
// them (t1k_table_commit).  Fold: t1k_sort_pairs over the bits of the largest possible key, t1k_run_table (t1k_sort.hip) numbers the runs,
// an inclusive scan of the counts (uint32, exact modulo 2^32) gives every run's sum as the difference of the scan at its last element and
// at the previous run's last element: a run's sum is at most (2^31 - 1) + the pending keys < 2^32, so the difference is exact, and no
// lane ever walks a run.  A sum beyond 2^31 - 1 refuses the fold (T1K_ERR_CAPACITY) and leaves the table as it was.  The table is folded
// whenever the pending keys reach its bound and when it is read.  `who` is the stage's name, the head of every message.
// T1kStage: the session around one table, from a stage's _begin to its _end -- the state checks and their messages, _get, the table part
// of _stats, _end, the argument checks and the opening of a stage with sites, the end of an _add call's event pair (t1k_stage_done) and
// the two-pass sequence of an _add call that counts, sums and emits (t1k_stage_two_pass).  None of it asks which stage is calling: what
// differs comes in as the T1kStage's own data (its names, its list of further blocks) or as a callback.  A stage's entry points keep
// what is theirs: the key layout, their own argument checks in their own order, the kernels and their launches.
#pragma once
#include <string>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_walk.h"

// ---- sites ----
// what a kernel takes of a T1kSiteMap
struct T1kSiteView {
  const unsigned long long *bits;  // [total / 64 + 1]
  const uint32_t *rank;            // [total / 64 + 1]
};
// is position g of the offset space a site, and which: the sites in front of it
__device__ __forceinline__ bool t1kSiteAt(const T1kSiteView &v, unsigned long long g, uint32_t &site) {
  const unsigned long long w = v.bits[g >> 6];
  site = v.rank[g >> 6] + (uint32_t)__popcll(w & ((1ull << (g & 63u)) - 1ull));
  return (w >> (g & 63u)) & 1ull;
}
inline T1kSiteView t1k_sites_view(const T1kSiteMap &m) {
  const char *S = (const char *)m.buf.p;
  return T1kSiteView{(const unsigned long long *)(S + m.at[0]), (const uint32_t *)(S + m.at[1])};
}
inline const unsigned long long *t1k_sites_offsets(const T1kSiteMap &m) { return (const unsigned long long *)((const char *)m.buf.p + m.at[2]); }

// ---- the count table ----
// room for `emit` more pending keys: T1K_ERR_CAPACITY (`hint`: what the caller can do about it) when the table would pass 2^31 entries;
// *keys / *vals: where they go.  What the table holds is kept.
int t1k_table_room(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit, const char *hint, unsigned long long **keys, uint32_t **vals);
// the `emit` keys written behind t1k_table_room are the table's; folds at the bound.  A fold that fails drops them again
int t1k_table_commit(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit);

// ---- the session of a stage: `fn` is the entry point's suffix ("_get"), the stage's name in front of it heads the message ----
// T1K_ERR_STATE when the stage is open (a _begin) / when it is not; hint: what the caller does first ("_begin"), for the message of an _add
int t1k_stage_closed(t1k_ctx *ctx, const T1kStage &s);
int t1k_stage_opened(t1k_ctx *ctx, const T1kStage &s, const char *fn, const char *hint = nullptr);
// the arguments of a _begin with sites: the site arrays given, alleleOff sound (pileupCheckOffsets), no more sites than allele positions
int t1k_stage_site_args(t1k_ctx *ctx, const T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos);
// the stage is open: alleleOff kept on the host, an empty table whose keys are all <= largestKey
void t1k_stage_open(T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, unsigned long long largestKey);
// checks the sites (inside the alleles, strictly ascending by (allele, pos): T1K_ERR_ARG), builds bitmap and directory, uploads them with
// alleleOff, then t1k_stage_open.  The arguments have passed t1k_stage_site_args.
int t1k_stage_open_sites(t1k_ctx *ctx, T1kStage &s, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos,
                         unsigned long long largestKey);
// the bodies of the twelve entry points _get, _stats (its table part; a stage's own counters follow in its file) and _end.  _get folds,
// then *nRuns = the runs; with keys and counts given (cap >= *nRuns entries each) they are copied out.  _end synchronises, closes map and
// table and frees every block of the stage
int t1k_stage_get(t1k_ctx *ctx, T1kStage t1k_ctx::*which, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
int t1k_stage_stats(t1k_ctx *ctx, T1kStage t1k_ctx::*which, uint64_t *keysEmitted, uint64_t *folds, double *foldMs);
int t1k_stage_end(t1k_ctx *ctx, T1kStage t1k_ctx::*which);
// stops the event pair of an _add call (ev[0] recorded at its start), synchronises -- the caller's arrays are the caller's again, the
// staging block the next call's -- and reports the device time
int t1k_stage_done(t1k_ctx *ctx, double *kernelMs);
// the sequence of an _add call whose check pass leaves per record the keys it will emit: check(): the launch that counts into count[0 .. n)
// (count[n] is 0) and ORs into *flag; the exclusive sum goes in behind it, then flag and total come back with ONE synchronise.  A refused
// batch and an empty one return before t1k_table_room: the table is untouched.  emit(keys, vals): the launch that writes the keys.
template <class Check, class Emit>
inline int t1k_stage_two_pass(t1k_ctx *ctx, T1kStage &s, uint32_t n, const uint32_t *flag, unsigned long long *count, double *kernelMs, Check &&check, Emit &&emit) {
  hipStream_t st = ctx->stream;
  const std::string add = std::string(s.who) + "_add";
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  check();
  T1K_HIP(ctx, hipGetLastError());
  int rc;
  if ((rc = t1k_exclusive_sum_u64(ctx, count, count, (uint64_t)n + 1))) return rc;  // (in place: every tile is read before it is written)
  uint32_t bad = 0;
  unsigned long long total = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&total, count + n, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (bad) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal(add.c_str(), "nothing emitted", bad));
  if (total == 0) return t1k_stage_done(ctx, kernelMs);
  unsigned long long *keys = nullptr;
  uint32_t *vals = nullptr;
  const std::string hint = std::string("lower ") + s.boundEnv + ", or add fewer records per call";
  if ((rc = t1k_table_room(ctx, s.who, s.tab, total, hint.c_str(), &keys, &vals))) return rc;
  emit(keys, vals);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_stage_done(ctx, kernelMs))) return rc;
  return t1k_table_commit(ctx, s.who, s.tab, total);
}
