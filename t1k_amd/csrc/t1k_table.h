// t1k_amd/csrc/t1k_table.h -- internal: the two pieces the sparse analyzer stages share (t1k_sitepile.hip; t1k_phase.hip, §11.5; t1k_support.hip, §11.7);
// the types live in t1k_dev.h (the context holds them), the host side in t1k_table.hip.
// T1kSiteMap: a set of (allele, position) sites as a bitmap over the allele-offset space (bit alleleOff[a] + p) and a rank directory (sites
// in front of each 64-bit word): a lane maps its allele position to a site index with one bit test and one population count.
// T1kCountTable: a sparse table of counts under 64-bit keys.  It is (key, count) pairs, ascending, followed by pending keys of count 1.
// A stage asks for room behind the pending keys (t1k_table_room), has a kernel write its keys there (count 1 each, no atomics) and commits
// them (t1k_table_commit).  Fold: t1k_sort_pairs over the bits of the largest possible key, t1k_run_table (t1k_sort.hip) numbers the runs,
// an inclusive scan of the counts (uint32, exact modulo 2^32) gives every run's sum as the difference of the scan at its last element and
// at the previous run's last element: a run's sum is at most (2^31 - 1) + the pending keys < 2^32, so the difference is exact, and no
// lane ever walks a run.  A sum beyond 2^31 - 1 refuses the fold (T1K_ERR_CAPACITY) and leaves the table as it was.  The table is folded
// whenever the pending keys reach its bound and when it is read.  `who` is the stage's name, the head of every message.
#pragma once
#include <string>
#include "t1k_dev.h"
#include "t1k_launch.h"

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
// checks the sites (inside the alleles, strictly ascending by (allele, pos): T1K_ERR_ARG), builds bitmap and directory and uploads them
// with alleleOff; m.off and m.nSites are set.  alleleOff has passed pileupCheckOffsets.
int t1k_sites_build(t1k_ctx *ctx, const char *who, T1kSiteMap &m, uint32_t nAlleles, const uint64_t *alleleOff, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos);
inline T1kSiteView t1k_sites_view(const T1kSiteMap &m) {
  const char *S = (const char *)m.buf.p;
  return T1kSiteView{(const unsigned long long *)(S + m.at[0]), (const uint32_t *)(S + m.at[1])};
}
inline const unsigned long long *t1k_sites_offsets(const T1kSiteMap &m) { return (const unsigned long long *)((const char *)m.buf.p + m.at[2]); }
void t1k_sites_close(T1kSiteMap &m);

// ---- the count table ----
// an empty table whose keys are all <= largestKey; boundEnv: the environment variable that overrides the pending bound of 2^28
void t1k_table_open(T1kCountTable &t, unsigned long long largestKey, const char *boundEnv);
// room for `emit` more pending keys: T1K_ERR_CAPACITY (`hint`: what the caller can do about it) when the table would pass 2^31 entries;
// *keys / *vals: where they go.  What the table holds is kept.
int t1k_table_room(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit, const char *hint, unsigned long long **keys, uint32_t **vals);
// the `emit` keys written behind t1k_table_room are the table's; folds at the bound.  A fold that fails drops them again
int t1k_table_commit(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t emit);
// folds, then *nRuns = the runs; with keys and counts given (cap >= *nRuns entries each) they are copied out
int t1k_table_get(t1k_ctx *ctx, const char *who, T1kCountTable &t, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
void t1k_table_close(T1kCountTable &t);
