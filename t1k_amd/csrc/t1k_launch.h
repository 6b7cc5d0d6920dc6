// t1k_amd/csrc/t1k_launch.h -- internal: kernel argument blocks and host launchers shared by the .hip files
#pragma once
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "t1k_dev.h"

#define T1K_USED_MASK_WORDS 10
struct ChainArgs {
  T1kRefDev ref;
  T1kReadsDev reads;
  int k, radius, hitLenRequired;
  double sim;
  uint32_t *recs; uint32_t recStride; uint64_t groupCap;   // group records: re|strand, allele, diag, meta, M[...]
  uint32_t *chunkStart, *chunkCount; int maxChunks;        // [re][maxChunks] runs of groups per (strand, allele chunk), reference order
  uint32_t *usedMask;                                      // [re][2][T1K_USED_MASK_WORDS] bit r = the list of the k-mer at read offset r (that strand) is used (k_near_hits rebuilds hits on near diagonals from it)
  uint32_t *usedOut, *usedCount;                           // [re][maxK][4] used k-mers (readOff, listStart, listLen, directory row); [re][2] counts per strand
  unsigned long long *memo;                                // [re][GAP_CACHE] memo of gap alignments
  uint32_t *jobList; uint32_t jobCap;
  uint32_t *retryList, *generalList, *bigList;  // dense lists (filled by k_arena_compact)
  uint32_t *jobStr, *retryStr, *generalStr, *bigStr, *finishStr, *waveStr, *waveList, *slowStr, *slowList;  // striped arenas the kernels append to
  uint32_t groupSegCap, jobSegCap, listSegCap, rareSegCap, genCandSegCap, genHitSegCap;  // listSegCap: slow / retry / finish arenas; rareSegCap: general / wave / big
  uint32_t maxK;  // upper bound of the k-mers of a read-end (both strands): stride of the used-list table
  uint32_t maxKFast;  // the same for the read-ends k_seed_groups takes (<= T1K_MAX_READ_LEN bases): its LDS layout; < maxK in a window with longer reads
  uint32_t *genJobStr, *genJobList; uint32_t genJobSegCap;  // alignments registered by the multi-diagonal groups
  uint32_t *genHits;  // hit lists of the multi-diagonal groups (k_gather_general)
  uint32_t *genCand; uint32_t genCandCap;                  // packed candidates of multi-diagonal groups (3 u32 each)
  uint32_t *bigScratch;
  int devDriven;           // this submission holds no counter fetch between its launches (t1k_run_chain: always 1): a launch behind an overflow ends at once
  int nearSimple;          // k_near_hits marks the two-diagonal groups whose hit list is its chain (T1K_NO_SIMPLE_CHAIN=1: leaves them to the general path)
  int earlyPrune;          // k_chain_fast<*, 0>: 0 = closed form only (T1K_NO_EARLY_PRUNE=1), 1 = + the groups that cannot pass the similarity filter by the gap-count bound
                           // (T1K_WALK_IN_CLOSED=0), 2 = + the gap walk's first pass: groups without a gap of more than three mismatches and groups its bound prunes (default)
  T1kCand *cand; uint64_t candCap;
  uint32_t *candStart, *candCount;
  unsigned long long *counters;
};

struct ExtendArgs {
  T1kRefDev ref;
  T1kReadsDev reads;
  int k;
  double sim;
  const T1kCand *cand;
  T1kExt *ext;
  uint64_t nCand;
  unsigned long long *counters;
  unsigned long long *memo;                 // per-read-end alignment memo (t1k_memo.h)
  uint32_t *jobStr; uint32_t jobSegCap;     // striped list of registered alignments
  uint32_t *retryStr; uint32_t retrySegCap; // striped list of candidates waiting for them
};

struct SelectArgs {
  T1kReadsDev reads;
  const T1kCand *cand;
  const T1kExt *ext;
  const uint32_t *candStart, *candCount;
  T1kOvl *ovl; uint64_t ovlCap;
  uint32_t *ovlStart, *ovlCount;
  // the packed form (k_select<.., PK = true>: deferred coverage without --relaxIntronAlign) finishes the lists itself: records cut and
  // packed into the store, the read set's list table written for the range (entries of this range's first read-end; reads.skip honoured)
  T1kOvlP *store;
  unsigned long long *listPtr;
  uint32_t *listCount;
  uint64_t *sortScratch;   // [wg][sortCap] packed keys (per-workgroup stride: sortCap * 6 words, shared with k_truncate)
  uint32_t sortCap;
  int alleleBits;          // bits of an allele index
  int relax;               // --relaxIntronAlign: the relaxed match counts come from the full alignments (else k_select writes them)
  int xl;                  // the window holds reads beyond T1K_MAX_READ_LEN: wider sort-key fields
  unsigned long long *counters;
  // read-ends by size class (k_select_classes): [class][nReadEnds], dense and ascending; a selection launch gets its own class's list,
  // the counter word that holds its length and the word it hands positions out from
  uint32_t *classList;
  int lenWord, hoWord;
};

struct FullArgs {
  T1kRefDev ref;
  T1kReadsDev reads;
  int relax;
  int noCov;               // the alignments only feed the relaxed counts: no per-base coverage is added (t1k_ctx_set_coverage_mode 1)
  int fullLen;             // span counted in ref.covFull
  int undo;                // second pass over the same records after an alignment queue overflowed: the coverage the first pass added for the
                           // ungapped alignments is taken back (weights negated, integer atomics: exact) and nothing is queued -- the range can run again
  T1kOvl *ovl;
  uint64_t nOvl;
  uint32_t *eqStr, *bandStr, *wideStr; uint32_t segCap;  // striped alignment queues
  unsigned long long *eqKeyStr, *bandKeyStr;              // their sort keys (see k_fullalign)
  unsigned long long *counters;
};

struct SlowArgs {
  T1kRefDev ref;
  T1kReadsDev reads;
  int relax;
  int noCov;
  T1kOvl *ovl;
  const uint32_t *slowQueue;  // (sorted) queue of overlap indices
  uint32_t nSlow;
  const uint32_t *runOf, *rep; uint32_t nRuns; uint64_t traceStride;  // runs of identical jobs: 1-based run of each job, first job of each run
  uint8_t *scratch; uint64_t perThread;  // per thread: int rows[GA_SCRATCH_INTS] | int8 ops[] | trace bytes
  int maxCells;
  unsigned long long *counters;
};

struct TruncArgs {
  T1kReadsDev reads;
  T1kOvl *ovl;
  const uint32_t *ovlStart;
  uint32_t *ovlCount;
  uint64_t *sortScratch; uint32_t sortCap;   // keys, then a T1kOvl staging area of sortCap records
  int alleleBits;
  int xl;                  // as SelectArgs::xl
  unsigned long long *counters;
};

// All fragment rows of a job on one GPU (t1k_pair_into appends, several contexts concurrently) and their coalescing into read
// groups (t1k_coalesce.hip).  Rows live in chunks; a fragment's row is contiguous, ordered by allele index.
struct t1k_rowset {
  int device = 0;
  t1k_ctx *owner = nullptr;         // its stream runs the coalescing kernels
  uint64_t nFrag = 0;
  T1kDevBuf bFrag;                  // rowPtr | h1 | h2 | rowCount | assigned
  unsigned long long *rowPtr = nullptr, *h1 = nullptr, *h2 = nullptr;
  uint32_t *rowCount = nullptr;
  uint8_t *assigned = nullptr;
  // after t1k_rowset_exchange: the fragments this rank owns (bFrag2 / bRecv), gid = their global fragment index
  uint32_t *gid = nullptr;
  bool exchanged = false;
  uint64_t nFragLocal = 0;
  T1kDevBuf bSend, bRecv, bFrag2, bAll;
  uint64_t allGroups = 0, allEntries = 0;
  T1kDevBuf bCursors;               // one append cursor per chunk
  std::vector<T1kDevBuf> chunks;
  size_t cur = 0;
  uint64_t chunkEntries = 0;
  std::mutex m;
  T1kDevBuf bWhitelist;
  const uint8_t *whitelist = nullptr;
  bool rawKept = false;             // rows = the raw fragment assignment lists (analyzer)
  // coalescing results (device)
  T1kDevBuf bWork, bGroupPtr, bGroupEnt, bGroupFirst;
  uint64_t nGroups = 0, nEntries = 0, nAssigned = 0;
  bool coalesced = false;
  hipStream_t copyStream = nullptr; // t1k_rowset_assigned_range: copies beside the pipelines (non-blocking stream)
  std::string err;
};
// ---- small host helpers of the device stages (beside t1k_ensure, t1k_dev.h) ----
// offsets of the pieces of one device block, in the order asked for: every piece starts 256-byte aligned and has 256 bytes behind it;
// `off` ends as the size of the block
struct T1kCarve {
  size_t off = 0;
  size_t operator()(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256 + 256; return o; }
};
// a device block that lives for one call.  On every return: the stream drained first, so that no launch of the call still uses the
// block the pool hands out again
struct T1kCallBlock {
  T1kDevBuf buf;
  hipStream_t stream = nullptr;
  T1kCallBlock() = default;
  T1kCallBlock(const T1kCallBlock &) = delete;
  T1kCallBlock &operator=(const T1kCallBlock &) = delete;
  int alloc(t1k_ctx *ctx, size_t bytes) { stream = ctx->stream; return t1k_ensure(ctx, buf, bytes); }
  ~T1kCallBlock() {
    if (!buf.p) return;
    (void)hipStreamSynchronize(stream);
    (void)t1k_dev_free(buf.p);
  }
};
// workgroups of a grid-stride launch over `items`, perBlock of them per workgroup and pass: enough for all, at most blocksPerCu per CU, at least one
inline unsigned t1k_grid(t1k_ctx *ctx, uint64_t items, uint32_t perBlock, uint32_t blocksPerCu = 16) {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * blocksPerCu, (items + perBlock - 1) / perBlock));
}
// read groups as a CSR handed to a stateless call (t1k_alt_batch, t1k_diplo_batch).
// t1k_parallel_check: fn(begin, end) over contiguous pieces of [0, n) on up to 16 host threads; the first non-empty message wins.
template <class F>
std::string t1k_parallel_check(uint64_t n, F fn) {
  unsigned T = std::thread::hardware_concurrency();
  if (T > 16) T = 16;
  if (T < 2 || n < (1ull << 16)) return fn((uint64_t)0, n);
  std::vector<std::string> msg(T);
  std::vector<std::thread> th;
  const uint64_t per = (n + T - 1) / T;
  for (unsigned t = 0; t < T; ++t) th.emplace_back([&, t] { msg[t] = fn(std::min(n, t * per), std::min(n, (t + 1) * per)); });
  for (auto &x : th) x.join();
  for (auto &m : msg) if (!m.empty()) return m;
  return std::string();
}
// t1k_group_pieces: the entries go up in pieces of pieceEntries (the environment variable `env`, in entries, overrides it) cut at group
// boundaries; a group longer than a piece is a piece of its own.  -> the group index where each piece begins, then nGroups
inline std::vector<uint64_t> t1k_group_pieces(uint64_t nGroups, const uint64_t *groupPtr, uint64_t pieceEntries, const char *env) {
  if (const char *e = getenv(env)) { const long long v = atoll(e); if (v > 0) pieceEntries = (uint64_t)v; }
  std::vector<uint64_t> cut{0};
  for (uint64_t g = 0; g < nGroups;) {
    uint64_t h = g + 1;
    while (h < nGroups && groupPtr[h + 1] - groupPtr[g] <= pieceEntries) ++h;
    cut.push_back(h);
    g = h;
  }
  return cut;
}

inline int t1k_bits(unsigned long long v) {  // bits that hold every value <= v (at least 1)
  int b = 1;
  while (b < 64 && (v >> b)) ++b;
  return b;
}

int t1k_rowset_chunk(t1k_rowset *rs, t1k_ctx *ctx, size_t *chunk, t1k_row_entry **rows, uint64_t *cap, unsigned long long **cursor);
int t1k_rowset_chunk_full(t1k_rowset *rs, t1k_ctx *ctx, size_t chunk);
int t1k_exclusive_sum64(t1k_ctx *ctx, const uint32_t *in, unsigned long long *out, uint32_t n);
int t1k_exclusive_sum32(t1k_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n);
int t1k_exclusive_sum_u64(t1k_ctx *ctx, const unsigned long long *in, unsigned long long *out, uint64_t n);

int t1k_launch_pack(t1k_ctx *ctx, const char *dAscii, const uint64_t *dOffs, uint32_t n, int S, uint64_t *bases, uint64_t *nmask, uint16_t *lens, int nCode);
size_t t1k_slow_per_thread(int maxCells);
size_t t1k_chain_big_scratch_u32();
int t1k_chain_max_chunks(uint32_t nAlleles);
int t1k_chain_memo_entries();
int t1k_chain_rec_stride(int maxLen);
int t1k_chain_max_kmers(int maxLen, int k);
int t1k_chain_used_u32(int maxK);
int t1k_launch_seed(t1k_ctx *ctx, const ChainArgs &a, bool longReads, bool xlong);  // t1k_seed.hip: k_seed_groups (+ k_seed_long when xlong)
int t1k_run_chain(t1k_ctx *ctx, const ChainArgs &a, int nWg, int bigBlocks, bool longReads, unsigned long long *hc);
void t1k_launch_extend(t1k_ctx *ctx, const ExtendArgs &a);
void t1k_launch_select(t1k_ctx *ctx, const SelectArgs &a, int nWg, bool packed);
void t1k_launch_fullalign(t1k_ctx *ctx, const FullArgs &a);
void t1k_launch_fullalign_slow(t1k_ctx *ctx, const SlowArgs &a, int nBlocks);
void t1k_launch_align_flags(t1k_ctx *ctx, const SlowArgs &a, uint32_t *flags);
void t1k_launch_align_reps(t1k_ctx *ctx, const uint32_t *flags, const uint32_t *runOf, uint32_t *rep, uint32_t n);
void t1k_launch_align_fill_apply(t1k_ctx *ctx, const SlowArgs &a, bool eq);
int t1k_inclusive_sum(t1k_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n);
void t1k_launch_truncate(t1k_ctx *ctx, const TruncArgs &a, int nWg);
void t1k_launch_coverage_scan(t1k_ctx *ctx, const T1kRefDev &ref, int32_t *out, const uint64_t *outOff);
int t1k_fetch_counters(t1k_ctx *ctx, unsigned long long *h);
// near-best full alignments of nOvl working records (t1k_capi.hip): relaxed counts + (unless noCov) per-base coverage
int t1k_fullalign_phase(t1k_ctx *ctx, const T1kReadsDev &rd, T1kOvl *ovl, uint64_t nOvl, int relaxFlag, int noCov, int maxLen, bool exactQueues, unsigned long long *hc);
struct T1kArenaCounts { uint64_t total; uint32_t maxSeg; bool overflow; };
T1kArenaCounts t1k_arena_counts(const t1k_ctx *ctx, int arena, uint32_t segCap);  // from the last t1k_fetch_counters
void t1k_launch_coverage_add(t1k_ctx *ctx, int32_t *dst, int32_t *src, uint64_t n);
int t1k_coverage_fold(t1k_ctx *ctx);  // covFull -> covDiff (on the context's stream, not synchronised)
void t1k_launch_missing_coverage(t1k_ctx *ctx, const T1kRefDev &ref, int32_t *scratch, int32_t *missing);
// device-driven launches (t1k_run_chain, t1k_assign_range): item counts read on the device from the arena's total word, grids from estimates
void t1k_arena_compact_dev(t1k_ctx *ctx, int arena, const uint32_t *src, uint32_t segCap, uint32_t *dst, uint64_t estTotal);
void t1k_launch_dp_dense_dev(t1k_ctx *ctx, const ChainArgs &a, const uint32_t *jobs, int arena, uint32_t cap, uint64_t est);
uint64_t t1k_arena_estimate(const t1k_ctx *ctx, int arena, uint64_t cap, uint32_t nRe);
void t1k_arena_estimate_set(t1k_ctx *ctx, int arena, uint64_t total, uint32_t nRe);
void t1k_launch_extend_retry_dev(t1k_ctx *ctx, const ExtendArgs &a, const uint32_t *list, int arena, uint64_t est);
void t1k_arena_compact64(t1k_ctx *ctx, int arena, const unsigned long long *src, uint32_t segCap, unsigned long long *dst, uint32_t maxSeg);
// keys[0 .. n) ascending -> runStart[0 .. runs] (runStart[runs] = n), runKey[0 .. runs), *runs on the host (one small copy back, stream
// synchronised).  flag and scan are scratch of n + 1 words each (left as: flag[i] = position i starts a run, scan[i] = runs in front
// of position i).  lone (or NULL): a key equal to *lone never joins a run.
int t1k_run_table(t1k_ctx *ctx, const unsigned long long *keys, uint32_t n, const unsigned long long *lone,
                  uint32_t *flag, uint32_t *scan, uint32_t *runStart, unsigned long long *runKey, uint32_t *runs);
int t1k_sort_pairs(t1k_ctx *ctx, const unsigned long long *keysIn, unsigned long long *keysOut, const uint32_t *valsIn, uint32_t *valsOut, uint32_t n, int endBit = 64);
void t1k_arena_compact(t1k_ctx *ctx, int arena, const uint32_t *src, uint32_t segCap, uint32_t *dst, uint32_t maxSeg);

// t1k_extract.hip
void t1k_launch_extract(t1k_ctx *ctx, const T1kRefDev &ref, const T1kReadsDev &reads, int k, int radius, int hitLenRequired, double oneMinusSim, uint32_t nFragments,
                        uint32_t epf, uint32_t maxK, uint8_t *good, uint8_t *state, unsigned long long *err, unsigned long long *stats, int nWg);
void t1k_launch_extract_huge(t1k_ctx *ctx, const T1kRefDev &ref, const T1kReadsDev &reads, int k, int radius, int hitLenRequired, double oneMinusSim,
                             uint32_t nFragments, uint32_t epf, uint32_t maxK, uint8_t *good, uint8_t *state, unsigned long long *err, unsigned long long *stats, int nWg,
                             uint32_t *scratch, uint32_t cap);
void t1k_launch_extract_big(t1k_ctx *ctx, const T1kRefDev &ref, const T1kReadsDev &reads, int k, int radius, int hitLenRequired, double oneMinusSim,
                            uint32_t nFragments, uint32_t epf, uint32_t maxK, uint8_t *good, uint8_t *state, unsigned long long *err, unsigned long long *stats, int nWg);
