/* include/t1k_gpu.h -- C ABI of libt1k_gpu.so: the MI355X (gfx950) genotyper hot path of T1K.
 *
 * The reference (mourisl/T1K) has no library/FFI seam for this path: its seam is the `genotyper` process
 * (run-t1k:430,434) and, inside it, the C++ methods listed below.  Each entry point names the reference routine it
 * replaces (paths relative to the reference repository root).  All functions are extern "C", take plain pointers
 * and sizes, return 0 on success or a negative t1k_status, never throw and never exit().  A t1k_ctx owns one GPU
 * (one HIP stream); it is driven by one host thread at a time; different contexts are independent.
 *
 * Layers:
 *   (1) device stage API      t1k_ctx_* / t1k_ref_upload / t1k_reads_upload / t1k_assign_batch / t1k_pair_batch /
 *                             t1k_align_batch / t1k_em_*          -- what a cgo/JNI/ctypes binding would call
 *   (2) whole-stage job API   t1k_job_*  (host C++ around (1): FASTA/FASTQ parsing, packing, group coalescing,
 *                             equivalence classes, allele selection, TSV writers) and t1k_genotyper_main(), the
 *                             argv-compatible replacement of the reference's genotyper main() (Genotyper.cpp:194-738).
 *   (3) diagnostics and tests t1k_route_report_* / t1k_seed_report_* (what a range's kernels decided) and t1k_ref_view_* (the reference
 *                             index as t1k_ref_upload built it, read back slice by slice); none of them changes what a run computes
 */
#ifndef T1K_GPU_H
#define T1K_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  T1K_OK = 0,
  T1K_ERR_ARG = -1,       /* bad argument */
  T1K_ERR_DEVICE = -2,    /* HIP error (message in t1k_last_error) */
  T1K_ERR_CAPACITY = -3,  /* a device arena overflowed; raise the matching t1k_params cap and retry */
  T1K_ERR_IO = -4,        /* file could not be opened / parsed */
  T1K_ERR_STATE = -5,     /* call made in the wrong order */
  T1K_ERR_INTERNAL = -6,  /* an internal invariant did not hold (a bug; results of the call are void) */
  T1K_ERR_COMMITTED = -7  /* a capacity limit was hit after part of the range's per-base coverage had been added: do not retry the range on this
                             context (its coverage is void); run again with smaller ranges */
} t1k_status;

typedef struct t1k_ctx t1k_ctx;
typedef struct t1k_job t1k_job;
typedef struct t1k_rowset t1k_rowset;
typedef struct t1k_comm t1k_comm;

/* Genotyper.cpp:218-229 defaults; SeqSet.hpp:760-772 constants */
typedef struct {
  int32_t kmer_length;          /* 11 (Genotyper.cpp:207) */
  int32_t radius;               /* 10 (SeqSet.hpp:763) */
  int32_t hit_len_required;     /* 31 (SeqSet.hpp:764) */
  double ref_seq_similarity;    /* -s, default 0.8 */
  int32_t relax_intron_align;   /* --relaxIntronAlign */
  int32_t max_assign_cnt;       /* -n, default 2000 */
  /* device arena sizing (0 = defaults).  The *_cap values are LIMITS: what a context allocates follows the demand of its ranges */
  int32_t max_read_len;         /* longest read accepted, default (and most) 1000 */
  int32_t workgroups;           /* persistent workgroups of the per-read-end kernels, default 2048 */
  int64_t group_cap;            /* (read-end, strand, allele) hit groups per batch */
  int64_t cand_cap;             /* candidate records per batch */
  int64_t ovl_cap;              /* overlap records of one t1k_assign_range */
  int64_t row_cap;              /* fragment-row entries per batch */
  int32_t n_base_code;          /* the two bits a non-ACGT base contributes to a k-mer code (the code of a window holding one still decides
                                   whether its neighbour repeats the previous k-mer): 3 in the genotyper (nucToNum, Genotyper.cpp:37-40:
                                   -1 & 3), 0 in fastq-extractor (FastqExtractor.cpp:51-54: 'N' -> 0).  t1k_params_default sets 3. */
  int32_t store_chunk_mb;       /* the overlap store (final overlap lists, resident until the next read upload) grows in chunks of
                                   this many MB (at least one range's worth); default 1536 */
} t1k_params;

void t1k_params_default(t1k_params *p);

/* ---- context ------------------------------------------------------------------------------------------------ */
int t1k_ctx_create(int device, const t1k_params *params, t1k_ctx **out);
void t1k_ctx_destroy(t1k_ctx *ctx);
const char *t1k_last_error(const t1k_ctx *ctx);
int t1k_device_count(void);
int t1k_device_memory(int device, uint64_t *freeBytes, uint64_t *totalBytes); /* free = what the driver reports + the blocks this library keeps cached for reuse (t1k_pool_release hands those back) */

/* ---- reference: SeqSet::InputRefSeq + KmerIndex::BuildIndexFromRead (SeqSet.hpp:906-982, KmerIndex.hpp:107-130) --
 * seqs: nAlleles sequences concatenated as ASCII (ACGT, anything else is treated as N); offsets[nAlleles+1] byte offsets;
 * exon: one byte per base, non-zero = exon position (_validDiff::exon, SeqSet.hpp:638-723).  Packs to 2-bit + masks,
 * builds the direct-address 4^k index (postings in (allele, offset) order with the reference's insert rule).  The context's earlier
 * reference is released first: after an upload that fails (other than on a NULL pointer, the allele count or the total size) the context
 * holds no reference, and the calls that need one say so. */
int t1k_ref_upload(t1k_ctx *ctx, const char *seqs, const uint64_t *offsets, const uint8_t *exon, uint32_t nAlleles);

/* ---- reads: one batch of read-ends resident in HBM -------------------------------------------------------------
 * seqs: nReadEnds ASCII reads concatenated; offsets[nReadEnds+1]; weights[nReadEnds] = multiplicity of the read-end
 * (the run length of identical sequences, Genotyper.cpp:463-480), NULL = all 1. */
int t1k_reads_upload(t1k_ctx *ctx, const char *seqs, const uint64_t *offsets, const uint32_t *weights, uint32_t nReadEnds);
/* The same upload in pieces, for a caller that gathers the text through a small page-locked staging buffer (t1k_pinned_alloc) while
 * earlier pieces are on their way: begin (read-ends, total text bytes, longest read), then pieces of the text (what = 0) and of the
 * offset array (what = 1, nReadEnds + 1 uint64; byteOffset / bytes in bytes of that array) in any order -- each an asynchronous copy
 * on the context's stream, tagged with the staging slot (0..3) it was sent from; t1k_reads_upload_wait(slot) returns once the last
 * piece sent from that slot has left the host buffer, which may then be refilled -- then end (packs the reads; every read-end gets
 * weight 1).  What Genotyper.cpp:451-480 does when it collects the read-ends of a run. */
int t1k_reads_upload_begin(t1k_ctx *ctx, uint32_t nReadEnds, uint64_t textBytes, int maxReadLen);
int t1k_reads_upload_piece(t1k_ctx *ctx, int what, const void *src, uint64_t byteOffset, uint64_t bytes, int slot);
int t1k_reads_upload_wait(t1k_ctx *ctx, int slot);
int t1k_reads_upload_end(t1k_ctx *ctx);

/* Identical read-ends collapse onto one representative whose weight is the sum of theirs: the sort + run-length loop of
 * Genotyper.cpp:451-480 (AssignRead is called once per distinct sequence with weight = multiplicity; the weight only feeds the
 * per-base coverage, SeqSet.hpp:2253-2274).  After the call the context's read set is the nDistinct distinct sequences (all
 * later read-end indices -- t1k_assign_range, t1k_pair_batch, t1k_pair_into -- refer to it) and distinctOf[i] is the index of
 * uploaded read-end i's sequence in it.  distinctOf: host array of the uploaded size. */
int t1k_reads_dedupe(t1k_ctx *ctx, uint32_t *distinctOf, uint32_t *nDistinct);

/* One overlap of a read-end on an allele: SeqSet::_overlap (SeqSet.hpp:89-144) after AssignRead. 48 bytes. */
typedef struct {
  int32_t seq_idx, read_start, read_end, seq_start, seq_end, strand;
  int32_t match_cnt, left_clip, right_clip, relaxed_match_cnt;
  double similarity;
} t1k_overlap;

/* SeqSet::AssignRead for every read-end of the uploaded batch (SeqSet.hpp:2119-2303: GetHitsFromRead 1071,
 * GetOverlapsFromHits 1232, GetOverlapsFromRead 1594, ExtendOverlap 1994, near-best GlobalAlignment + base coverage
 * 2188-2285).  Results stay on the device; per-base coverage accumulates in the context. */
int t1k_assign_batch(t1k_ctx *ctx);
/* the same for the sub-range [first, first+count) of the read set.  The final overlap lists of every read-end assigned since
 * the read set was uploaded stay resident (the "overlap store", grown in chunks of store_chunk_mb) and are
 * published in a table shared by all contexts that alias the read set (t1k_reads_share / t1k_reads_attach): mate pairing finds
 * both mates' lists whichever call, on whichever context, produced them.  t1k_overlaps_download returns the lists of the last
 * call only (its read-end indices are relative to `first`). */
int t1k_assign_range(t1k_ctx *ctx, uint64_t first, uint32_t count);
/* copy the overlap lists out (tests / --outputReadAssignment): counts[nReadEnds]; ovl may be NULL to query the total */
int t1k_overlaps_download(t1k_ctx *ctx, uint32_t *counts, t1k_overlap *ovl, uint64_t cap, uint64_t *total);

/* TEST-ONLY: overlap lists made by the host instead of t1k_assign_range's, so that mate pairing can be checked on lists a test
 * constructed.  counts[nReadEnds] for the context's own uploaded read set (whose text is irrelevant to pairing), ovl = the lists one
 * after the other (`similarity` is not stored: pairing recomputes it from the other fields).  T1K_ERR_ARG if a record lies outside its
 * allele or does not fit the packed form of the overlap store. */
int t1k_overlaps_upload(t1k_ctx *ctx, const uint32_t *counts, const t1k_overlap *ovl);
/* TEST-ONLY: the sizes at which the pairing kernel changes its route: out[0] = overlaps of both mates the in-LDS join table takes (more:
 * the per-workgroup tables in device memory), out[1] = overlaps of both mates the first launch takes (more: the second launch),
 * out[2] = row entries per tile of the rowset form's rank sort, out[3] = list records per round of the streamed passes. */
void t1k_pair_limits(uint32_t out[4]);
/* TEST-ONLY: the allele numbers (largest - smallest + 1) the two lists of a fragment may span to be joined through the in-LDS table
 * indexed by allele offset when they hold more than out[0] of t1k_pair_limits together (shorter ones: the hash table); wider fragments
 * take the device-memory tables.  T1K_PAIR_DIRECT=0 turns the route off. */
uint32_t t1k_pair_direct_cap(void);

/* One kept (fragment, allele) assignment: Genotyper::_readAssignment (Genotyper.hpp:44-56). 24 bytes. */
typedef struct {
  int32_t allele_idx, start, end;
  float weight, qual, adjust_weight;
} t1k_row_entry;

/* SeqSet::ReadAssignmentToFragmentAssignment + Genotyper::SetReadAssignments for nFragments fragments
 * (SeqSet.hpp:2310-2655, Genotyper.hpp:778-832).  end1[i]/end2[i] index the context's read set (after t1k_reads_dedupe: the
 * distinct sequences; end2 NULL = single-end run, "-u"); both read-ends must have been assigned since the upload;
 * hasN[i] != 0 if either mate contains an N (Genotyper.cpp:537-539).  Rows stay on the device, in the reference's row order. */
int t1k_pair_batch(t1k_ctx *ctx, const uint32_t *end1, const uint32_t *end2, const uint8_t *hasN, uint32_t nFragments);
/* rowCounts[nFragments]; fragAssigned[nFragments] = fragmentAssigned flag (Genotyper.cpp:564-565) */
int t1k_rows_download(t1k_ctx *ctx, uint32_t *rowCounts, uint8_t *fragAssigned, t1k_row_entry *rows, uint64_t cap, uint64_t *total);

/* ---- all fragment rows of a job, resident on one GPU, and Genotyper::CoalesceReadAssignments over them ------------------------
 * (Genotyper.hpp:841-908).  t1k_pair_into is t1k_pair_batch writing fragment i's row as fragment fragBase + i of the rowset, ordered
 * by allele index (the order of a coalesced group's entries, 847-853), alleles outside the whitelist left out (822-823); several
 * contexts of one GPU may append concurrently.  t1k_rowset_coalesce then folds all fragments into read groups in fragment order:
 * groups numbered by first appearance, start = min, the `end` rule of 893-894 and the float weight sums evaluated in exactly the
 * reference's order (bit-identical, whatever the batching).  Results: groupPtr[nGroups + 1] into entries[nEntries];
 * firstFragment[nGroups] = the fragment that opened each group. */
typedef struct {
  int32_t allele, start, end;
  float weight, adjust_weight;
} t1k_group_entry;
int t1k_rowset_create(t1k_ctx *owner, uint64_t nFragments, const uint8_t *whitelist /* [nAlleles] or NULL */, t1k_rowset **out);
/* A rowset made for an upper bound of the fragment count (an input that is still being inflated when the job starts, t1k_reads_open_stream):
 * the fragments that turned out to exist.  No counterpart in the reference, whose vectors grow (Genotyper.cpp:365-440). */
int t1k_rowset_trim(t1k_rowset *rs, uint64_t n_fragments);
void t1k_rowset_destroy(t1k_rowset *rs);
/* raw != 0: t1k_pair_into stores the fragment assignment list itself (SeqSet::ReadAssignmentToFragmentAssignment's result) without the
 * -n / separator / whitelist drops of SetReadAssignments -- what the analyzer's BarcodeSummary::AddFragment reads (BarcodeSummary.hpp:24-57) */
int t1k_rowset_set_raw(t1k_rowset *rs, int raw);
/* device memory the row chunks hold so far and (rowEntries, may be NULL) the row entries written so far: the job layer projects the whole
 * job's rows from them when it decides which windows keep their read sets */
int t1k_rowset_device_bytes(t1k_rowset *rs, uint64_t *bytes, uint64_t *rowEntries);
const char *t1k_rowset_last_error(const t1k_rowset *rs);
int t1k_pair_into(t1k_ctx *ctx, t1k_rowset *rs, const uint32_t *end1, const uint32_t *end2, const uint8_t *hasN, uint32_t nFragments, uint64_t fragBase);
int t1k_rowset_coalesce(t1k_rowset *rs, uint64_t *nGroups, uint64_t *nEntries, uint64_t *assignedFragments);
/* the same; `sized` (may be NULL) is called once with the number of groups and entries as soon as they are known -- the fold of the
 * groups (the longest step) is then still running on the device, so a caller can size its host tables beside it.  Not called when no
 * fragment has a row. */
int t1k_rowset_coalesce_sized(t1k_rowset *rs, uint64_t *nGroups, uint64_t *nEntries, uint64_t *assignedFragments, void (*sized)(uint64_t nGroups, uint64_t nEntries, void *user), void *user);
int t1k_rowset_groups_download(t1k_rowset *rs, uint64_t *groupPtr, t1k_group_entry *entries, uint32_t *firstFragment);
/* fragAssigned[nFragments]: Genotyper.cpp:564-565 */
int t1k_rowset_assigned_download(t1k_rowset *rs, uint8_t *fragAssigned);
/* the flags of fragments [first, first + count), callable while t1k_pair_into calls for later fragments are in flight (the job's
 * output writer follows the windows of the device loop with it) */
int t1k_rowset_assigned_range(t1k_rowset *rs, uint64_t first, uint64_t count, uint8_t *fragAssigned);
/* rows of fragments [first, first + count) in the reference's row order (--outputReadAssignment, tests) */
int t1k_rowset_rows_download(t1k_rowset *rs, uint64_t first, uint32_t count, uint32_t *rowCounts, t1k_row_entry *rows, uint64_t cap, uint64_t *total);
/* TEST-ONLY: the sizes at which t1k_rowset_coalesce's fold changes its route: out[0] = rows per batch of the pipelined loops, out[1] = the
 * run length (fragments of a group) from which this process folds a group with the four-wavefront kernel (4096, or T1K_CO_LONG_RUN as the
 * library read it), out[2] = slots (entries of a group) per tile. */
void t1k_coalesce_limits(uint32_t out[3]);

/* ---- multi-GPU: one rank per GPU, each owning a contiguous slice of the fragments in file order -------------------
 * Ranks are processes (one per GPU, e.g. under torch.distributed.run: rank 0 calls t1k_comm_unique_id and hands the 128 bytes to
 * the others) or threads of one process (t1k_comm_group_create: `genotyper --gpus N`).  Transport: RCCL over xGMI (librccl.so.1,
 * bound lazily); ranks of one process that share a device use an in-process transport (transport = 0, or automatically): that is
 * how the multi-rank path is tested on one GPU.
 *   t1k_comm_allreduce            in-place sum over the ranks (kind 0: int32 -- the coverage arrays; 1: f64 -- the EM contributions)
 *   t1k_rowset_exchange           every fragment row goes to the rank that owns its pattern (hash mod nRanks); that rank coalesces the
 *                                 group over ALL its fragments in global order, so group contents do not depend on the sharding
 *   t1k_rowset_groups_gather      every rank's group table on every rank; merged by first fragment on the host (the job layer)
 *   t1k_em_shard                  t1k_em_update runs the row pass (one sum per read group) on [rowBegin, rowEnd) only (collective: the
 *                                 ranks' ranges must partition the read groups in rank order), all-gathers the ranks' pieces of the
 *                                 per-group sums (every element has one writer: nothing is added, 8 B per read group in all), then the
 *                                 class pass everywhere in group order: same doubles as on one GPU */
typedef struct t1k_comm_group t1k_comm_group;
int t1k_comm_unique_id(void *id128);
t1k_comm_group *t1k_comm_group_create(int nRanks);
void t1k_comm_group_destroy(t1k_comm_group *g);
int t1k_comm_init(t1k_ctx *ctx, int nRanks, int rank, const void *id128, t1k_comm_group *group, int transport /* -1 auto, 0 in-process, 1 RCCL */, t1k_comm **out);
int t1k_comm_bind(t1k_comm *c, t1k_ctx *ctx);  /* use the communicator with another context of the same device */
/* a rank that cannot go on says so before it returns: ranks waiting for it are released and every later collective of the job fails
 * with T1K_ERR_STATE instead of waiting (in-process transport: the meeting points; RCCL: ncclCommAbort) */
int t1k_comm_abort(t1k_comm *c);
void t1k_comm_destroy(t1k_comm *c);
const char *t1k_comm_last_error(const t1k_comm *c);
int t1k_comm_rank(const t1k_comm *c);
int t1k_comm_size(const t1k_comm *c);
int t1k_comm_is_rccl(const t1k_comm *c);
int t1k_comm_allreduce(t1k_comm *c, void *dev, uint64_t count, int kind);
int t1k_comm_allgather_u64(t1k_comm *c, const uint64_t *mine, uint32_t k, uint64_t *all);
int t1k_comm_alltoallv(t1k_comm *c, const void *sendbuf, const uint64_t *sendOff, void *recvbuf, const uint64_t *recvOff);
int t1k_comm_allgatherv(t1k_comm *c, const void *mine, const uint64_t *bytes, const uint64_t *displ, void *out);
int t1k_comm_allgatherv_host(t1k_comm *c, void *host, const uint64_t *bytes, const uint64_t *displ, uint64_t total);
int t1k_rowset_exchange(t1k_rowset *rs, t1k_comm *comm, uint64_t fragBase);
int t1k_rowset_groups_gather(t1k_rowset *rs, t1k_comm *comm, uint64_t *totalGroups, uint64_t *totalEntries, uint64_t *totalAssigned);
int t1k_rowset_groups_download_all(t1k_rowset *rs, uint32_t *sizes, t1k_group_entry *entries, uint32_t *firstFragment);
int t1k_em_shard(t1k_ctx *ctx, uint32_t rowBegin, uint32_t rowEnd, t1k_comm *comm);

/* per-base coverage of each allele's own base (posWeight[pos].count[base], SeqSet.hpp:2253-2274, read back by
 * GetSeqMissingBaseCoverage 2717-2755).  out[sum of allele lengths], alleles concatenated in upload order. */
int t1k_coverage_get(t1k_ctx *ctx, int32_t *out, uint64_t cap);
int t1k_coverage_reset(t1k_ctx *ctx);
/* per allele: number of exon positions whose coverage is below max(1, 1 % of the allele's median exon coverage)
 * (SeqSet::GetSeqMissingBaseCoverage, SeqSet.hpp:2717-2755), computed on the device; missing[nAlleles] */
int t1k_missing_coverage(t1k_ctx *ctx, int32_t *missing);
/* ---- per-base coverage only where it is read ------------------------------------------------------------------------------------
 * posWeight (SeqSet.hpp:2253-2274) has one reader, GetSeqMissingBaseCoverage (2717-2755) via Genotyper::FinalizeReadAssignments
 * (Genotyper.hpp:935), and alleleInfo[].missingCoverage is consumed for the SELECTED alleles of a gene only (Genotyper.hpp:1754,
 * 1870-1878; its use in EMupdate is overwritten by `adjust = 1`, 389-390 / 400-401).  A context in deferred mode
 * (t1k_ctx_set_coverage_mode(ctx, 1)) therefore adds no coverage in t1k_assign_range -- without --relaxIntronAlign it skips the
 * near-best full alignments altogether (relaxedMatchCnt = matchCnt there, SeqSet.hpp:2247-2250), with it they run for the relaxed
 * counts alone.  The caller keeps the finished read sets instead of letting the next upload overwrite them:
 *   t1k_readset_detach(reader)        the distinct read-ends of the reader context and the table of their final lists change owner
 *   t1k_readset_take_store(rs, pipe)  ... and so do the overlap-store chunks of slot `slot` of every context that assigned ranges of it
 * and, once allele selection has its candidates (Genotyper.hpp:1462-1695),
 *   t1k_coverage_selected(ctx, rs, selected[nAlleles])  adds to ctx's coverage arrays what t1k_assign_range would have added for the
 *                                     overlaps on the alleles with selected[a] != 0: identical per-base coverage for those alleles
 * (integer sums), so t1k_missing_coverage returns the same numbers for them.  *nRecords = records aligned (may be NULL). */
typedef struct t1k_readset t1k_readset;
int t1k_ctx_set_coverage_mode(t1k_ctx *ctx, int deferred);
int t1k_readset_detach(t1k_ctx *reader, t1k_readset **out);
int t1k_readset_take_store(t1k_readset *rs, t1k_ctx *pipe, int slot);
uint64_t t1k_readset_bytes(const t1k_readset *rs);   /* device memory the read set holds */
uint32_t t1k_readset_size(const t1k_readset *rs);    /* distinct read-ends */
const char *t1k_readset_last_error(const t1k_readset *rs);
void t1k_readset_destroy(t1k_readset *rs);
int t1k_coverage_selected(t1k_ctx *ctx, t1k_readset *rs, const uint8_t *selected, uint64_t *nRecords);
/* Identical read-ends across the windows of a job (the reference sorts ALL read-ends and assigns each distinct sequence once,
 * Genotyper.cpp:451-480; a window only sees its own).  A table of the sequences assigned in the windows whose lists stay resident:
 *   t1k_xwin_link(x, reader, w, &n)  after t1k_reads_dedupe of window w: its read-ends found in the table are marked (t1k_assign_range
 *                                    skips them), the others are entered; n = how many were found
 *   t1k_xwin_resolve(x, ctx, w)      once every earlier window's assignment ranges are done: the marked read-ends' list-table entries are
 *                                    copied from the windows that hold their lists (before any fragment of w is paired) */
typedef struct t1k_xwin t1k_xwin;
int t1k_xwin_create(t1k_ctx *owner, uint64_t maxReadEnds, uint32_t maxWindows, t1k_xwin **out);
void t1k_xwin_destroy(t1k_xwin *x);
const char *t1k_xwin_last_error(const t1k_xwin *x);
int t1k_xwin_link(t1k_xwin *x, t1k_ctx *reader, uint32_t window, uint32_t *nExternal);
int t1k_xwin_resolve(t1k_xwin *x, t1k_ctx *ctx, uint32_t window);

/* Several contexts on one GPU (pipelines of one job) can share the read-only device data of one of them: dst aliases src's
 * reference (and gets its own, zeroed coverage array) / src's packed reads.  src must outlive dst. */
int t1k_ref_share(t1k_ctx *dst, const t1k_ctx *src);
/* Device memory of the library is pooled per process (a freed block is reused by the next job: fresh VRAM costs ~35 ms per GB of
 * driver zeroing; T1K_POOL_GB bounds what is kept).  This returns every cached block to the driver; result = bytes released. */
uint64_t t1k_pool_release(void);
/* Page-locked host memory from a per-process cache (t1k_pool_release empties it too): what a caller should gather read text into
 * before t1k_reads_upload -- from pageable memory a multi-GB upload is staged by the runtime on the calling thread and other
 * streams' small copies wait behind its pieces.  NULL when the memory cannot be pinned (the caller falls back to malloc).  No
 * counterpart in the reference (host-only program). */
void *t1k_pinned_alloc(uint64_t bytes);
void t1k_pinned_free(void *p);
int t1k_reads_share(t1k_ctx *dst, const t1k_ctx *src);
/* the same with a choice of the overlap-store slot (0 or 1) dst writes its lists to, emptied first if resetStore != 0: a job
 * keeps two read sets (windows of fragments) in flight, so the lists of one stay valid while the next is being assigned */
int t1k_reads_attach(t1k_ctx *dst, const t1k_ctx *src, int storeSlot, int resetStore);
/* adds src's coverage into dst's and clears src's; both contexts must live on the same device and hold the same reference */
int t1k_coverage_absorb(t1k_ctx *dst, t1k_ctx *src);

/* ---- candidate extraction: IsGoodCandidate (FastqExtractor.cpp:113-118) = !IsLowComplexity (FastqExtractor.cpp:89-111) &&
 * SeqSet::HasHitInSet (SeqSet.hpp:1915-1990: GetHitsFromRead 1071, fullest (strand, sequence) bucket 1929-1964, GetOverlapsFromHits 1232
 * with filter 0, mismatch threshold 1974-1979) for every fragment of the uploaded batch.  The context is created with the
 * extractor's parameters (kmer_length = SeqSet::InferKmerLength, hit_len_required as FastqExtractor.cpp:383-416 computes it,
 * ref_seq_similarity = -s) and its reference uploaded with t1k_ref_upload (exon = NULL; SeqSet::InputRefFa 872-904 keeps one
 * sequence per FASTA record).  Read-ends of a fragment are consecutive in the batch (endsPerFragment 1 or 2); the second end is
 * only tested when the first fails (FastqExtractor.cpp:459-464).  good[nReadEnds / endsPerFragment] receives 0 / 1.
 * stats (may be NULL, else 8 words) receives {read-ends screened, index look-ups of the read-ends the screen let through, postings of their
 * used lists, read-ends with a hit, read-ends chained, k_extract_screen ns, k_extract ns (HIP events on the context's stream), 1 if the
 * batch had to be run again in the large LDS shape (a bucket of more than 1024 hits; more than 8192 is T1K_ERR_CAPACITY)}. */
int t1k_extract_batch(t1k_ctx *ctx, uint32_t endsPerFragment, uint8_t *good, uint64_t *stats);

/* ---- AlignAlgo::GlobalAlignment (AlignAlgo.hpp:215-421) as a batch --------------------------------------------
 * job i aligns t = text[tOff[i] .. tOff[i]+tLen[i]) against p = pat[pOff[i] .. +pLen[i]) (ASCII, N = wildcard).
 * Outputs per job: score, number of MATCH / MISMATCH / indel columns (SeqSet::GetAlignStats, SeqSet.hpp:438-455) and,
 * if ops != NULL, the edit string (0 match,1 mismatch,2 insert,3 delete) at ops[opsOff[i]..], length in nOps[i]. */
/* production match-count routine (exact <=3-mismatch fast path + banded forward sweep) on equal-length jobs: nMatch only */
int t1k_align_count_batch(t1k_ctx *ctx, const char *text, const uint32_t *tOff, const char *pat, const uint32_t *pOff, const uint32_t *len, uint32_t nJobs,
                          int32_t *nMatch);
/* the gap alignment of the dense DP phase itself (no fast path), one lane per job, for |tLen - pLen| <= 4: nMatch only.  Job i's text is
 * text[tOff[i] .. + tLen[i]) and lies at position tOff[i] of ONE packed stream made of text[0 .. max(tOff + tLen)) (likewise the patterns), so the
 * caller decides where a window falls against the stream's 32-base words; a text without N is read without its N mask. */
int t1k_gap_count_batch(t1k_ctx *ctx, const char *text, const uint32_t *tOff, const uint32_t *tLen, const char *pat, const uint32_t *pOff,
                        const uint32_t *pLen, uint32_t nJobs, int32_t *nMatch);
int t1k_align_batch(t1k_ctx *ctx, const char *text, const uint32_t *tOff, const uint32_t *tLen, const char *pat, const uint32_t *pOff,
                    const uint32_t *pLen, uint32_t nJobs, int32_t *score, int32_t *nMatch, int32_t *nMismatch, int32_t *nIndel, int8_t *ops,
                    const uint32_t *opsOff, uint32_t *nOps);

/* ---- EM: Genotyper::EMupdate / QuantifyAlleleEquivalentClass inner loop (Genotyper.hpp:372-421, 1234-1314) -------
 * CSR over read groups: rowPtr[nGroups+1], ecIdx[nnz] (distinct classes of each group in first-appearance order),
 * count[nGroups] (group read count), ecLen[nEc] (class effective length).  t1k_em_update performs one EMupdate:
 * x1 = EM(x0); returns sum|x1-x0| in *diff and the expected read counts in ecReadCount (all host pointers).
 * The summation order is the reference's (bit-identical doubles).  allreduce (may be NULL) is called on the
 * device-resident partial read-count vector between the E and M steps when the groups are sharded over GPUs. */
typedef void (*t1k_allreduce_fn)(void *dev_f64, uint64_t n, void *user);
int t1k_em_setup(t1k_ctx *ctx, const uint64_t *rowPtr, const uint32_t *ecIdx, const double *count, const int32_t *ecLen, uint32_t nGroups,
                 uint32_t nEc, t1k_allreduce_fn allreduce, void *user);
int t1k_em_update(t1k_ctx *ctx, const double *x0, double *x1, double *ecReadCount, double *diff);
/* TEST-ONLY: the step sizes of t1k_em_update's ordered sums: out[0] = entries per ordered piece (a read group's row and a class are added
 * one piece at a time, the sum carried from piece to piece), out[1] = entries per step of the class pass (the unit of its prefetches). */
void t1k_em_limits(uint32_t out[2]);
/* Replaces count[nGroups] of the structure t1k_em_setup left on the context (host pointer); nothing else of it changes.  The serial
 * bootstrap (T1K_BOOTSTRAP_SERIAL=1) runs every replicate through this and t1k_em_update. */
int t1k_em_set_count(t1k_ctx *ctx, const double *count);

/* ---- bootstrap of the EM (genotyper --bootstrap; no counterpart in the reference) ------------------------------------------
 * Poisson bootstrap of the read groups of the structure t1k_em_setup left on the context, which is read in place and not changed.  Replicate
 * r = 0 .. nReplicates; replicate 0 is the data.  Group g of count c_g has n_g = max(1, llrint(c_g)) draws: k[g][r] = sum over i < n_g of
 * X(u(seed, r, g, i)), X the Poisson(1) draw of a 64-bit hash (DESIGN §16 gives u and the thresholds of X), and the replicate's count is
 * c'[g][r] = c_g * (double)k / (double)n_g (k = n_g for replicate 0, and for every replicate when identity != 0).  Integer arithmetic only:
 * the same k on every run.  Counts must lie in 0 .. 2^27 (T1K_ERR_CAPACITY).
 * Every per-replicate array of these calls is replicate-minor with stride Rpad = t1k_boot_stride(nReplicates), the replicates padded to a
 * multiple of 64: element (i, r) at [i * Rpad + r].  Padding replicates (r > nReplicates) have k = 0 and may not be active.
 *   t1k_boot_begin     draws k and c' on the device and keeps them there until t1k_boot_end (or the next t1k_boot_begin)
 *   t1k_boot_nonempty  nonEmpty[Rpad]: 1 where some c'[g][r] is not 0 (an EM of a replicate without counts has nothing to estimate)
 *   t1k_boot_counts    TEST-ONLY (and the serial bootstrap): k[nGroups][Rpad], count[nGroups][Rpad]; either may be NULL
 *   t1k_boot_update    one EMupdate of every replicate with active[r] != 0, as t1k_em_update on c'[.][r]: x0, x1, ecReadCount are
 *                      [nEc][Rpad], diff is [Rpad] (host pointers; x1 may not overlap x0).  Bit for bit the doubles t1k_em_update gives
 *                      with c'[.][r] as the counts.  Nothing of an inactive replicate is written, on the device or in the caller's arrays;
 *                      a block of 64 replicates without an active one costs nothing
 *   t1k_boot_limits    TEST-ONLY: out[0] = entries whose operands the row and class passes request ahead of their additions, out[1] = the
 *                      n_g from which the lanes of a wavefront share a replicate's draws, out[2] = replicates per block
 *   t1k_boot_times     device ms of the row passes, of the class passes, and the updates run since t1k_boot_begin */
int t1k_boot_begin(t1k_ctx *ctx, uint32_t nReplicates /* 1 .. 1000 */, uint64_t seed, int identity);
uint32_t t1k_boot_stride(uint32_t nReplicates);
int t1k_boot_nonempty(t1k_ctx *ctx, uint8_t *nonEmpty);
int t1k_boot_counts(t1k_ctx *ctx, uint32_t *k, double *count);
int t1k_boot_update(t1k_ctx *ctx, const uint8_t *active, const double *x0, double *x1, double *ecReadCount, double *diff);
void t1k_boot_end(t1k_ctx *ctx);
void t1k_boot_limits(uint32_t out[3]);
void t1k_boot_times(const t1k_ctx *ctx, double ms3[3]);

/* ---- per-barcode allele EM (analyzer --barcodeEM; no counterpart in the reference; estimator: DESIGN §11) ---------------------
 * One independent EM per barcode, the whole iteration loop in one launch.  Barcode b (of the slice [0, nBarcodes)):
 *   bcAllelePtr[b] .. [b+1]   its alleles U_b in bcAllele[], strictly ascending global ids < nAlleles (the "local" alleles)
 *   bcGroupPtr[b] .. [b+1]    its groups, in the order the EM adds them; groupCount[g] = c_g (finite, > 0)
 *   groupEntryPtr[g] .. [g+1] group g's list S_g in entryLocal[]: strictly ascending indices into U_b, at least one
 * The offsets need not start at 0: a slice of a larger table is passed as the offsets of its barcodes, the other arrays whole.
 * Start theta_a = f_a / N_b (f_a = sum over a's groups of c_g / |S_g|); an update is psum_g = sum_{a in S_g} theta_a,
 * n_a = sum_{g ∋ a} c_g * (theta_a / psum_g), theta'_a = (n_a + alpha * rho[bcAllele]) / (N_b + alpha); it stops after the update
 * whose sum |theta' - theta| < tol, or after maxIter updates.  nOut (laid out as bcAllele, at the same absolute positions) = the n of
 * the last update (all 0 where N_b = 0), itersOut[b] = updates run.  rho may be NULL when alpha == 0.  kernelMs (may be NULL): the
 * kernel's device time.  Barcodes whose state exceeds the per-wave LDS arena -- 4|U_b| + 4G + (G+1) + (|U_b|+1) + 2E four-byte words
 * against 2048, or against T1K_BARCODE_EM_LDS if that is lower -- run the same arithmetic on global memory. */
int t1k_barcode_em(t1k_ctx *ctx, uint32_t nBarcodes, const uint64_t *bcAllelePtr, const uint32_t *bcAllele, const uint64_t *bcGroupPtr,
                   const double *groupCount, const uint64_t *groupEntryPtr, const uint32_t *entryLocal, const double *rho, uint32_t nAlleles,
                   double alpha, double tol, int32_t maxIter, double *nOut, int32_t *itersOut, double *kernelMs);

/* ---- UMI collapse of the per-barcode allele lists (analyzer --umi) ------------------------------------------
 * Fragment f: row fragRow[f] < nRows of the per-barcode table, the strictly ascending allele list listAllele[listPtr[f] .. listPtr[f+1])
 * (not empty, ids < nAlleles; listPtr may start anywhere: a slice of a larger table) and the UMI word fragUmi[f]: the code in bits 0-31
 * (2 bits per base, A 0 C 1 G 2 T 3, first base most significant), the length 1 - 16 in bits 32-36, or all ones for "no UMI".
 * Its gene is alleleGene[its smallest allele] < nGenes, its bucket (row, gene, length).  With mismatch = 1 a UMI u joins the neighbour v
 * (same bucket, Hamming distance 1) with c(v) >= 2 c(u) - 1 and (c(v) > c(u), or c(v) == c(u) and v < u) that has the largest count,
 * ties to the smallest code; root(u) follows these parents to the end.  mismatch = 0: root(u) = u.  A key = (bucket, root): one molecule
 * with the intersection of its fragments' lists or, when that is empty, one molecule per distinct list among them; a fragment without a
 * UMI is a molecule of its own.
 * Outputs, sized by the caller: fragMol[nFrag]; *nMol <= nFrag molecules in no particular order with molRow, molFrags (fragments
 * behind each), molListPtr[*nMol + 1] (starting at 0) into molList (at most listPtr[nFrag] - listPtr[0] entries); the dense tables
 * frac[nRows * nAlleles] = sum over ascending n of (double)K(r, a, n) / (double)n and uniq = K(r, a, 1), K(r, a, n) = the row's molecules
 * of n alleles that hold a.  stats may be NULL.  Negative codes: mismatch not 0 / 1, a row, allele, gene, UMI word or offset out of
 * range, a list not ascending, nRows * nGenes >= 2^28 (the 64-bit sort key holds 28 bits of row and gene, 4 of length, 32 of code),
 * nRows * nAlleles >= 2^40 or not fitting 64 bits beside the longest list's length (the table's sort key), 2^31 fragments, 2^32 entries. */
typedef struct {
  uint64_t distinct;   /* distinct (bucket, UMI) */
  uint64_t keys;       /* distinct (bucket, root) */
  uint64_t corrected;  /* distinct UMIs that joined a neighbour */
  uint64_t split;      /* keys with an empty intersection */
  uint64_t no_umi;     /* fragments without a UMI */
  double kernel_ms;    /* device time from the first kernel to the last (the sizes read back in between included) */
} t1k_umi_stats;
int t1k_umi_collapse(t1k_ctx *ctx, uint32_t nFrag, const uint32_t *fragRow, const uint64_t *fragUmi, const uint64_t *listPtr, const uint32_t *listAllele,
                     uint32_t nRows, const uint32_t *alleleGene, uint32_t nAlleles, uint32_t nGenes, int32_t mismatch, uint32_t *fragMol, uint32_t *nMol,
                     uint32_t *molRow, uint32_t *molFrags, uint64_t *molListPtr, uint32_t *molList, double *frac, int32_t *uniq, t1k_umi_stats *stats);

/* ---- per-base pileup of alignments onto alleles (analyzer --pileup) ---------------------------------------------
 * A table of 14 int32 counters per allele position lives on the context between t1k_pileup_begin and t1k_pileup_end.  It is
 * COUNTER-MAJOR: with T = alleleOff[nAlleles], counter c of position p of allele a is counts[c * T + alleleOff[a] + p]; c = 0 .. 6 are
 * A C G T N del ins weighted by w_all, c = 7 .. 13 the same seven weighted by w_uniq.  alleleOff[0] = 0, ascending.
 * One record = one alignment: its edit string ops[ops_at .. ops_at + n_ops) (0 match, 1 mismatch, 2 insert, 3 delete) is walked from
 * allele position seq_start and from text[read_at] (the first base of the read window, strand-corrected; a byte that is not A/C/G/T
 * counts as N).  Ops 0 and 1 book the read base at the allele position and advance both; 3 books del and advances the allele; 2 books
 * ins at the allele position consumed last before it (seq_start if none yet; clamped to the allele's last position) and advances the
 * read.  Every booking adds w_all to the first seven counters' cell and w_uniq (<= w_all) to the second seven's.
 * t1k_pileup_add may be called any number of times; text / ops are the call's own.  It books nothing unless the whole call is sound:
 * T1K_ERR_ARG for an allele >= nAlleles, w_uniq > w_all, an op outside 0 .. 3, a walk that leaves the allele, `text` or `ops`;
 * T1K_ERR_CAPACITY when the bookings on one allele (the sum of w_all * n_ops over the table's life) could carry a counter past
 * 2^31 - 1; T1K_ERR_STATE for add / get / end without begin, or begin while a table is open.  kernelMs (may be NULL): device time of
 * the call's kernels.  t1k_pileup_get copies the 14 * T counters out; the table stays open. */
typedef struct {
  uint32_t allele, seq_start;
  uint64_t read_at, ops_at;
  uint32_t n_ops, w_all, w_uniq, reserved;
} t1k_pileup_aln;  /* 40 bytes */
int t1k_pileup_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */);
int t1k_pileup_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const char *text, uint64_t textBytes, const int8_t *ops, uint64_t opsBytes,
                   double *kernelMs);
int t1k_pileup_get(t1k_ctx *ctx, int32_t *counts /* [14 * alleleOff[nAlleles]] */);
int t1k_pileup_end(t1k_ctx *ctx);

/* ---- per-barcode pileup at sites (analyzer --barcodePileup) -------------------------------------------------------
 * What t1k_pileup_* counts, split by barcode and restricted to nSites sites (siteAllele[s], sitePos[s]): strictly ascending by
 * (allele, pos), pos 0-based and < the allele's length (else T1K_ERR_ARG).  The table is sparse: a list of (key, count) runs,
 * key = ((barcode * nSites + site) * 7 + plane) * 2 + (1 - uniq), plane = 0 .. 6 for A C G T N del ins, ascending by key, only cells
 * that received a booking.  A uniq booking is stored once, under uniq = 1 (the even key): the reader adds the even run of a cell to its
 * plain counter as well (plain = even + odd, _uniq = even).  T1K_ERR_CAPACITY from _begin if nBarcodes > 2^31 or nBarcodes * nSites * 14
 * does not fit the key (2^63); nSites = 0 is legal (the table stays empty).
 * t1k_sitepile_add: records as for t1k_pileup_add (w_all / w_uniq are ignored); record i books once per entry of
 * book[bookPtr[i] .. bookPtr[i + 1]), an entry being barcode << 1 | uniq.  Nothing is emitted unless the whole call is sound:
 * T1K_ERR_ARG for an allele >= nAlleles, a barcode >= nBarcodes, a bookPtr that decreases, an op outside 0 .. 3, a walk that leaves its
 * allele, `text` or `ops`; T1K_ERR_CAPACITY when the table and the call's keys exceed 2^31 entries or a counter would pass 2^31 - 1
 * (the table is as before the call); T1K_ERR_STATE for add / get / stats / end without begin, or begin while a table is open.
 * Pending keys are folded into runs whenever they reach 2^28 (env T1K_SITEPILE_PENDING) and at _get.
 * t1k_sitepile_get: *nRuns = the runs; with keys and counts given (cap >= *nRuns entries each) they are copied out -- a size query
 * (keys = NULL) followed by a fill.  The table stays open.  t1k_sitepile_stats: keys emitted and folds so far, device time of the folds. */
int t1k_sitepile_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos,
                       uint64_t nBarcodes);
int t1k_sitepile_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint64_t *bookPtr /* [n + 1] */, const uint32_t *book, const char *text, uint64_t textBytes,
                     const int8_t *ops, uint64_t opsBytes, double *kernelMs);
int t1k_sitepile_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
int t1k_sitepile_stats(t1k_ctx *ctx, uint64_t *keysEmitted, uint64_t *folds, double *foldMs);
int t1k_sitepile_end(t1k_ctx *ctx);

/* ---- read-backed phasing of site pairs (analyzer --phase) -----------------------------------------------------------
 * Which states two sites show on one fragment.  Sites as for t1k_sitepile_begin, at most 2^28 of them (else T1K_ERR_CAPACITY); nSites = 0
 * is legal (the table stays empty).  A record observes a site with the column of its edit string that consumes that allele position:
 * ops 0 and 1 give the read base (state 0 .. 3 for A C G T, 4 = N for anything else), op 3 gives state 5 = del; insert columns observe
 * nothing.  A booking is a fragment-assignment: bookRec[2b] = rec1, bookRec[2b + 1] = rec2, its mate on the same allele, or 0xFFFFFFFF
 * for "no mate", and bookUniq[b] != 0 when its fragment has one assignment.  Its observations are the union of its records': a site both
 * show in the same state counts once, a site they show in different states is dropped for this booking (a discordant site); rec1 == rec2
 * gives that record's own list.  Every unordered pair of a booking's observed sites s < t in states x, y adds 1 to cell (s, t, x, y).
 * The table is sparse: (key, count) runs ascending by key, key = (((s * nSites + t) * 36 + x * 6 + y) << 1) | (1 - uniq).  A uniq booking
 * is stored once, under the even key: the reader forms plain = even + odd, _uniq = even.
 * t1k_phase_add: records as for t1k_pileup_add (w_all / w_uniq are ignored).  Nothing is emitted unless the whole call is sound:
 * T1K_ERR_ARG for an allele >= nAlleles, a record index >= n, mates on different alleles, an op outside 0 .. 3, a walk that leaves its
 * allele, `text` or `ops`; T1K_ERR_CAPACITY when a call holds 2^31 observations or more, or the table and the call's keys exceed 2^31
 * entries -- pairs grow with the square of a booking's observed sites -- or a counter would pass 2^31 - 1 (the table is as before the
 * call); T1K_ERR_STATE for add / get / stats / end without begin, or begin while a table is open.  Pending keys are folded into runs
 * whenever they reach 2^28 (env T1K_PHASE_PENDING) and at _get.
 * t1k_phase_get: as t1k_sitepile_get.  t1k_phase_stats: observations of the records walked, bookings with two observed sites or more,
 * keys emitted, discordant sites and folds so far, device time of the folds. */
int t1k_phase_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos);
int t1k_phase_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, uint32_t nBook, const uint32_t *bookRec /* [2 * nBook] */, const uint8_t *bookUniq /* [nBook] */,
                  const char *text, uint64_t textBytes, const int8_t *ops, uint64_t opsBytes, double *kernelMs);
int t1k_phase_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
int t1k_phase_stats(t1k_ctx *ctx, uint64_t *observations, uint64_t *bookings, uint64_t *keysEmitted, uint64_t *discordant, uint64_t *folds, double *foldMs);
int t1k_phase_end(t1k_ctx *ctx);

/* ---- strand, mate, read-end distance and template support at sites (analyzer --siteSupport) ----------------------------
 * What t1k_pileup_* counts, restricted to sites as for t1k_sitepile_begin (at most 2^28 of them, else T1K_ERR_CAPACITY; nSites = 0 is
 * legal) and split by the evidence behind a booking.  Records as for t1k_pileup_add (w_all / w_uniq / reserved are ignored and stay
 * untouched); rec[i] describes the read-end record i is a window of: its length read_len (1 .. 65535), the bases clip_front in front of
 * the window in the strand-corrected read-end, and strand (0: the read-end lies on the allele's forward strand, 1: reverse).  Record i
 * books once per entry of book[bookPtr[i] .. bookPtr[i + 1]); an entry's flags are bit 0 uniq (its fragment has one assignment), bit 1
 * mate (the read-end comes from file 2), bit 2 orient (of its template), and t_start <= t_end < the allele's length are the template's
 * first and last allele position.
 * A column of state 0 .. 6 (A C G T N del ins) that books at site s, at allele position pos, has c = clip_front + the read bases of the
 * window in front of it and the end distance d = min(c, read_len - 1 - c) where it consumes base c (ops 0, 1, 2), d = min(c, read_len - c)
 * for op 3, which lies between bases c - 1 and c; d is stored saturated at 511.  With every booking the column adds 1 under two keys of ONE
 * sparse table of (key, count) runs, ascending by key:
 *   family A, the support:   ((((s * 7 + state) * 2 + strand) * 2 + mate) * 512 + d) * 2 + (1 - uniq), below 2^57.  A uniq booking is
 *                            stored once, under the even key, as in t1k_sitepile_*: plain = even + odd, _uniq = even;
 *   family B, the templates: 2^57 | (((s * 7 + state) * 2 + orient) << 24) | (dStart << 12) | dEnd with dStart = min(pos - t_start, 4095)
 *                            and dEnd = min(t_end - pos, 4095), each clamped below at 0; below 2^58.  The reader counts the RUNS of a
 *                            (site, state) and ignores their counts: templates that differ only beyond 4095 bases from the site are one.
 * Nothing is emitted unless the whole call is sound: T1K_ERR_ARG for what t1k_sitepile_add refuses (allele, ops, walks, bookPtr), a
 * strand > 1, read_len == 0 or > 65535, a read window that leaves its read (clip_front + the read bases the walk consumes > read_len),
 * flags >= 8, t_start > t_end, t_end >= the length of the record's allele; T1K_ERR_CAPACITY and T1K_ERR_STATE as t1k_sitepile_*.  Pending
 * keys are folded into runs whenever they reach 2^28 (env T1K_SUPPORT_PENDING) and at _get.  t1k_support_get / _stats: as t1k_sitepile_get /
 * _stats. */
typedef struct { uint32_t read_len, clip_front, strand; } t1k_support_rec;   /* per record; strand: 0 forward, 1 reverse */
typedef struct { uint32_t flags, t_start, t_end; } t1k_support_book;         /* per booking; flags: bit 0 uniq, bit 1 mate (file 2), bit 2 orient */
int t1k_support_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */, uint64_t nSites, const uint32_t *siteAllele, const uint32_t *sitePos);
int t1k_support_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const t1k_support_rec *rec /* [n] */, const uint64_t *bookPtr /* [n + 1] */,
                    const t1k_support_book *book, const char *text, uint64_t textBytes, const int8_t *ops, uint64_t opsBytes, double *kernelMs);
int t1k_support_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
int t1k_support_stats(t1k_ctx *ctx, uint64_t *keysEmitted, uint64_t *folds, double *foldMs);
int t1k_support_end(t1k_ctx *ctx);

/* ---- novel indel evidence per allele, left-aligned (analyzer --indels) -------------------------------------------------
 * The gap runs of the edit strings t1k_pileup_* counts column by column, taken as events.  alleleText holds the alleles' bases back to
 * back (A C G T N only, else T1K_ERR_ARG), allele a at alleleText[alleleOff[a] .. alleleOff[a + 1]).  Records as for t1k_pileup_add
 * (w_all / w_uniq / reserved are ignored and stay untouched); strand[i]: 0 when record i lies on the allele's forward strand, 1 on the
 * reverse.  Record i books once per entry of bookUniq[bookPtr[i] .. bookPtr[i + 1]) -- one per assignment overlap that points at it; the
 * entry is 1 when the overlap's fragment has a single assignment, else 0.
 * An event is a maximal run of columns of one gap op (3 deletion, 2 insertion) that holds neither the first nor the last column of its
 * edit string.  A run that does is an EDGE run: no event, its columns are only counted (edgeDelBooked / edgeInsBooked).  An insertion run
 * and a deletion run that touch are two events.  A deletion of L allele bases from p (0-based) on is (DEL, p, L); read bases S (L of them,
 * as `text` holds them, anything but A/C/G/T taken as N) in front of allele base p are (INS, p, L, S).  Every event is left-normalised
 * against the allele's bases alone, an N equal to nothing, itself included, with no bound but p == 0:
 *   DEL: while p > 0 and allele[p-1] == allele[p+L-1]: p -= 1
 *   INS: while p > 0 and allele[p-1] == S[-1]: S = allele[p-1] + S[:-1]; p -= 1
 * With every booking the event adds 1 under one key of ONE sparse table of (key, count) runs, ascending by key, every key below 2^63:
 *   ((((g << 2 | type) << 27 | payload) << 1 | strand) << 1) | (1 - uniq),  g = alleleOff[allele] + p after normalisation;
 *   type 0: a deletion, payload L (a deletion of 2^27 bases or more: T1K_ERR_CAPACITY);
 *   type 1: a short insertion -- L <= 13 and every base of the normalised S one of ACGT -- payload (1 << 2L) | the bases, 2 bits each
 *           (A 0, C 1, G 2, T 3), the first base highest;
 *   type 2: a long insertion -- L > 13, or an N in the normalised S -- payload min(L, 2^27 - 1): LONG INSERTIONS ARE TOLD APART BY
 *           POSITION AND LENGTH ONLY.
 * A uniq booking is stored once, under the even key, as in t1k_sitepile_*: plain = even + odd, _uniq = even.
 * Nothing is emitted unless the whole call is sound, its sound records included: T1K_ERR_ARG for what t1k_sitepile_add refuses (allele,
 * ops, walks, bookPtr), a strand > 1, a bookUniq > 1; T1K_ERR_CAPACITY for 2^31 bookings or more on one record and as t1k_sitepile_*;
 * T1K_ERR_STATE as t1k_sitepile_*.  Pending keys are folded into runs whenever they reach 2^28 (env T1K_INDEL_PENDING) and at _get.
 * t1k_indel_get: as t1k_sitepile_get.  t1k_indel_stats, over the calls that were taken: events -- the events of distinct records,
 * bookings not multiplied in; shifted -- those of them whose position moved under normalisation; edgeDelBooked / edgeInsBooked -- the
 * columns of edge runs x their record's bookings; keysEmitted / folds / foldMs as t1k_sitepile_stats.  All but foldMs are deterministic. */
int t1k_indel_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */, const char *alleleText /* [alleleOff[nAlleles]], ACGTN */);
int t1k_indel_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint8_t *strand /* [n]: 0 / 1 */, const uint64_t *bookPtr /* [n + 1] */, const uint8_t *bookUniq,
                  const char *text, uint64_t textBytes, const int8_t *ops, uint64_t opsBytes, double *kernelMs);
int t1k_indel_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns);
int t1k_indel_stats(t1k_ctx *ctx, uint64_t *events, uint64_t *shifted, uint64_t *edgeDelBooked, uint64_t *edgeInsBooked, uint64_t *keysEmitted, uint64_t *folds, double *foldMs);
int t1k_indel_end(t1k_ctx *ctx);

/* ---- CIGAR, MD:Z and NM:i of alignments (analyzer --sam) -----------------------------------------------------------------
 * Stateless.  Records as for t1k_pileup_add; read_at, w_all and w_uniq are ignored (no read text is read).  alleleText holds the alleles'
 * bases back to back, allele a at alleleText[alleleOff[a] .. alleleOff[a + 1]).  For record i, its edit string walked from allele position
 * seq_start:
 *   cigar[cigarPtr[i] .. cigarPtr[i + 1]): <front>S when clip[2i] > 0, then <length><letter> per maximal run of columns of one class in
 *     column order (ops 0 and 1: M, op 2: I, op 3: D), then <back>S when clip[2i + 1] > 0.  Decimal, no padding, no terminator; runs are
 *     literal (a string that begins or ends with I or D stays so).  clip = NULL: no clips.
 *   md[mdPtr[i] .. mdPtr[i + 1]): the value of MD:Z: as samtools calmd writes it -- a number, then items, each followed by a number.  An
 *     op-1 column is the item <allele base>; a maximal run of op-3 columns that are consecutive in the edit string is ^<allele bases>
 *     (op-2 columns are invisible but end a deletion run: 3 2 3 gives 0^A0^C0); the number is the count of op-0 columns since the item
 *     before, 0 when there are none.  Allele bases are copied as they stand.
 *   nm[i]: the columns with op 1, 2 or 3.  refSpan[i]: the columns with op 0, 1 or 3.
 * cigarPtr[0] = mdPtr[0] = 0; both arenas are packed in record order.  What the caller's arenas have to hold, per record:
 *   CIGAR <= 2 * n_ops + 22 bytes: a run of L columns costs digits(L) + 1 <= L + 1 bytes and there are at most n_ops runs whose lengths
 *     add up to n_ops, 2 * n_ops in all; a clip costs at most 10 digits + S = 11 bytes, and there are two.
 *   MD <= 3 * n_ops + 11 bytes: the most expensive column is a one-column deletion behind no match, 0^C = 3 bytes; a number of d > 1
 *     digits stands for >= 10^(d-1) >= d match columns that cost nothing themselves; the final number has at most 10 digits (11 leaves
 *     one spare).
 * The CIGAR bound is attained: a string whose class alternates every column costs 2 * n_ops, two clips of ten digits 22.  The MD bound is
 * not tight: deletion runs need a column between them, and the dearest such column is a mismatch (0A, 2 bytes), so the worst string
 * alternates ops 3 and 1 at 2.5 * n_ops + 2 bytes; a lone deletion column (0^C0) costs 3 * n_ops + 1.
 * T1K_ERR_ARG: an allele >= nAlleles, n_ops == 0, an op outside 0 .. 3, a string that leaves `ops`, a walk that leaves its allele,
 * alleleOff not starting at 0 or decreasing; T1K_ERR_CAPACITY: an arena too small (the message names it and the bytes it needs).  A
 * failing call leaves every output array as it was.  n == 0: T1K_OK, only cigarPtr[0] and mdPtr[0] are written.  kernelMs (may be
 * NULL): device time from the first kernel to the last. */
int t1k_cigar_batch(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint32_t *clip /* [2 * n]: front, back soft clip of record i; NULL = none */,
                    const int8_t *ops, uint64_t opsBytes, uint32_t nAlleles, const uint64_t *alleleOff /* [nAlleles + 1] */, const char *alleleText /* [alleleOff[nAlleles]] */,
                    uint64_t *cigarPtr /* [n + 1] */, char *cigar, uint64_t cigarCap, uint64_t *mdPtr /* [n + 1] */, char *md, uint64_t mdCap,
                    uint32_t *nm /* [n] */, uint32_t *refSpan /* [n] */, double *kernelMs /* may be NULL */);

/* ---- runner-up evidence per called allele (genotyper --alternatives) ----------------------------------------------------------
 * Stateless; all pointers are host pointers.  The read groups as a CSR: group g holds the alleles entryAllele[groupPtr[g] .. groupPtr[g + 1]),
 * strictly ascending, and weighs q[g] (the job: llrint(count[g] * 2^20), count[g] the group's count in the EM).  alleleGene[a] < nGenes is the
 * gene of allele a; slotOf[a] = 2 * alleleGene[a] + k where a is the allele called in slot k (0 / 1) of its gene, 0xFFFFFFFF for every other
 * allele; a slot belongs to at most one allele.  tables = four arrays of nAlleles sums of q, one after the other, over the groups that hold b:
 *   total[b]    all of them;
 *   both0[b]    those that also hold the allele of slot 0 of b's gene (none when the slot is empty; the called allele itself: its total);
 *   both1[b]    the same for slot 1;
 *   neither[b]  those that hold no called allele of b's gene.
 * The sums are 64-bit integers (global atomic adds): the same bits for every launch shape, piece size and run.  The entries are uploaded in
 * pieces cut at group boundaries, 2^24 entries each (env T1K_ALT_PIECE, in entries, read by every call); a group longer than a piece is a
 * piece of its own.  t1k_alt_pieces: how many pieces a call with this groupPtr makes.
 * Nothing is written unless the whole call is sound.  T1K_ERR_ARG: groupPtr[0] != 0 or a groupPtr that decreases; an entry >= nAlleles; the
 * entries of a group not strictly ascending (a duplicate would count twice); an alleleGene >= nGenes; a slotOf that is neither 0xFFFFFFFF
 * nor 2 * alleleGene[a] + {0, 1}; two alleles with one slotOf; a NULL array that would be read.  T1K_ERR_CAPACITY: the sum of q over all
 * groups -- the bound of every cell -- could reach 2^63; 2^32 groups or more; more than 65536 genes (the slot bitsets of a workgroup, four
 * of 2 * nGenes bits, must fit 64 KB of LDS).  nGroups == 0: T1K_OK, the tables are zeroed.  kernelMs (may be NULL): device time of the
 * pieces' kernels. */
int t1k_alt_batch(t1k_ctx *ctx, uint64_t nGroups, const uint64_t *groupPtr /* [nGroups + 1] */, const uint32_t *entryAllele, const uint64_t *q /* [nGroups] */, uint32_t nAlleles,
                  const uint32_t *alleleGene /* [nAlleles] */, uint32_t nGenes, const uint32_t *slotOf /* [nAlleles] */, uint64_t *tables /* [4 * nAlleles] */, double *kernelMs /* may be NULL */);
uint64_t t1k_alt_pieces(uint64_t nGroups, const uint64_t *groupPtr);

/* ---- co-occurrence of allele-pair candidates (genotyper --diplotypes) ------------------------------------------------------------
 * Stateless; all pointers are host pointers.  The read groups as a CSR over candidate ids: group g holds entryCand[groupPtr[g] ..
 * groupPtr[g + 1]), strictly ascending, and weighs q[g] (as t1k_alt_batch).  Ids are gene-major: gene x owns the ids candPtr[x] ..
 * candPtr[x + 1), n_x of them.  matrix = sum of n_x^2 64-bit cells; the block of gene x begins at the sum of n_y^2 over y < x; cell (i, j)
 * of local ids at i * n_x + j holds, for i <= j, the sum of q over the groups that hold both candidates (the diagonal: the candidate's
 * total); the cells i > j are 0.  The sums are 64-bit integers (global atomic adds): the same bits for every launch shape, piece size and
 * run.  The entries are uploaded in pieces cut at group boundaries, 2^24 entries each (env T1K_DIPLO_PIECE, in entries, read by every
 * call); a group longer than a piece is a piece of its own; the matrix stays on the device across the pieces and is copied out once.
 * t1k_diplo_pieces: how many pieces a call with this groupPtr makes.
 * Every check is made before the first launch and nothing is written unless all of them pass.  T1K_ERR_ARG: groupPtr[0] != 0 or a groupPtr
 * that decreases; candPtr[0] != 0 or a candPtr that decreases; an entry >= candPtr[nGenes]; the entries of a group not strictly ascending;
 * a NULL array that would be read.  T1K_ERR_CAPACITY: a gene with more than 2048 candidates; more than 2^29 cells; the sum of q over all
 * groups -- the bound of every cell -- could reach 2^63; 2^32 groups or more.  nGroups == 0: T1K_OK, the matrix is zeroed.  kernelMs (may
 * be NULL): device time of the pieces' kernels. */
int t1k_diplo_batch(t1k_ctx *ctx, uint64_t nGroups, const uint64_t *groupPtr /* [nGroups + 1] */, const uint32_t *entryCand, const uint64_t *q /* [nGroups] */, uint32_t nGenes,
                    const uint32_t *candPtr /* [nGenes + 1] */, uint64_t *matrix, double *kernelMs /* may be NULL */);
uint64_t t1k_diplo_pieces(uint64_t nGroups, const uint64_t *groupPtr);

/* ---- profiling counters of the last t1k_assign_batch (algorithmic-traffic terms of SURVEY.md 8d) --------------- */
typedef struct {
  uint64_t read_ends, lookups, postings, hits, groups, candidates, extended, near_best, dp_calls, rows, batches;
  /* kernel time (HIP events on the launch stream), summed over the batches of the last run:
     ms_seed = k_seed_groups, ms_chain = the remaining chain kernels, ms_fullalign = k_fullalign + DP kernels + k_truncate (near zero for a
     range whose lists k_select finishes itself: deferred coverage without relax_intron_align); extended = the overlaps the selection
     emitted, before lists of more than 1000 are cut */
  double ms_seed, ms_chain, ms_extend, ms_select, ms_fullalign, ms_pair, ms_em, ms_total;
  /* job level (t1k_job_stats): read_ends above counts the DISTINCT read-ends the kernels ran on, read_ends_total all of them;
     pair_overlaps = overlap records read by mate pairing; dp_cells = cell updates of the traced alignment kernels;
     wall-clock phases of the last run: mapping + indexing the read files, the window loop on the device, coalescing + download,
     writing the output files */
  uint64_t read_ends_total, pair_overlaps, dp_cells;
  double ms_load, ms_device, ms_coalesce, ms_write;
} t1k_stats;
int t1k_stats_get(t1k_ctx *ctx, t1k_stats *out);

/* ---- route report: which kernel chained each group (diagnostics and tests) -----------------------------------------
 * Off by default, and then t1k_assign_range issues exactly the launches and copies it issues without it.  t1k_route_report_enable(ctx, 1)
 * clears the report and starts it; (ctx, 0) stops it and drops what it held.  While it is on, every range that t1k_assign_range
 * finishes adds its totals and one record per multi-diagonal group; a range that ran again after a capacity error counts once, from the
 * pass that was kept.  The records cost one copy of the general list, the big list and the listed group records per range.
 * totals: arena totals of the kept passes (work-list lengths, not kernel launches) and T1K_STAT_FAST; eq / band / wide are the
 * alignment queues of t1k_assign_range's own full alignments (0 with deferred coverage and no relax_intron_align).
 * t1k_route_report_get: *nRecs = the records held; with recs given (cap >= *nRecs) they are copied out, in the order of the ranges. */
enum { T1K_ROUTE_GENERAL_LANE = 0,    /* k_chain_general: n <= 32, or simple and n <= 96 */
       T1K_ROUTE_WAVE_SMALL = 1,      /* k_chain_wave, first launch: n <= 512 */
       T1K_ROUTE_WAVE_LARGE = 2,      /* k_chain_wave, second launch: n <= 4096 */
       T1K_ROUTE_BIG_BY_SIZE = 3,     /* k_chain_big, more than 4096 hits (n is not kept by the kernels: 0xFFFFFFFF) */
       T1K_ROUTE_BIG_BY_SCRATCH = 4,  /* k_chain_big after the lane / wavefront met a gap beyond the register band */
       T1K_ROUTE_KINDS = 5 };
typedef struct {
  uint64_t ranges, ranges_nw5, ranges_nw10, ranges_xlong;  /* kept passes, by the instantiation of the chain kernels (xlong: also counted under its NW) */
  uint64_t groups, fast, slow, jobs, retry, finish, general, wave, genjobs, big, eq, band, wide, extjobs, extretry;
} t1k_route_totals;
typedef struct {
  uint32_t read_end, allele, n;   /* read-end index in the uploaded set; hits of the group (record word 4) */
  uint8_t strand;                 /* 0: the read-end as given, 1: its reverse complement */
  uint8_t near_done, simple;      /* k_near_hits wrote the hit list; ... and marked it a two-diagonal chain */
  uint8_t route;                  /* T1K_ROUTE_* */
  uint8_t nw, xlong, reserved[2]; /* 5 / 10; 1: the range held read-ends beyond 320 bases (k_near_hits did not run) */
} t1k_route_rec;
int t1k_route_report_enable(t1k_ctx *ctx, int on);
int t1k_route_report_get(t1k_ctx *ctx, t1k_route_totals *totals /* may be NULL */, t1k_route_rec *recs /* may be NULL */, uint64_t cap, uint64_t *nRecs);

/* ---- seed report: which k-mers of each read-end had their posting lists used (diagnostics and tests) ----------------
 * The look-up rule of SeqSet::GetHitsFromRead as the seeding kernels decided it, per read-end.  Host side only: no kernel knows of it.
 * Off by default, and then t1k_assign_range issues exactly the launches and copies it issues without it.  t1k_seed_report_enable(ctx, 1)
 * clears the report and starts it (start it again after another read set was uploaded: the records are indexed by read-end in the
 * uploaded set); (ctx, 0) stops it and drops what it held.  While it is on, every range that t1k_assign_range finishes copies, for each of
 * its read-ends, the used-k-mer counts per strand, the used entries and the two used-offset masks out of the seeding kernels' buffers;
 * a range that ran again after a capacity error counts once, from the pass that was kept, and a read-end assigned again replaces its record.
 * t1k_seed_report_get, every array optional (NULL), n = the read-ends of the uploaded set:
 *   seen[n]                            1: a finished range held the read-end since the report was started
 *   counts[n][2]                       used k-mers of the read-end as given / of its reverse complement
 *   masks[n][2][T1K_SEED_MASK_WORDS]   bit r = the list of the k-mer at read offset r of that strand is used; all zero for a read-end the
 *                                      mask kernel does not seed (shorter than k, beyond 320 bases, or linked to an earlier window)
 *   used[*nUsed]                       the used entries of all seen read-ends, by read-end, the read-end as given first, in the order the
 *                                      kernel kept them (ascending offset); cap < *nUsed: T1K_ERR_ARG, *nUsed is still set
 * T1K_ERR_STATE while the report is off. */
#define T1K_SEED_MASK_WORDS 10
typedef struct {
  uint32_t read_off, list_len;    /* offset of the k-mer in its strand's text; postings of its list */
  uint8_t strand, reserved[3];    /* 0: the read-end as given, 1: its reverse complement */
} t1k_seed_used;
int t1k_seed_report_enable(t1k_ctx *ctx, int on);
int t1k_seed_report_get(t1k_ctx *ctx, uint8_t *seen, uint32_t *counts, uint32_t *masks, t1k_seed_used *used, uint64_t cap, uint64_t *nUsed);

/* ---- reference view: the arrays t1k_ref_upload built, read back (diagnostics and tests) ----------------------------
 * Host side only: no kernel is launched and nothing in the context changes, so with the view unused t1k_ref_upload issues exactly the
 * launches and copies it issues without it.  Works on a context that uploaded its reference and on one that took it through
 * t1k_ref_share.  T1K_ERR_ARG when the context holds no reference.
 * t1k_ref_view_geometry: the sizes.  len[x] = elements of array x that the build defines (not the slack the kernels may fetch behind
 * them), elem_bytes[x] = bytes of one element:
 *   BASES / NMASK / EXON / POSTED   n_words 64-bit words, 32 positions a word, position q of a word in bits 2q (and 2q + 1 of BASES)
 *   BASES_T                         the transposed copy and the 512 zero words behind it; 0 when it was not built (has_bases_t = 0)
 *   BLOCK_T                         first word of every block of 64 alleles in BASES_T; 0 when it was not built
 *   ALLELE_OFF (u64) / ALLELE_LEN (u32) / ALLELE_HAS_N (u8)   one per allele;  SEP_START (u32) one more;  SEP_POS (i32) n_sep
 *   K_START                         4^k + 1;  K_HAS / K_MULTI  4^k / 32 words (at least 1);  K_HAS_PRE  4^max(1, k - 2) / 32 words
 *   K_DIR_IDX                       4^k;  K_DIR  dir_rows * dir_stride;  K_DIR_MASK (u64)  dir_rows * dir_mask_words
 *   K_POST (allele u32, offset u32) / K_POST_ALLELE (u32)     n_postings
 * t1k_ref_view_copy: elements [first, first + count) of one array to host memory (count * elem_bytes bytes); T1K_ERR_ARG for an unknown
 * array or a slice that leaves it (count = 0 at first <= len is legal).  At k = 15 K_START alone is 4 GB: read the cells you need. */
enum { T1K_REF_BASES = 0, T1K_REF_NMASK, T1K_REF_EXON, T1K_REF_POSTED, T1K_REF_BASES_T, T1K_REF_BLOCK_T, T1K_REF_ALLELE_OFF, T1K_REF_ALLELE_LEN,
       T1K_REF_ALLELE_HAS_N, T1K_REF_SEP_START, T1K_REF_SEP_POS, T1K_REF_K_START, T1K_REF_K_HAS, T1K_REF_K_MULTI, T1K_REF_K_HAS_PRE,
       T1K_REF_K_DIR_IDX, T1K_REF_K_DIR, T1K_REF_K_DIR_MASK, T1K_REF_K_POST, T1K_REF_K_POST_ALLELE, T1K_REF_ARRAYS };
typedef struct {
  uint32_t n_alleles, k;
  uint64_t total_bases, n_words, n_postings, bases_t_len, n_sep;
  uint32_t dir_rows, dir_stride, dir_mask_words, has_bases_t;
  uint64_t len[T1K_REF_ARRAYS];
  uint32_t elem_bytes[T1K_REF_ARRAYS];
} t1k_ref_geometry;
int t1k_ref_view_geometry(t1k_ctx *ctx, t1k_ref_geometry *out);
int t1k_ref_view_copy(t1k_ctx *ctx, int array, uint64_t first, uint64_t count, void *out);

/* wall time (ms) the context has spent allocating device memory and the bytes it asked for (diagnostics) */
double t1k_alloc_ms(t1k_ctx *ctx, uint64_t *bytes);
/* the device blocks the context holds right now, in bytes; print != 0: one line on stderr naming every block of 64 MB and more (diagnostics, T1K_DEBUG_MEM) */
uint64_t t1k_ctx_mem_report(t1k_ctx *ctx, const char *tag, int print);

/* ---- whole-stage job API (host C++ + the device stages above) ------------------------------------------------- */
/* argv-compatible replacement of the reference's genotyper executable (Genotyper.cpp:194-738). Returns the exit code. */
int t1k_genotyper_main(int argc, char **argv);
/* argv-compatible replacement of the reference's fastq-extractor main() (FastqExtractor.cpp:260-626; run-t1k:377-403) */
int t1k_extractor_main(int argc, char **argv);
/* argv-compatible replacement of the reference's bam-extractor main() (BamExtractor.cpp:463-949; run-t1k:350): candidate reads from a
 * coordinate-sorted BAM file -- reads over the gene intervals, reads on alternative contigs and unaligned reads that pass
 * IsLowComplexity + SeqSet::HasHitInSet (t1k_extract_batch).  The BAM container is read natively (BGZF blocks inflated in parallel). */
int t1k_bam_extractor_main(int argc, char **argv);
/* argv-compatible replacement of the reference's analyzer main() (Analyzer.cpp:236-733; run-t1k:438-449): re-assignment of the aligned reads
 * to the selected alleles, novel-variant calling (VariantCaller.hpp: host code over the GPU's overlap lists and alignments, see
 * t1k_variants_call below) and the per-barcode expression table */
int t1k_analyzer_main(int argc, char **argv);

typedef struct {
  t1k_params dev;
  double filter_frac, filter_cov, cross_gene_rate, squarem_min_alpha; /* --frac --cov --crossGeneRate --squaremMinAlpha */
  int32_t allele_digit_units;                                         /* --alleleDigitUnits, -1 = automatic */
  char allele_delimiter;                                              /* --alleleDelimiter, 0 = automatic */
  int32_t threads;                                                    /* -t: host parser/packer threads */
  int32_t device;                                                     /* GPU ordinal; -1 = host-only job (group bookkeeping only, cannot run) */
  int32_t output_read_assignment;                                     /* --outputReadAssignment */
  int32_t batch_fragments;                                            /* fragments per device batch (0 = default) */
  uint64_t bootstrap_seed;                                            /* --bootstrapSeed (default 1) */
  int32_t bootstrap;                                                  /* --bootstrap: replicates of the quantification, 1 .. 1000; 0 = no table */
  int32_t alternatives;                                               /* --alternatives: alternatives listed per called allele, 1 .. 1000; 0 = no table */
  int32_t diplotypes;                                                 /* --diplotypes: allele pairs listed per gene, 1 .. 1000; 0 = no table */
  int32_t diplo_candidates;                                           /* --diploCandidates: candidates per gene, 2 .. 2048 (default 512) */
} t1k_job_params;
void t1k_job_params_default(t1k_job_params *p);

int t1k_job_create(const t1k_job_params *p, const char *refFasta, t1k_job **out);
void t1k_job_destroy(t1k_job *job);
const char *t1k_job_last_error(const t1k_job *job);
/* load + keep reads on the host (FASTA/FASTQ, optionally gz); file2 NULL = single-end; barcodeFile may be NULL */
int t1k_job_load_reads(t1k_job *job, const char *file1, const char *file2, const char *barcodeFile);
/* several files per mate, read back to back (ReadFiles::AddReadFile, Genotyper.cpp: every -u / -1 / -2 adds one); files2 NULL = single-end */
int t1k_job_load_reads_multi(t1k_job *job, const char *const *files1, uint32_t n1, const char *const *files2, uint32_t n2, const char *barcodeFile);
/* The same input opened on its own, before or beside t1k_job_create (both calls block; a caller with two threads -- the genotyper
 * executable, bench.py -- maps and indexes the read files while the reference is parsed and the contexts come up; the reference's main
 * does the two one after the other, Genotyper.cpp:226-232 then 365-454).  `threads` as -t (0 = the default of a job).
 * t1k_job_attach_reads hands the input to an UNSHARDED job exactly as t1k_job_load_reads_multi would have left it and consumes the handle
 * (also on failure); t1k_reads_close is for a handle that was never attached.  A rank of a sharded job (t1k_job_set_shard with a
 * communicator) gets T1K_ERR_STATE whatever the input: its open is the collective t1k_job_load_reads, including the cases in which that
 * call ends up indexing the whole input on every rank (a barcode file, gz, non-strict layouts). */
typedef struct t1k_reads t1k_reads;
int t1k_reads_open(const char *const *files1, uint32_t n1, const char *const *files2, uint32_t n2, const char *barcodeFile, int threads, t1k_reads **out);
/* The same for a job of ONE rank, with ordinary .gz inputs not waited for: the .gz files of every mate (four-line FASTQ, not bgzip-framed; the same
 * number of files for each mate, read back to back) -- and the barcode file with them when it is a .gz file too -- are inflated by a decoder that publishes its progress while a second thread indexes the records behind it, and t1k_job_run
 * takes the fragments as they arrive -- as the reference's record-at-a-time reader does (ReadFiles.hpp:13, 95, 155-204; kseq.h:94-150).
 * t1k_reads_fragments / t1k_job_fragments wait for the end of the stream.  Inputs that are not eligible (plain files, mates with different
 * numbers of files, small files, text whose first 4 MB are not strict four-line records, T1K_STREAM_GZ=0) are opened exactly as by
 * t1k_reads_open.  Text that leaves the strict layout further on (a blank line between records, a last record without its quality line:
 * things the whole-file reader takes as the reference's kseq does) ends the stream; t1k_job_run then opens the files whole by itself and
 * starts over (one line on stderr says so), so the caller sees the result of t1k_reads_open at the price of the time lost. */
int t1k_reads_open_stream(const char *const *files1, uint32_t n1, const char *const *files2, uint32_t n2, const char *barcodeFile, int threads, t1k_reads **out);
const char *t1k_reads_last_error(const t1k_reads *reads);
int t1k_reads_fragments(const t1k_reads *reads, uint64_t *nFragments);
void t1k_reads_close(t1k_reads *reads);
int t1k_job_attach_reads(t1k_job *job, t1k_reads *reads);
/* or hand reads over from memory: concatenated ASCII + offsets, mates parallel; ids may be NULL ("r<i>") */
int t1k_job_set_reads(t1k_job *job, const char *seq1, const uint64_t *off1, const char *seq2, const uint64_t *off2, uint32_t nFragments);
/* read-end assignment, pairing, coalescing, EC build, EM, allele selection (Genotyper.cpp:451-650) */
int t1k_job_run(t1k_job *job);
/* optional, before t1k_job_run: the *_aligned*.fa files (which only need the fragmentAssigned flags) are then written by background
 * threads while the classes are built and the EM runs; t1k_job_write_outputs with the same prefix waits for them */
int t1k_job_set_output_prefix(t1k_job *job, const char *prefix);
/* <prefix>_genotype.tsv, _allele.tsv, _aligned*.fa, (_assign.tsv) (Genotyper.cpp:653-718), (_alternatives.tsv: prm.alternatives > 0), (_diplotypes.tsv: prm.diplotypes > 0), (_bootstrap.tsv: prm.bootstrap > 0) */
int t1k_job_write_outputs(t1k_job *job, const char *prefix);
/* results in memory: one line per gene, same text as _genotype.tsv */
int t1k_job_genotype_text(t1k_job *job, char *buf, uint64_t cap, uint64_t *needed);
/* after t1k_job_run of a job with prm.alternatives > 0 (the rank that writes the tables): the text of <prefix>_alternatives.tsv */
int t1k_job_alternatives_text(t1k_job *job, char *buf, uint64_t cap, uint64_t *needed);
/* after t1k_job_run of a job with prm.diplotypes > 0 (the rank that writes the tables): the text of <prefix>_diplotypes.tsv */
int t1k_job_diplotypes_text(t1k_job *job, char *buf, uint64_t cap, uint64_t *needed);
/* after t1k_job_run of a job with prm.bootstrap > 0 (the rank that writes the tables): the text of <prefix>_bootstrap.tsv */
int t1k_job_bootstrap_text(t1k_job *job, char *buf, uint64_t cap, uint64_t *needed);
/* ... and what it was computed from: abundance[(B + 1)][nAlleles], row r the per-allele abundance replicate r ended with (row 0: the data,
 * bit for bit the abundances of t1k_job_allele_table); rounds[B + 1]: SQUAREM rounds of each replicate's EM (0: none was run);
 * valid[B + 1]: 0 for a replicate without counts or with an abundance that is not finite.  Any array may be NULL; the two sizes always come back. */
int t1k_job_bootstrap_matrix(t1k_job *job, double *abundance, int32_t *rounds, uint8_t *valid, uint32_t *nReplicates, uint32_t *nAlleles);
/* TEST-ONLY: what the job's EM ran on besides the read groups, per allele of the reference and in its order: ec[a], its equivalence class (-1: in no
 * read group; a class's members in ascending order are its members in the EM's order), weight[a], the start weight, effLen[a] (a class's
 * length is the smallest of its members'), series[a], its major allele as an index into t1k_job_series_names.  Any array may be NULL. */
int t1k_job_em_alleles(t1k_job *job, int32_t *ec, int32_t *weight, int32_t *effLen, int32_t *series, uint32_t *nAlleles);
/* the names of the series (major alleles, the unit _genotype.tsv names), one per line, in reference order */
int t1k_job_series_names(t1k_job *job, char *buf, uint64_t cap, uint64_t *needed);
/* per allele of the job's reference, in its order: the gene (index into the lines of _genotype.tsv) and, after t1k_job_run, the abundance; either may be NULL */
int t1k_job_allele_table(t1k_job *job, int32_t *gene, double *abundance, uint32_t *nAlleles);
int t1k_job_counts(t1k_job *job, uint64_t *fragments, uint64_t *assignedFragments, uint64_t *groups, uint64_t *ecs, int32_t *emIterations);
int t1k_job_stats(t1k_job *job, t1k_stats *out);
t1k_ctx *t1k_job_ctx(t1k_job *job);
/* ---- multi-GPU jobs: one job per GPU (rank), every rank loads the same inputs and owns the fragments
 * [F * rank / nRanks, F * (rank + 1) / nRanks) in file order.  t1k_job_run then does, per rank: read-end assignment and pairing of its
 * slice (no collective), the coverage all-reduce, the row exchange + coalescing + group gather (t1k_rowset_exchange ...), the
 * replicated class build, the EM with a sharded row pass, and the replicated selection; every rank ends with the same result and the
 * complete fragmentAssigned flags, rank 0 writes the files.  The result is identical to a single-GPU run for any nRanks. */
int t1k_job_set_shard(t1k_job *job, int rank, int nRanks, t1k_comm *comm);
/* rank threads of one process: dst uses the read files src has mapped (t1k_job_load_reads on src only) */
int t1k_job_share_reads(t1k_job *dst, t1k_job *src);
int t1k_job_run_local(t1k_job *job);
/* the two halves of t1k_job_run: t1k_job_run_local = windows of fragments through the GPU up to the coalesced read groups (with the
 * exchanges of a sharded job), t1k_job_finish = classes, EM, pruning, selection */
int t1k_job_finish(t1k_job *job);
/* the job's group table as a byte string: [u64 nGroups][u64 nEntries][u64 assignedFragments][u64 groupPtr[nGroups+1]]
 * [u32 firstFragment[nGroups]][t1k_group_entry entries[nEntries]] */
int t1k_job_groups_serialize(t1k_job *job, void *buf, uint64_t cap, uint64_t *needed);
/* host half of the multi-GPU merge: the tables of all pattern owners become this job's table, ordered by first fragment */
int t1k_job_groups_merge(t1k_job *job, const void *const *bufs, const uint64_t *lens, uint32_t n);
/* host-side CoalesceReadAssignments (Genotyper.hpp:841-908) on caller-provided fragment rows, in order (tests; device = -1 jobs);
 * fragments[i] = global index of fragment i (NULL: 0, 1, ...) */
int t1k_job_coalesce_rows(t1k_job *job, const t1k_row_entry *rows, const uint32_t *rowCounts, const uint32_t *fragments, uint32_t nFragments);
/* device pointer + element count of the int32 coverage difference array (for an in-place all-reduce) */
int t1k_coverage_device(t1k_ctx *ctx, void **devPtr, uint64_t *count);

/* ---- novel-variant calling of the analyzer stage (VariantCaller.hpp:92-1311), host code ----------------------------------------------
 * One assignment of a fragment as SeqSet::ReadAssignmentToFragmentAssignment leaves it (_fragmentOverlap, SeqSet.hpp:146-173) with the
 * edit strings SeqSet::AddFragmentAlignmentInfo adds (SeqSet.hpp:2657-2681, 2758-2778: AlignAlgo::GlobalAlignment of the allele window
 * [seq_start, seq_end] against the read window [read_start, read_end] of the strand-corrected read -- t1k_align_batch): ops1 / ops2 are
 * where the strings of o1 / o2 start in the caller's `ops` bytes (0 match, 1 mismatch, 2 insert, 3 delete; no terminator). */
typedef struct {
  int32_t allele_idx;                 /* _fragmentOverlap::seqIdx */
  int32_t has_mate_pair, o1_from_r2;  /* SeqSet.hpp:155-156 */
  t1k_overlap o1, o2;                 /* o2 is read only when has_mate_pair */
  uint64_t ops1, ops2;
  uint32_t n_ops1, n_ops2;
} t1k_frag_assignment;
/* The overlaps behind a fragment's kept assignments: for every allele of the fragment's row (alleles[nAlleles], the row's order) the choice
 * SeqSet::ReadAssignmentToFragmentAssignment makes among the mates' overlaps on that allele (SeqSet.hpp:2310-2458: compatible pairs, or single
 * overlaps when one list is empty / the run is single-end, ranked by _fragmentOverlap::operator<), taken from the read-ends' final overlap
 * lists (t1k_overlaps_download).  paired = 0: a -u run (l2 ignored).  Fills allele_idx, has_mate_pair, o1_from_r2, o1, o2 of out[nAlleles]
 * (the ops fields are left 0).  T1K_ERR_ARG: an allele has no candidate in the lists.  Host code. */
int t1k_fragment_details(const t1k_overlap *l1, uint32_t n1, const t1k_overlap *l2, uint32_t n2, int paired, const int32_t *alleles, uint32_t nAlleles,
                         t1k_frag_assignment *out);
typedef struct {  /* _variant (VariantCaller.hpp:7-20) + the exonic coordinate OutputAlleleVCF prints */
  int32_t allele_idx, ref_pos, exon_pos;
  char ref, var;
  int32_t qual, group, output_group;
  double var_support, all_support, var_uniq_support;
} t1k_variant;
typedef struct t1k_variants t1k_variants;
/* VariantCaller::SetSeqAbundance + SetMaxVarGroupToResolve + ComputeVariant (249-271, 978-1140) on the alleles of `job` (a host-only job
 * will do: nothing here runs on the device).  abundance[nAlleles] = Genotyper::GetAlleleAbundance after the analyzer's EM
 * (Analyzer.cpp:609, 674); fragments in file order: fragment f has assignments asg[asgPtr[f] .. asgPtr[f + 1]) in the reference's list
 * order and reads read1[f][0 .. len1[f]) / read2[f][0 .. len2[f]) (read2 / len2 NULL: single-end).  var_max_group = --varMaxGroup.
 * The job must outlive the result. */
int t1k_variants_call(t1k_job *job, const double *abundance, int32_t var_max_group, uint32_t nFragments, const uint64_t *asgPtr, const t1k_frag_assignment *asg,
                      const int8_t *ops, const char *const *read1, const uint32_t *len1, const char *const *read2, const uint32_t *len2, t1k_variants **out);
uint32_t t1k_variants_count(const t1k_variants *v);
int t1k_variants_get(const t1k_variants *v, t1k_variant *out /* [t1k_variants_count] */);
/* the text of <prefix>_allele.vcf (VariantCaller::OutputAlleleVCF, 1202-1227); buf may be NULL to query the size */
int t1k_variants_vcf(const t1k_variants *v, char *buf, uint64_t cap, uint64_t *needed);
/* VariantCaller::AdjustFragmentAssignment (1229-1311) for one fragment: keep[i] = 1 for the assignments BarcodeSummary::AddFragment counts */
int t1k_variants_adjust(const t1k_variants *v, const t1k_frag_assignment *asg, uint32_t n, const int8_t *ops, const char *read1, uint32_t len1, const char *read2, uint32_t len2,
                        uint8_t *keep);
void t1k_variants_destroy(t1k_variants *v);

#ifdef __cplusplus
}
#endif
#endif /* T1K_GPU_H */
