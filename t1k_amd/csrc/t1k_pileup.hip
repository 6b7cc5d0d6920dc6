// t1k_amd/csrc/t1k_pileup.hip -- per-base pileup of alignments onto alleles (analyzer --pileup): 14 int32 counters per
// allele position (A C G T N del ins, weighted by w_all and by w_uniq), kept on the context from t1k_pileup_begin to t1k_pileup_end.
//
// One kernel, two instantiations:
//   k_pileup<false>  the check: walks every record's edit string without booking -- an op outside 0 .. 3, a walk that leaves its allele
//                    or the text sets a flag word.  Only when the flag comes back clear does the host launch
//   k_pileup<true>   the booking: the same walk with integer atomicAdd into the counter-major table.
// One wave64 per record, 64 edit columns per step (the walk itself: t1k_walk.h, shared with k_sitepile).  A lane's allele coordinate is seq_start + the non-insert ops before it, its read
// coordinate the non-delete ops before it: a ballot, a population count below the lane, and wave-uniform running totals -- no lane
// walks the string.  The table is counter-major (14 planes of alleleOff[nAlleles] ints), so a run of matches books 64 consecutive
// ints of at most five planes.  Record index, n_ops and the step count are wave-uniform (readfirstlane): no exec-mask loop around
// the cross-lane operations.  Integer sums are exact in any order: the table does not depend on the order of arrival.
#include <algorithm>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_walk.h"

struct PileupArgs {
  const t1k_pileup_aln *aln;
  uint32_t n;
  const char *text;
  unsigned long long textBytes;
  const int8_t *ops;
  const unsigned long long *alleleOff;  // [nAlleles + 1]
  unsigned long long total;             // alleleOff[nAlleles]: ints per plane
  int32_t *table;                       // [14][total]
  uint32_t *flag;
};

template <bool BOOK>
__global__ __launch_bounds__(256) void k_pileup(PileupArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.n; r += nWaves) {
    const t1k_pileup_aln *rec = P.aln + r;
    const uint32_t allele = pileupUniform(rec->allele), seqStart = pileupUniform(rec->seq_start), nOps = pileupUniform(rec->n_ops);
    const uint32_t wAll = pileupUniform(rec->w_all), wUniq = pileupUniform(rec->w_uniq);
    const unsigned long long readAt = pileupUniform64(rec->read_at), opsAt = pileupUniform64(rec->ops_at);
    if (BOOK && wAll == 0) continue;
    const unsigned long long base = pileupUniform64(P.alleleOff[allele]);
    const unsigned long long len = pileupUniform64(P.alleleOff[allele + 1]) - base;
    // (the walk itself lives in t1k_walk.h; the check instantiation asks for no columns)
    const PileupWalkEnd end = pileupWalk<!BOOK, BOOK>(P.ops, opsAt, nOps, seqStart, len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long myP) {
      if (!active) return;
      const uint32_t plane = op == 2 ? (uint32_t)PILEUP_INS : op == 3 ? (uint32_t)PILEUP_DEL : pileupBasePlane(P.text[readAt + myP]);
      int32_t *cell = P.table + (unsigned long long)plane * P.total + base + pos;
      atomicAdd(cell, (int32_t)wAll);
      if (wUniq) atomicAdd(cell + (unsigned long long)PILEUP_UNIQ * P.total, (int32_t)wUniq);
    });
    if (!BOOK) {
      uint32_t bad = end.bad;
      if (len == 0 || end.t > len) bad |= PILEUP_BAD_ALLELE_WALK;
      if (readAt + end.p > P.textBytes) bad |= PILEUP_BAD_TEXT_WALK;
      if (bad && lane == 0) atomicOr(P.flag, bad);
    }
  }
}

static unsigned pileupGrid(t1k_ctx *ctx, uint64_t records) {  // four records per workgroup and pass
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 16, (records + 3) / 4));
}

extern "C" {

int t1k_pileup_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff) {
  if (!ctx) return T1K_ERR_ARG;
  if (ctx->pileupOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_pileup_begin: a table is open already (t1k_pileup_end first)");
  if (!alleleOff || alleleOff[0] != 0) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_begin: bad arguments (alleleOff NULL or not starting at 0)");
  for (uint32_t a = 0; a < nAlleles; ++a)
    if (alleleOff[a + 1] < alleleOff[a]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_begin: the allele offsets decrease");
  const uint64_t total = alleleOff[nAlleles];
  if (total >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_pileup_begin: more than 2^32 allele positions");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  // [14 planes | alleleOff]
  const size_t tableBytes = (size_t)PILEUP_PLANES * total * 4, offAt = (tableBytes + 255) / 256 * 256;
  if ((rc = t1k_ensure(ctx, ctx->bPileup, offAt + 8ull * (nAlleles + 1)))) return rc;
  if (tableBytes) T1K_HIP(ctx, hipMemsetAsync(ctx->bPileup.p, 0, tableBytes, ctx->stream));
  T1K_HIP(ctx, hipMemcpyAsync((char *)ctx->bPileup.p + offAt, alleleOff, 8ull * (nAlleles + 1), hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->pileupOff.assign(alleleOff, alleleOff + nAlleles + 1);
  ctx->pileupLoad.assign(nAlleles, 0);
  ctx->pileupOpen = true;
  return T1K_OK;
}

int t1k_pileup_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const char *text, uint64_t textBytes, const int8_t *ops, uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if (!ctx->pileupOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_pileup_add: no table is open (t1k_pileup_begin first)");
  if (n == 0) return T1K_OK;
  if (!aln || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: bad arguments (NULL arrays)");
  const uint32_t nAlleles = (uint32_t)ctx->pileupLoad.size();
  const uint64_t total = ctx->pileupOff[nAlleles];
  // what the host can tell from the records alone; the strings themselves are walked on the device before anything is booked
  std::vector<uint64_t> load(ctx->pileupLoad);
  for (uint32_t i = 0; i < n; ++i) {
    const t1k_pileup_aln &r = aln[i];
    if (r.allele >= nAlleles) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: record " + std::to_string(i) + " names an unknown allele");
    if (r.w_uniq > r.w_all) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: record " + std::to_string(i) + " has w_uniq > w_all");
    if (r.ops_at > opsBytes || r.n_ops > opsBytes - r.ops_at) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: the edit string of record " + std::to_string(i) + " leaves `ops`");
    if (r.read_at > textBytes) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: the read window of record " + std::to_string(i) + " starts behind `text`");
    if (r.seq_start > ctx->pileupOff[r.allele + 1] - ctx->pileupOff[r.allele]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: record " + std::to_string(i) + " starts behind its allele");
    load[r.allele] += (uint64_t)r.w_all * r.n_ops;
    if (load[r.allele] > 0x7FFFFFFFull) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_pileup_add: the bookings on one allele could carry an int32 counter past 2^31 - 1");
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  size_t off = 0;
  auto piece = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256 + 256; return o; };
  const size_t oAln = piece(sizeof(t1k_pileup_aln) * (size_t)n), oText = piece(textBytes), oOps = piece(opsBytes), oFlag = piece(4);
  int rc;
  if ((rc = t1k_ensure(ctx, ctx->bPileupIn, off))) return rc;
  char *D = (char *)ctx->bPileupIn.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oAln, aln, sizeof(t1k_pileup_aln) * (size_t)n, hipMemcpyHostToDevice, st));
  if (textBytes) T1K_HIP(ctx, hipMemcpyAsync(D + oText, text, textBytes, hipMemcpyHostToDevice, st));
  if (opsBytes) T1K_HIP(ctx, hipMemcpyAsync(D + oOps, ops, opsBytes, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oFlag, 0, 4, st));
  PileupArgs a{};
  a.aln = (const t1k_pileup_aln *)(D + oAln); a.n = n; a.text = D + oText; a.textBytes = textBytes; a.ops = (const int8_t *)(D + oOps);
  const size_t tableBytes = (size_t)PILEUP_PLANES * total * 4;
  a.alleleOff = (const unsigned long long *)((char *)ctx->bPileup.p + (tableBytes + 255) / 256 * 256);
  a.total = total; a.table = (int32_t *)ctx->bPileup.p; a.flag = (uint32_t *)(D + oFlag);
  const unsigned grid = pileupGrid(ctx, n);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_pileup<false>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  uint32_t flag = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag)
    return t1k_fail(ctx, T1K_ERR_ARG, std::string("t1k_pileup_add: nothing booked:") + ((flag & PILEUP_BAD_OP) ? " an op outside 0 .. 3;" : "") +
                                          ((flag & PILEUP_BAD_ALLELE_WALK) ? " a walk leaves its allele;" : "") + ((flag & PILEUP_BAD_TEXT_WALK) ? " a walk leaves `text`;" : ""));
  hipLaunchKernelGGL(k_pileup<true>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  T1K_HIP(ctx, hipStreamSynchronize(st));  // text / ops are the caller's again, the staging block the next call's
  ctx->pileupLoad.swap(load);
  float ms = 0;
  if (kernelMs && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms;
  return T1K_OK;
}

int t1k_pileup_get(t1k_ctx *ctx, int32_t *counts) {
  if (!ctx) return T1K_ERR_ARG;
  if (!ctx->pileupOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_pileup_get: no table is open");
  const size_t tableBytes = (size_t)PILEUP_PLANES * ctx->pileupOff.back() * 4;
  if (!tableBytes) return T1K_OK;
  if (!counts) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_get: bad arguments (NULL counts)");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  T1K_HIP(ctx, hipMemcpyAsync(counts, ctx->bPileup.p, tableBytes, hipMemcpyDeviceToHost, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return T1K_OK;
}

int t1k_pileup_end(t1k_ctx *ctx) {
  if (!ctx) return T1K_ERR_ARG;
  if (!ctx->pileupOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_pileup_end: no table is open");
  ctx->pileupOpen = false;
  ctx->pileupOff.clear();
  ctx->pileupLoad.clear();
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (T1kDevBuf *b : {&ctx->bPileup, &ctx->bPileupIn})
    if (b->p) { (void)t1k_dev_free(b->p); b->p = nullptr; b->bytes = 0; }
  return T1K_OK;
}

}  // extern "C"
