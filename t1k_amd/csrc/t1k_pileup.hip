// t1k_amd/csrc/t1k_pileup.hip -- per-base pileup of alignments onto alleles (analyzer --pileup): 14 int32 counters per
// allele position (A C G T N del ins, weighted by w_all and by w_uniq), kept on the context from t1k_pileup_begin to t1k_pileup_end.
//
// One kernel, two instantiations:
//   k_pileup<false>  the check: walks every record's edit string without booking -- an op outside 0 .. 3, a walk that leaves its allele
//                    or the text sets a flag word.  Only when the flag comes back clear does the host launch
//   k_pileup<true>   the booking: the same walk with integer atomicAdd into the counter-major table.
// One wave64 per record, 64 edit columns per step.  Shared with k_sitepile and kept in t1k_walk.h: the record header, the walk, its verdict, and
// on the host the offset and record checks, the staging of a batch and the refusal message.  A lane's allele coordinate is seq_start + the non-insert ops before it, its read
// coordinate the non-delete ops before it: a ballot, a population count below the lane, and wave-uniform running totals -- no lane
// walks the string.  The table is counter-major (14 planes of alleleOff[nAlleles] ints), so a run of matches books 64 consecutive
// ints of at most five planes.  Record index, n_ops and the step count are wave-uniform (readfirstlane): no exec-mask loop around
// the cross-lane operations.  Integer sums are exact in any order: the table does not depend on the order of arrival.
#include <algorithm>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_walk.h"

struct PileupArgs {
  PileupBatch in;
  unsigned long long total;             // alleleOff[nAlleles]: ints per plane
  int32_t *table;                       // [14][total]
};

template <bool BOOK>
__global__ __launch_bounds__(256) void k_pileup(PileupArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) {
    if (BOOK && pileupUniform(P.in.aln[r].w_all) == 0) continue;  // (in front of the header's loads, as k_sitepile skips a record without bookings)
    const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);
    // (the walk itself lives in t1k_walk.h; the check instantiation asks for no columns)
    const PileupWalkEnd end = pileupWalk<!BOOK, BOOK>(P.in.ops, R.opsAt, R.nOps, R.seqStart, R.len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long myP) {
      if (!active) return;
      const uint32_t plane = op == 2 ? (uint32_t)PILEUP_INS : op == 3 ? (uint32_t)PILEUP_DEL : pileupBasePlane(P.in.text[R.readAt + myP]);
      int32_t *cell = P.table + (unsigned long long)plane * P.total + R.base + pos;
      atomicAdd(cell, (int32_t)R.wAll);
      if (R.wUniq) atomicAdd(cell + (unsigned long long)PILEUP_UNIQ * P.total, (int32_t)R.wUniq);
    });
    if (!BOOK) {
      const uint32_t bad = pileupWalkVerdict(end, R.len, R.readAt, P.in.textBytes);
      if (bad && lane == 0) atomicOr(P.in.flag, bad);
    }
  }
}

extern "C" {

int t1k_pileup_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff) {
  if (!ctx) return T1K_ERR_ARG;
  if (ctx->pileupOpen) return t1k_fail(ctx, T1K_ERR_STATE, "t1k_pileup_begin: a table is open already (t1k_pileup_end first)");
  int rc;
  if ((rc = pileupCheckOffsets(ctx, "t1k_pileup_begin", "alleleOff NULL or not starting at 0", nAlleles, alleleOff))) return rc;
  const uint64_t total = alleleOff[nAlleles];
  T1K_HIP(ctx, hipSetDevice(ctx->device));
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
    const std::string fault = pileupRecordFault(r, i, ctx->pileupOff, textBytes, opsBytes);
    if (!fault.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: " + fault);
    if (r.w_uniq > r.w_all) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_pileup_add: record " + std::to_string(i) + " has w_uniq > w_all");
    load[r.allele] += (uint64_t)r.w_all * r.n_ops;
    if (load[r.allele] > 0x7FFFFFFFull) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_pileup_add: the bookings on one allele could carry an int32 counter past 2^31 - 1");
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t tableBytes = (size_t)PILEUP_PLANES * total * 4;
  PileupArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, (const unsigned long long *)((char *)ctx->bPileup.p + (tableBytes + 255) / 256 * 256), nullptr};
  a.total = total; a.table = (int32_t *)ctx->bPileup.p;
  int rc;
  if ((rc = pileupStage(ctx, ctx->bPileupIn, opsBytes, [](T1kCarve &) {}, a.in))) return rc;
  const unsigned grid = t1k_grid(ctx, n, 4);  // four records per workgroup and pass
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_pileup<false>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  uint32_t flag = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.in.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal("t1k_pileup_add", "nothing booked", flag));
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
