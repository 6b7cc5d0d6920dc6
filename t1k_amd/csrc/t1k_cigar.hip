// t1k_amd/csrc/t1k_cigar.hip -- CIGAR, MD:Z and NM:i of a batch of alignments from their edit strings and the alleles' bases (analyzer --sam;
// DESIGN §11.6).  Stateless: one call, nothing kept on the context.
//
// One wave64 per record, 64 edit columns per step; the record header, the walk and its verdict are k_pileup's (t1k_walk.h).  Two passes over
// the same device function, so that both count the same bytes:
//   k_cigar_size  the check walk (an op outside 0 .. 3, a walk that leaves its allele: the flag word) and per record the bytes of its CIGAR
//                 and of its MD value, nm and refSpan.  Only when the flag comes back clear does the host take the exclusive sums of the
//                 two byte counts (t1k_exclusive_sum_u64, once per arena), check them against the caller's capacities and launch
//   k_cigar_emit  the bytes, every record at its offset -- no atomics, plain vector stores.
// Inside a step nothing is walked and nothing goes through the LDS or a lane-to-lane move: the step's columns are five ballots (active,
// match, mismatch, insert, delete), and what a lane needs from the lanes below it is a shift, a count of leading zeros or a population
// count of those masks.
//   CIGAR: a lane is a run head when its class (M for ops 0 and 1, I, D) differs from the lane's below it; lane 0 compares with the class
//          carried from the step before.  A head CLOSES the run in front of it and writes it: its length is the distance to the highest
//          head below the lane, or lane + the carried length when there is none.  The run open at the end of a step is carried (class,
//          length so far); lane 0 writes the last one behind the walk.
//   MD:    every item is written by its own column.  A mismatch writes <matches since the item before><allele base>, the first column of
//          a deletion run (op 3 whose previous column is not op 3: an insert ends a run) <matches>^<base>, its other columns <base>.
//          The matches are the op-0 columns between the lane and the highest item below it, or the carried count + those below the lane.
//          Carried: the open match count and whether the step's last column was a deletion.  Lane 0 writes the final number.
//   A lane's output offset inside a step is the sum of the bytes of the items below it.  An item has at most 12 bytes (ten digits, ^, a
//   base), so the sum is four ballots -- one per bit of the byte count -- weighted by the population counts below the lane (cigarScan):
//   the wave prefix sum without a scan network.  ds_bpermute / DPP shifts would take six dependent steps per sum for the same result.
#include <algorithm>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_walk.h"

struct CigarArgs {
  PileupBatch in;                        // (text is not read: textBytes = 0)
  const uint32_t *clip;                  // [2 * n] front, back soft clip, or NULL
  const char *alleleText;
  unsigned long long *cigarPtr, *mdPtr;  // [n + 1]: k_cigar_size writes the records' byte counts, k_cigar_emit reads their exclusive sums
  uint32_t *nm, *refSpan;                // [n]
  char *cigar, *md;                      // k_cigar_emit: the arenas, cigarPtr[n] and mdPtr[n] bytes
};

__device__ __forceinline__ uint32_t cigarDigits(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ void cigarPut(char *dst, uint32_t v, uint32_t digits) {
  for (uint32_t d = digits; d-- > 0; v /= 10u) dst[d] = (char)('0' + v % 10u);
}
__device__ __forceinline__ uint32_t cigarTop(uint64_t m) { return 63u - (uint32_t)__clzll((long long)m); }  // the highest set bit of m != 0
// bytes < 16 on every lane: the sum over the lanes below this one; total: over the wave
__device__ __forceinline__ uint32_t cigarScan(uint32_t bytes, uint32_t &total) {
  uint32_t pre = 0;
  total = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint64_t m = __ballot((bytes >> b) & 1u);
    pre += pileupBelow(m) << b;
    total += (uint32_t)__popcll(m) << b;
  }
  return pre;
}

template <bool EMIT>
__device__ __forceinline__ void cigarRecord(const CigarArgs &P, uint32_t r, uint32_t lane) {
  const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);  // (its weights and read_at are not read here)
  const uint32_t front = P.clip ? pileupUniform(P.clip[2u * r]) : 0u, back = P.clip ? pileupUniform(P.clip[2u * r + 1u]) : 0u;
  const uint64_t lowMask = (1ull << lane) - 1ull;
  // wave-uniform: the next free byte of the record in either arena (k_cigar_size: the bytes so far), and what is carried over a step seam
  unsigned long long cAt = EMIT ? pileupUniform64(P.cigarPtr[r]) : 0ull, mAt = EMIT ? pileupUniform64(P.mdPtr[r]) : 0ull;
  uint32_t cCls = 3u, cLen = 0, cM = 0, cDel = 0, nm = 0, span = 0;
  auto letter = [](uint32_t cls) { return cls == 0u ? 'M' : cls == 1u ? 'I' : 'D'; };
  auto clipItem = [&](uint32_t len) {
    if (len == 0) return;
    const uint32_t dg = cigarDigits(len);
    if (EMIT && lane == 0) { cigarPut(P.cigar + cAt, len, dg); P.cigar[cAt + dg] = 'S'; }
    cAt += dg + 1u;
  };
  clipItem(front);
  const PileupWalkEnd end = pileupWalk<!EMIT, true>(P.in.ops, R.opsAt, R.nOps, R.seqStart, R.len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long) {
    const uint64_t mA = __ballot(active ? 1 : 0), mZ = __ballot((active && op == 0) ? 1 : 0), mX = __ballot((active && op == 1) ? 1 : 0);
    const uint64_t mI = __ballot((active && op == 2) ? 1 : 0), mD = __ballot((active && op == 3) ? 1 : 0);
    const uint32_t nAct = (uint32_t)__popcll(mA);  // 1 .. 64: the active lanes are 0 .. nAct - 1
    const uint32_t under = lane ? lane - 1u : 0u;
    // CIGAR
    const uint32_t cls = op == 2 ? 1u : op == 3 ? 2u : 0u;
    const uint32_t prev = lane == 0 ? cCls : ((mI >> under) & 1ull) ? 1u : ((mD >> under) & 1ull) ? 2u : 0u;
    const bool head = active && cls != prev;
    const uint64_t mH = __ballot(head ? 1 : 0), hb = mH & lowMask;
    const uint32_t len = hb ? lane - cigarTop(hb) : cLen + lane;
    const bool closes = head && len > 0;  // (the first column of the string is a head with nothing in front of it)
    const uint32_t dg = cigarDigits(len);
    uint32_t total;
    const uint32_t pre = cigarScan(closes ? dg + 1u : 0u, total);
    if (EMIT && closes) {
      char *dst = P.cigar + cAt + pre;
      cigarPut(dst, len, dg);
      dst[dg] = letter(prev);
    }
    cAt += total;
    if (mH) {  // wave-uniform
      const uint32_t j = cigarTop(mH);
      cLen = nAct - j;
      cCls = ((mI >> j) & 1ull) ? 1u : ((mD >> j) & 1ull) ? 2u : 0u;
    } else cLen += nAct;
    // MD
    const bool isDel = active && op == 3;
    const bool prevDel = lane == 0 ? cDel != 0 : ((mD >> under) & 1ull) != 0;
    const bool delStart = isDel && !prevDel, numbered = (active && op == 1) || delStart;
    const uint64_t mItem = mX | mD, ib = mItem & lowMask;
    const uint32_t m = ib ? (uint32_t)__popcll(mZ & lowMask & ~((2ull << cigarTop(ib)) - 1ull)) : cM + (uint32_t)__popcll(mZ & lowMask);
    const uint32_t mdg = cigarDigits(m);
    const uint32_t bytes = numbered ? mdg + (delStart ? 2u : 1u) : isDel ? 1u : 0u;
    const uint32_t mpre = cigarScan(bytes, total);
    if (EMIT && bytes) {
      char *dst = P.md + mAt + mpre;
      if (numbered) {
        cigarPut(dst, m, mdg);
        dst += mdg;
        if (delStart) *dst++ = '^';
      }
      *dst = P.alleleText[R.base + pos];  // (pos < len: the check walk of k_cigar_size has been over this record)
    }
    mAt += total;
    if (mItem) cM = (uint32_t)__popcll((mZ >> cigarTop(mItem)) >> 1);  // the matches above the step's last item
    else cM += (uint32_t)__popcll(mZ);
    cDel = (uint32_t)((mD >> (nAct - 1u)) & 1ull);
    nm += (uint32_t)__popcll(mX | mI | mD);
    span += (uint32_t)__popcll(mZ | mX | mD);
  });
  // the run that is still open (n_ops > 0: there is one), the back clip, and MD's final number
  {
    const uint32_t dg = cigarDigits(cLen);
    if (EMIT && lane == 0) { cigarPut(P.cigar + cAt, cLen, dg); P.cigar[cAt + dg] = letter(cCls); }
    cAt += dg + 1u;
  }
  clipItem(back);
  {
    const uint32_t dg = cigarDigits(cM);
    if (EMIT && lane == 0) cigarPut(P.md + mAt, cM, dg);
    mAt += dg;
  }
  if (!EMIT) {
    const uint32_t bad = pileupWalkVerdict(end, R.len, 0ull, ~0ull);
    if (lane == 0) {
      if (bad) atomicOr(P.in.flag, bad);
      P.cigarPtr[r] = cAt; P.mdPtr[r] = mAt;
      P.nm[r] = nm; P.refSpan[r] = span;
    }
  }
}

__global__ __launch_bounds__(256) void k_cigar_size(CigarArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) cigarRecord<false>(P, r, lane);
}

__global__ __launch_bounds__(256) void k_cigar_emit(CigarArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) cigarRecord<true>(P, r, lane);
}

extern "C" {

int t1k_cigar_batch(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint32_t *clip, const int8_t *ops, uint64_t opsBytes, uint32_t nAlleles, const uint64_t *alleleOff,
                    const char *alleleText, uint64_t *cigarPtr, char *cigar, uint64_t cigarCap, uint64_t *mdPtr, char *md, uint64_t mdCap, uint32_t *nm, uint32_t *refSpan, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  if (!cigarPtr || !mdPtr) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_cigar_batch: bad arguments (NULL cigarPtr / mdPtr)");
  if (n == 0) { cigarPtr[0] = mdPtr[0] = 0; return T1K_OK; }
  if (!aln || (opsBytes && !ops) || !nm || !refSpan || (cigarCap && !cigar) || (mdCap && !md)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_cigar_batch: bad arguments (NULL arrays)");
  int rc;
  if ((rc = pileupCheckOffsets(ctx, "t1k_cigar_batch", "alleleOff NULL or not starting at 0", nAlleles, alleleOff))) return rc;
  const uint64_t total = alleleOff[nAlleles];
  if (total && !alleleText) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_cigar_batch: bad arguments (NULL alleleText)");
  // what the host can tell from the records alone (no read text: read_at is not looked at); the strings themselves are walked on the device
  const std::vector<uint64_t> off(alleleOff, alleleOff + nAlleles + 1);
  for (uint32_t i = 0; i < n; ++i) {
    const std::string fault = pileupRecordFault(aln[i], i, off, ~0ull, opsBytes);
    if (!fault.empty()) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_cigar_batch: " + fault);
    if (aln[i].n_ops == 0) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_cigar_batch: record " + std::to_string(i) + " has an empty edit string");
  }
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  T1kCallBlock blk, out;  // (freed on every return, behind the stream's work)
  blk.stream = out.stream = st;
  CigarArgs a{};
  a.in = PileupBatch{aln, n, nullptr, 0, ops, nullptr, nullptr};
  size_t oClip = 0, oOff = 0, oText = 0, oCp = 0, oMp = 0, oNm = 0, oSpan = 0;
  if ((rc = pileupStage(ctx, blk.buf, opsBytes, [&](T1kCarve &piece) {
         oClip = piece(clip ? 8ull * n : 0); oOff = piece(8ull * (nAlleles + 1ull)); oText = piece(total);
         oCp = piece(8ull * (n + 1ull)); oMp = piece(8ull * (n + 1ull)); oNm = piece(4ull * n); oSpan = piece(4ull * n);
       }, a.in))) return rc;
  char *D = (char *)blk.buf.p;
  if (clip) T1K_HIP(ctx, hipMemcpyAsync(D + oClip, clip, 8ull * n, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oOff, alleleOff, 8ull * (nAlleles + 1ull), hipMemcpyHostToDevice, st));
  if (total) T1K_HIP(ctx, hipMemcpyAsync(D + oText, alleleText, total, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oCp, 0, 8ull * (n + 1ull), st));
  T1K_HIP(ctx, hipMemsetAsync(D + oMp, 0, 8ull * (n + 1ull), st));
  a.in.alleleOff = (const unsigned long long *)(D + oOff);
  a.clip = clip ? (const uint32_t *)(D + oClip) : nullptr;
  a.alleleText = D + oText;
  a.cigarPtr = (unsigned long long *)(D + oCp); a.mdPtr = (unsigned long long *)(D + oMp);
  a.nm = (uint32_t *)(D + oNm); a.refSpan = (uint32_t *)(D + oSpan);
  const unsigned grid = t1k_grid(ctx, n, 4);  // four records per workgroup and pass
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_cigar_size, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_exclusive_sum_u64(ctx, a.cigarPtr, a.cigarPtr, (uint64_t)n + 1))) return rc;  // (in place: every tile is read before it is written)
  if ((rc = t1k_exclusive_sum_u64(ctx, a.mdPtr, a.mdPtr, (uint64_t)n + 1))) return rc;
  uint32_t flag = 0;
  unsigned long long cBytes = 0, mBytes = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.in.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&cBytes, a.cigarPtr + n, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&mBytes, a.mdPtr + n, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal("t1k_cigar_batch", "nothing written", flag));
  if (cBytes > cigarCap) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_cigar_batch: the cigar arena is too small: " + std::to_string(cBytes) + " bytes needed, " + std::to_string(cigarCap) + " given");
  if (mBytes > mdCap) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_cigar_batch: the md arena is too small: " + std::to_string(mBytes) + " bytes needed, " + std::to_string(mdCap) + " given");
  T1kCarve piece;
  const size_t oCigar = piece(cBytes), oMd = piece(mBytes);
  if ((rc = t1k_ensure(ctx, out.buf, piece.off))) return rc;
  a.cigar = (char *)out.buf.p + oCigar; a.md = (char *)out.buf.p + oMd;
  hipLaunchKernelGGL(k_cigar_emit, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  T1K_HIP(ctx, hipStreamSynchronize(st));  // (a device fault shows here, before any output array is touched)
  // everything is sound: only now the caller's arrays
  T1K_HIP(ctx, hipMemcpyAsync(cigarPtr, a.cigarPtr, 8ull * (n + 1ull), hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(mdPtr, a.mdPtr, 8ull * (n + 1ull), hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(nm, a.nm, 4ull * n, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(refSpan, a.refSpan, 4ull * n, hipMemcpyDeviceToHost, st));
  if (cBytes) T1K_HIP(ctx, hipMemcpyAsync(cigar, a.cigar, cBytes, hipMemcpyDeviceToHost, st));
  if (mBytes) T1K_HIP(ctx, hipMemcpyAsync(md, a.md, mBytes, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  float ms = 0;
  if (kernelMs && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) *kernelMs = ms;
  return T1K_OK;
}

}  // extern "C"
