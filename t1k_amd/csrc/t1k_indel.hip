// t1k_amd/csrc/t1k_indel.hip -- novel indel evidence per allele, left-aligned (analyzer --indels): the gap runs of the edit
// strings t1k_pileup.hip counts column by column, taken as events, normalised against the allele's bases and counted per booking.  The
// result is ONE sparse T1kCountTable, kept on the context from t1k_indel_begin to _end.
//
// An event is a maximal run of columns of one gap op (3 deletion, 2 insertion) that holds neither the first nor the last column of its
// edit string; a run that does is an EDGE run: its columns are counted (t1k_indel_stats), nothing else.  An insertion run and a deletion
// run that touch are two events.  A deletion of L allele bases from p on is (DEL, p, L); read bases S (L of them, as `text` holds them,
// anything but A/C/G/T as N) in front of allele base p are (INS, p, L, S).  Left-normalisation, against the allele's bases only, an N
// equal to nothing, itself included:
//   DEL: while p > 0 and allele[p-1] == allele[p+L-1]: p -= 1
//   INS: while p > 0 and allele[p-1] == S[-1]: S = allele[p-1] + S[:-1]; p -= 1
// S is never copied: after j shifts of an insertion first in front of q (its read bases R[0 .. L) in `text`), S[i] is allele[q - j + i] for
// i < j and R[i - j] from there on, so its last base is R[L - 1 - j] while j < L and allele[q - j + L - 1] beyond -- which is also the last
// deleted base of a deletion first at q after j shifts: one loop serves both.
// Per (event, booking) one key, count 1:
//   ((((g << 2 | type) << 27 | payload) << 1 | strand) << 1) | (1 - uniq)                                                     < 2^63
//   g = alleleOff[allele] + p (normalised) < 2^32;  type 0 deletion, payload L (< 2^27, else the call is refused);  type 1 short insertion
//   (L <= 13, all of S in ACGT), payload (1 << 2L) | the bases, 2 bits each, the first highest;  type 2 long insertion (L > 13, or an N
//   in S), payload min(L, 2^27 - 1): long insertions are told apart by position and length only.  A uniq booking is stored ONCE, under the
//   even key, as in t1k_sitepile.hip and t1k_support.hip: plain = even + odd, _uniq = even.
// One kernel, two instantiations, one wave64 per record, shaped like k_support; header, walk and verdict are t1k_walk.h's:
//   k_indel<false>  check and count: the walk's checks, a deletion too long for its payload, and per record four words -- events x
//                   bookings, events, edge deletion columns x bookings, edge insertion columns x bookings.  Only when the flag word comes
//                   back clear does the host take the exclusive sums and launch
//   k_indel<true>   emit at precomputed slots -- no atomics -- and the fifth word, the events whose position moved.
// An event is detected at the first column behind its run: op[c] != op[c-1], op[c-1] a gap, the run's start > 0.  Inside a 64-column step
// the start is the highest boundary column below the lane (a ballot); across steps two wave-uniform values carry on: the op of the last
// column so far and the length of the run that ends there.  The detecting lane has the allele position behind the run and the read bases
// in front of it from the walk; it normalises in a loop of its own (divergent, no cross-lane operation) and builds the key.  Inside a
// step with e events, booking b owns the e slots from slot + b e.
// No LDS, no scratch, no atomics on data (the flag word of the check excepted).  The table and its fold are a T1kCountTable (t1k_table.h),
// folded whenever the pending keys reach a bound (2^28, env T1K_INDEL_PENDING) and at _get.  The four statistics are sums of the
// per-record words (t1k_exclusive_sum_u64): they do not depend on the order in which waves finish.
// Shared with the other sparse stages, and not written out here: the session (ctx->ind, a T1kStage without sites: state checks, _get, the
// table part of _stats, _end) and the end of an _add call (t1k_stage_done) in t1k_table.h; the checks of records and booking lists
// (pileupBookLists) and the staging (pileupStage) in t1k_walk.h.  The sequence of _add stays here: it sums four rows in one scan, tells a
// too long deletion from the walk's faults, emits for events without bookings and scans a second time -- t1k_stage_two_pass does none of it.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"
#include "t1k_table.h"
#include "t1k_walk.h"

enum { INDEL_REF = 0 };  // of ctx->ind.more: the block [alleleOff | alleleText]
enum { INDEL_SHORT_MAX = 13, INDEL_PAYLOAD_BITS = 27, INDEL_BAD_DEL_LEN = 16, INDEL_WORDS = 5 };  // (the flag bit behind PILEUP_BAD_*)
static const uint32_t INDEL_PAYLOAD_MAX = (1u << INDEL_PAYLOAD_BITS) - 1u;

struct IndelArgs {
  PileupBatch in;
  const char *allele;                   // the alleles' bases back to back, A C G T N
  const uint8_t *strand;                // [n]
  const unsigned long long *bookPtr;    // [n + 1] into bookUniq
  const uint8_t *bookUniq;
  // [INDEL_WORDS][n + 1], the last of each row 0: <false> writes rows 0 .. 3 (events x bookings, events, edge del columns x bookings, edge ins
  // columns x bookings), <true> reads the exclusive sums of row 0 and writes row 4 (events whose position moved)
  unsigned long long *word;
  unsigned long long *keys;             // <true>: the pending keys of this call
  uint32_t *vals;                       //         and their counts (1 each)
};

__device__ __forceinline__ char indelBase(char c) { return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : 'N'; }  // a read base
__device__ __forceinline__ bool indelSame(char a, char b) { return a == b && a != 'N'; }                                // (both of A C G T N)

template <bool EMIT>
__global__ __launch_bounds__(256) void k_indel(IndelArgs P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nWaves = gridDim.x * 4u;
  for (uint32_t r = pileupUniform(blockIdx.x * 4u + (threadIdx.x >> 6)); r < P.in.n; r += nWaves) {
    const unsigned long long bookAt = pileupUniform64(P.bookPtr[r]);
    const uint32_t nBook = (uint32_t)(pileupUniform64(P.bookPtr[r + 1]) - bookAt);
    const PileupRec R = pileupLoadRec(P.in.aln, P.in.alleleOff, r);  // (its weights are not read here)
    const uint32_t strand = pileupUniform(P.strand[r]), nOps = R.nOps;
    const unsigned long long len = R.len, readAt = R.readAt;
    const uint32_t g0 = (uint32_t)R.base;                            // (fewer than 2^32 allele positions: pileupCheckOffsets)
    // <true>: the record's allele, the read bases of its window and its bookings (one address each: the wave-uniform registers are few)
    const char *al = P.allele + R.base, *rd = P.in.text + readAt;
    const uint8_t *uq = P.bookUniq + bookAt;
    unsigned long long slot = EMIT ? pileupUniform64(P.word[r]) : 0ull;  // wave-uniform: the next free key of this record
    // wave-uniform, from step to step: the first column of the step; the op of the last column so far and the length of the run that ends there
    uint32_t c0 = 0, carryLen = 0;
    int carryOp = -1;
    // <false>: the run from column 0 is still open, and its op
    bool leadOpen = true;
    int leadOp = -1;
    unsigned long long events = 0, edgeDel = 0, edgeIns = 0;
    uint32_t bad = 0, shifted = 0;
    const PileupWalkEnd end = pileupWalk<!EMIT, true>(P.in.ops, R.opsAt, nOps, R.seqStart, len, lane, [&](bool active, int op, unsigned long long pos, unsigned long long myP) {
      int prev = __shfl_up(op, 1);
      if (lane == 0) prev = carryOp;
      const bool bound = active && op != prev;                       // the column starts a run (column 0 does: carryOp is -1 there)
      const uint64_t mB = __ballot(bound ? 1 : 0);
      const uint64_t lower = mB & ((1ull << lane) - 1ull);
      // the run that ends in front of this lane's column: from the highest boundary below the lane, or from an earlier step
      const uint32_t L = lower ? lane - (63u - (uint32_t)__clzll((long long)lower)) : lane + carryLen;
      const bool ev = bound && (prev == 2 || prev == 3) && L < c0 + lane;  // (L == the column: the run holds column 0, an edge run)
      const uint64_t mE = __ballot(ev ? 1 : 0);
      const uint32_t e = (uint32_t)__popcll(mE);
      if (!EMIT) {
        events += e;
        if (__ballot((ev && prev == 3 && L > INDEL_PAYLOAD_MAX) ? 1 : 0)) bad |= INDEL_BAD_DEL_LEN;
        if (c0 == 0) leadOp = (int)pileupUniform((uint32_t)op);
        const uint64_t mBehind = c0 == 0 ? mB & ~1ull : mB;             // boundaries behind column 0
        if (leadOpen && mBehind) {                                      // the run from column 0 ends here, in front of the string's last column
          leadOpen = false;
          const uint32_t n = c0 + (uint32_t)__builtin_ctzll(mBehind);
          edgeDel += leadOp == 3 ? n : 0u;  // (two sums, not a choice between two counters: a chosen address would put both into scratch)
          edgeIns += leadOp == 2 ? n : 0u;
        }
      } else if (e) {  // wave-uniform
        unsigned long long key = 0;
        bool moved = false;
        if (ev) {
          const bool ins = prev == 2;
          // (allele positions, and g, fit 32 bits: pileupCheckOffsets)
          const uint32_t T = (uint32_t)pos + (op == 2 ? 1u : 0u);       // the allele position behind the run (an insert column behind a deletion books one in front of it)
          const uint32_t q = ins ? T : T - L;                           // in front of this base the bases are inserted; the first deleted base
          const char *S = rd + (myP - L);                               // ins: the inserted bases, L of them
          // one loop for both: after j shifts the base that must equal allele[q - j - 1] is the last of S -- S[L - 1 - j] while j < L, a base of
          // the allele put in front earlier beyond -- or the last deleted base, allele[q - j + L - 1] either way
          uint32_t j = 0;
          while (j < q) {
            const char last = (ins && j < L) ? indelBase(S[L - 1 - j]) : al[q - j + L - 1];
            if (!indelSame(al[q - j - 1], last)) break;
            ++j;
          }
          moved = j != 0;
          const uint32_t p = q - j;
          uint32_t type = 0, payload = L;                               // (a deletion: L <= INDEL_PAYLOAD_MAX, the check pass saw to it)
          if (ins) {
            type = 2;
            payload = min(L, INDEL_PAYLOAD_MAX);
            if (L <= (uint32_t)INDEL_SHORT_MAX) {
              uint32_t bits = 1;
              bool acgt = true;
              for (uint32_t i = 0; i < L; ++i) {
                const char c = i < j ? al[p + i] : indelBase(S[i - j]);
                acgt = acgt && c != 'N';
                bits = (bits << 2) | (c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u);
              }
              if (acgt) { type = 1; payload = bits; }
            }
          }
          key = ((((unsigned long long)(g0 + p) << 2) | type) << INDEL_PAYLOAD_BITS) | payload;
          key = ((key << 1) | strand) << 1;                             // 1 - uniq (bit 0) comes with the booking
        }
        shifted += (uint32_t)__popcll(__ballot(moved ? 1 : 0));
        const unsigned long long mine = slot + pileupBelow(mE);
        for (uint32_t b = 0; b < nBook; ++b) {
          const uint32_t uniq = pileupUniform(uq[b]);
          if (ev) {
            const unsigned long long at = mine + (unsigned long long)b * e;
            P.keys[at] = key | (1u - uniq);
            P.vals[at] = 1u;
          }
        }
        slot += (unsigned long long)e * nBook;
      }
      const uint32_t nAct = min(64u, nOps - c0);                        // the step's columns
      carryOp = __builtin_amdgcn_readlane(op, (int)(nAct - 1u));
      carryLen = mB ? nAct - (63u - (uint32_t)__clzll((long long)mB)) : carryLen + nAct;
      c0 += 64u;
    });
    if (!EMIT) {
      // the run that holds the last column (the whole string, if the run from column 0 never ended)
      edgeDel += carryOp == 3 ? carryLen : 0u;
      edgeIns += carryOp == 2 ? carryLen : 0u;
      bad |= pileupWalkVerdict(end, len, readAt, P.in.textBytes);
      if (lane == 0) {
        const unsigned long long row = (unsigned long long)P.in.n + 1ull;
        if (bad) atomicOr(P.in.flag, bad);
        P.word[r] = events * nBook;
        P.word[row + r] = events;
        P.word[2ull * row + r] = edgeDel * nBook;
        P.word[3ull * row + r] = edgeIns * nBook;
      }
    } else if (lane == 0) P.word[4ull * ((unsigned long long)P.in.n + 1ull) + r] = shifted;
  }
}

extern "C" {

int t1k_indel_begin(t1k_ctx *ctx, uint32_t nAlleles, const uint64_t *alleleOff, const char *alleleText) {
  if (!ctx) return T1K_ERR_ARG;
  T1kStage &s = ctx->ind;
  T1kDevBuf &ref = s.more[INDEL_REF].b;
  int rc;
  if ((rc = t1k_stage_closed(ctx, s))) return rc;
  if ((rc = pileupCheckOffsets(ctx, "t1k_indel_begin", "NULL arrays, or alleleOff not starting at 0", nAlleles, alleleOff))) return rc;
  const uint64_t total = alleleOff[nAlleles];
  if (total && !alleleText) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_indel_begin: bad arguments (NULL arrays, or alleleOff not starting at 0)");
  for (uint64_t i = 0; i < total; ++i) {
    const char c = alleleText[i];
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N') return t1k_fail(ctx, T1K_ERR_ARG, "t1k_indel_begin: a byte of alleleText outside ACGTN at offset " + std::to_string(i));
  }
  // one device block [alleleOff | alleleText]
  T1kCarve piece;
  const size_t oOff = piece(8ull * (nAlleles + 1ull)), oText = piece(total);
  (void)oOff;
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = t1k_ensure(ctx, ref, piece.off))) return rc;
  char *D = (char *)ref.p;
  T1K_HIP(ctx, hipMemcpyAsync(D, alleleOff, 8ull * (nAlleles + 1ull), hipMemcpyHostToDevice, ctx->stream));
  if (total) T1K_HIP(ctx, hipMemcpyAsync(D + oText, alleleText, total, hipMemcpyHostToDevice, ctx->stream));
  T1K_HIP(ctx, hipStreamSynchronize(ctx->stream));  // alleleOff / alleleText are the caller's again
  ctx->indTextAt = oText;
  ctx->indEvents = ctx->indShifted = ctx->indEdgeDel = ctx->indEdgeIns = 0;
  t1k_stage_open(s, nAlleles, alleleOff, (1ull << 63) - 1ull);
  return T1K_OK;
}

int t1k_indel_add(t1k_ctx *ctx, const t1k_pileup_aln *aln, uint32_t n, const uint8_t *strand, const uint64_t *bookPtr, const uint8_t *bookUniq, const char *text, uint64_t textBytes,
                  const int8_t *ops, uint64_t opsBytes, double *kernelMs) {
  if (!ctx) return T1K_ERR_ARG;
  if (kernelMs) *kernelMs = 0;
  T1kStage &s = ctx->ind;
  const T1kDevBuf &ref = s.more[INDEL_REF].b;
  int rc;
  if ((rc = t1k_stage_opened(ctx, s, "_add", "_begin"))) return rc;
  if (n == 0) return T1K_OK;
  if (!aln || !strand || !bookPtr || (textBytes && !text) || (opsBytes && !ops)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_indel_add: bad arguments (NULL arrays)");
  // what the host can tell from the records and the booking lists alone; the strings themselves are walked on the device before anything is emitted
  std::vector<uint64_t> bp;
  if ((rc = pileupBookLists(ctx, "t1k_indel_add", aln, n, s.off, textBytes, opsBytes, bookPtr, 31, bookUniq, "bookUniq", [&](uint32_t i) {
        return strand[i] > 1 ? "record " + std::to_string(i) + " has a strand other than 0 or 1" : std::string();
      }, bp))) return rc;
  const uint64_t book0 = bookPtr[0], nBook = bp[n];
  for (uint64_t j = book0; j < book0 + nBook; ++j)
    if (bookUniq[j] > 1) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_indel_add: booking " + std::to_string(j) + " has a uniq other than 0 or 1");
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  IndelArgs a{};
  a.in = PileupBatch{aln, n, text, textBytes, ops, (const unsigned long long *)ref.p, nullptr};
  const uint64_t row = (uint64_t)n + 1;
  size_t oStrand = 0, oBp = 0, oBook = 0, oWord = 0;
  if ((rc = pileupStage(ctx, s.in, opsBytes, [&](T1kCarve &piece) {
        oStrand = piece(n); oBp = piece(8ull * row); oBook = piece(nBook); oWord = piece(8ull * INDEL_WORDS * row);
      }, a.in))) return rc;
  char *D = (char *)s.in.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oStrand, strand, n, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oBp, bp.data(), 8ull * row, hipMemcpyHostToDevice, st));
  if (nBook) T1K_HIP(ctx, hipMemcpyAsync(D + oBook, bookUniq + book0, nBook, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oWord, 0, 8ull * INDEL_WORDS * row, st));
  a.allele = (const char *)ref.p + ctx->indTextAt;
  a.strand = (const uint8_t *)(D + oStrand);
  a.bookPtr = (const unsigned long long *)(D + oBp); a.bookUniq = (const uint8_t *)(D + oBook);
  a.word = (unsigned long long *)(D + oWord);
  const unsigned grid = t1k_grid(ctx, n, 4);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_indel<false>, dim3(grid), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  uint32_t flag = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&flag, a.in.flag, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (flag & ~(uint32_t)INDEL_BAD_DEL_LEN) return t1k_fail(ctx, T1K_ERR_ARG, pileupRefusal("t1k_indel_add", "nothing emitted", flag));
  if (flag) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_indel_add: nothing emitted: a deletion of 2^27 bases or more");
  // rows 0 .. 3 in one sum: row k's total is the difference of the sums at its last (zero) entry and at row k - 1's
  if ((rc = t1k_exclusive_sum_u64(ctx, a.word, a.word, 4 * row))) return rc;  // (in place: every tile is read before it is written)
  unsigned long long upTo[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) T1K_HIP(ctx, hipMemcpyAsync(&upTo[k], a.word + (k + 1) * row - 1, 8, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  const uint64_t emit = upTo[0], events = upTo[1] - upTo[0], edgeDel = upTo[2] - upTo[1], edgeIns = upTo[3] - upTo[2];
  unsigned long long shifted = 0;
  if (events) {  // (records without a booking take part: their events may move as well)
    if (emit && (rc = t1k_table_room(ctx, s.who, s.tab, emit, "lower T1K_INDEL_PENDING, or add fewer records per call", &a.keys, &a.vals))) return rc;
    hipLaunchKernelGGL(k_indel<true>, dim3(grid), dim3(256), 0, st, a);
    T1K_HIP(ctx, hipGetLastError());
    unsigned long long *moved = a.word + 4 * row;
    if ((rc = t1k_exclusive_sum_u64(ctx, moved, moved, row))) return rc;
    T1K_HIP(ctx, hipMemcpyAsync(&shifted, moved + n, 8, hipMemcpyDeviceToHost, st));
  }
  if ((rc = t1k_stage_done(ctx, kernelMs))) return rc;
  if (emit && (rc = t1k_table_commit(ctx, s.who, s.tab, emit))) return rc;
  ctx->indEvents += events; ctx->indShifted += shifted; ctx->indEdgeDel += edgeDel; ctx->indEdgeIns += edgeIns;
  return T1K_OK;
}

int t1k_indel_get(t1k_ctx *ctx, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *nRuns) { return t1k_stage_get(ctx, &t1k_ctx::ind, keys, counts, cap, nRuns); }

int t1k_indel_stats(t1k_ctx *ctx, uint64_t *events, uint64_t *shifted, uint64_t *edgeDelBooked, uint64_t *edgeInsBooked, uint64_t *keysEmitted, uint64_t *folds, double *foldMs) {
  int rc;
  if ((rc = t1k_stage_stats(ctx, &t1k_ctx::ind, keysEmitted, folds, foldMs))) return rc;
  if (events) *events = ctx->indEvents;
  if (shifted) *shifted = ctx->indShifted;
  if (edgeDelBooked) *edgeDelBooked = ctx->indEdgeDel;
  if (edgeInsBooked) *edgeInsBooked = ctx->indEdgeIns;
  return T1K_OK;
}

int t1k_indel_end(t1k_ctx *ctx) { return t1k_stage_end(ctx, &t1k_ctx::ind); }

}  // extern "C"
