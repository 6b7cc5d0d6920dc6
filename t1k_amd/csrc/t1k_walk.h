// t1k_amd/csrc/t1k_walk.h -- internal: what k_pileup (t1k_pileup.hip), k_sitepile (t1k_sitepile.hip), k_support (t1k_support.hip), k_phase_obs (t1k_phase.hip) and k_cigar_size /
// k_cigar_emit (t1k_cigar.hip) share, on both sides of the launch.
// Device: the record header of a wave (pileupLoadRec), the edit-string walk of one alignment by one wave64 (pileupWalk) and the verdict on
// where it ended (pileupWalkVerdict).  64 edit columns per step.  A lane's allele coordinate is seq_start + the non-insert ops before it, its
// read coordinate the non-delete ops before it: a ballot, a population count below the lane, and wave-uniform running totals -- no lane
// walks the string.  The loop control is wave-uniform, so the per-column callback runs with all 64 lanes converged and may itself use
// cross-lane operations.
// Host: the front end of a batch of t1k_pileup_aln records -- the allele offsets of a _begin call, the per-record checks of an _add call,
// the checks of its booking lists (t1k_sitepile.hip, t1k_support.hip, t1k_indel.hip), the staging of aln / text / ops / the flag word, and
// the message of a batch the device refused.
#pragma once
#include <string>
#include <vector>
#include "t1k_dev.h"
#include "t1k_launch.h"

enum { PILEUP_PLANES = 14, PILEUP_N = 4, PILEUP_DEL = 5, PILEUP_INS = 6, PILEUP_UNIQ = 7 };
enum { PILEUP_BAD_OP = 1, PILEUP_BAD_ALLELE_WALK = 2, PILEUP_BAD_TEXT_WALK = 4, PILEUP_BAD_READ_WINDOW = 8 };  // (the last: k_support's own check)

__device__ __forceinline__ uint32_t pileupUniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long pileupUniform64(unsigned long long v) {
  return ((unsigned long long)pileupUniform((uint32_t)(v >> 32)) << 32) | pileupUniform((uint32_t)v);
}
__device__ __forceinline__ uint32_t pileupBelow(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the counter plane of a column that is no gap: the read base, anything but A/C/G/T as N
__device__ __forceinline__ uint32_t pileupBasePlane(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : (uint32_t)PILEUP_N; }

// the head of both kernels' argument blocks: one batch of records on the device
struct PileupBatch {
  const t1k_pileup_aln *aln;
  uint32_t n;
  const char *text;
  unsigned long long textBytes;
  const int8_t *ops;
  const unsigned long long *alleleOff;  // [nAlleles + 1]
  uint32_t *flag;                       // PILEUP_BAD_* of the whole batch
};

// record r as its wave sees it, every field wave-uniform; base, len: its allele's first position in the offset space and its length
struct PileupRec {
  uint32_t allele, seqStart, nOps, wAll, wUniq;
  unsigned long long readAt, opsAt, base, len;
};
__device__ __forceinline__ PileupRec pileupLoadRec(const t1k_pileup_aln *aln, const unsigned long long *alleleOff, uint32_t r) {
  const t1k_pileup_aln *rec = aln + r;
  PileupRec R;
  R.allele = pileupUniform(rec->allele); R.seqStart = pileupUniform(rec->seq_start); R.nOps = pileupUniform(rec->n_ops);
  R.wAll = pileupUniform(rec->w_all); R.wUniq = pileupUniform(rec->w_uniq);
  R.readAt = pileupUniform64(rec->read_at); R.opsAt = pileupUniform64(rec->ops_at);
  R.base = pileupUniform64(alleleOff[R.allele]);
  R.len = pileupUniform64(alleleOff[R.allele + 1]) - R.base;
  return R;
}

struct PileupWalkEnd {
  unsigned long long t, p;  // allele position behind the last column, read bases consumed
  uint32_t bad;             // CHECK: PILEUP_BAD_OP if some op lies outside 0 .. 3
};

// ops[opsAt .. opsAt + nOps) from allele position seqStart of an allele of `len` bases; nOps, seqStart and len are wave-uniform.
// COLUMNS: column(active, op, pos, readPos) once per step on every lane -- active: the lane has a column; pos: the allele position the
// column books at (an insert: the position consumed last, seq_start if none yet, clamped to the allele's last position; with len == 0
// or on a walk that leaves the allele pos may lie outside 0 .. len - 1, which the check reports); readPos: the read bases in front of it.
template <bool CHECK, bool COLUMNS, class F>
__device__ __forceinline__ PileupWalkEnd pileupWalk(const int8_t *ops, unsigned long long opsAt, uint32_t nOps, uint32_t seqStart, unsigned long long len, uint32_t lane, F &&column) {
  unsigned long long t = seqStart, p = 0;
  uint32_t bad = 0;
  for (uint32_t c0 = 0; c0 < nOps; c0 += 64u) {
    const uint32_t col = c0 + lane;
    const bool active = col < nOps;
    const int op = active ? (int)ops[opsAt + col] : -1;
    const bool isT = active && op != 2, isP = active && op != 3;
    const uint64_t mT = __ballot(isT ? 1 : 0), mP = __ballot(isP ? 1 : 0);
    if (COLUMNS) {
      const unsigned long long myT = t + pileupBelow(mT), myP = p + pileupBelow(mP);
      unsigned long long pos = myT;
      if (op == 2) {
        pos = myT > seqStart ? myT - 1 : myT;   // the allele position consumed last; none yet: seq_start
        if (pos >= len) pos = len - 1;            // (an all-insert window at the allele's end)
      }
      column(active, op, pos, myP);
    }
    if (CHECK) bad |= __ballot((active && (op < 0 || op > 3)) ? 1 : 0) ? (uint32_t)PILEUP_BAD_OP : 0u;
    t += (uint32_t)__popcll(mT);
    p += (uint32_t)__popcll(mP);
  }
  return PileupWalkEnd{t, p, bad};
}

// the PILEUP_BAD_* bits of a finished check walk: its ops, and where it ended against the allele's length and the text's
__device__ __forceinline__ uint32_t pileupWalkVerdict(const PileupWalkEnd &end, unsigned long long len, unsigned long long readAt, unsigned long long textBytes) {
  uint32_t bad = end.bad;
  if (len == 0 || end.t > len) bad |= PILEUP_BAD_ALLELE_WALK;
  if (readAt + end.p > textBytes) bad |= PILEUP_BAD_TEXT_WALK;
  return bad;
}

// ---- host side: `who` is the calling entry point's name, the head of every message ----
// the allele offsets of a _begin call: given, from 0, never decreasing, fewer than 2^32 positions; badStart: the caller's words for the first
static inline int pileupCheckOffsets(t1k_ctx *ctx, const char *who, const char *badStart, uint32_t nAlleles, const uint64_t *alleleOff) {
  if (!alleleOff || alleleOff[0] != 0) return t1k_fail(ctx, T1K_ERR_ARG, std::string(who) + ": bad arguments (" + badStart + ")");
  for (uint32_t a = 0; a < nAlleles; ++a)
    if (alleleOff[a + 1] < alleleOff[a]) return t1k_fail(ctx, T1K_ERR_ARG, std::string(who) + ": the allele offsets decrease");
  if (alleleOff[nAlleles] >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, std::string(who) + ": more than 2^32 allele positions");
  return T1K_OK;
}

// what the host can tell from record i alone (off: the open table's allele offsets): the fault in words, T1K_ERR_ARG all of them, or empty
static inline std::string pileupRecordFault(const t1k_pileup_aln &r, uint32_t i, const std::vector<uint64_t> &off, uint64_t textBytes, uint64_t opsBytes) {
  if ((uint64_t)r.allele + 1 >= off.size()) return "record " + std::to_string(i) + " names an unknown allele";
  if (r.ops_at > opsBytes || r.n_ops > opsBytes - r.ops_at) return "the edit string of record " + std::to_string(i) + " leaves `ops`";
  if (r.read_at > textBytes) return "the read window of record " + std::to_string(i) + " starts behind `text`";
  if (r.seq_start > off[r.allele + 1] - off[r.allele]) return "record " + std::to_string(i) + " starts behind its allele";
  return std::string();
}

// the booking lists of an _add call whose record i books once per entry of book[bookPtr[i] .. bookPtr[i + 1]), and with them the records:
// per record, in this order, bookPtr decreases (T1K_ERR_ARG), 2^bookBits bookings or more (T1K_ERR_CAPACITY), pileupRecordFault, and the
// stage's own checks of the record, own(i): the fault in words, T1K_ERR_ARG, or empty; then bookings without a `book` (bookName: the
// argument's name).  bp: bookPtr rebased to the call's first booking, bp[n] the call's bookings
template <class Own>
static inline int pileupBookLists(t1k_ctx *ctx, const std::string &who, const t1k_pileup_aln *aln, uint32_t n, const std::vector<uint64_t> &off, uint64_t textBytes, uint64_t opsBytes,
                                  const uint64_t *bookPtr, int bookBits, const void *book, const char *bookName, Own &&own, std::vector<uint64_t> &bp) {
  for (uint32_t i = 0; i < n; ++i) {
    if (bookPtr[i + 1] < bookPtr[i]) return t1k_fail(ctx, T1K_ERR_ARG, who + ": bookPtr decreases at record " + std::to_string(i));
    if (bookPtr[i + 1] - bookPtr[i] >= (1ull << bookBits))
      return t1k_fail(ctx, T1K_ERR_CAPACITY, who + ": record " + std::to_string(i) + " has 2^" + std::to_string(bookBits) + " bookings or more");
    std::string fault = pileupRecordFault(aln[i], i, off, textBytes, opsBytes);
    if (fault.empty()) fault = own(i);
    if (!fault.empty()) return t1k_fail(ctx, T1K_ERR_ARG, who + ": " + fault);
  }
  if (bookPtr[n] != bookPtr[0] && !book) return t1k_fail(ctx, T1K_ERR_ARG, who + ": bad arguments (NULL " + bookName + ")");
  bp.resize((size_t)n + 1);
  for (uint32_t i = 0; i <= n; ++i) bp[i] = bookPtr[i] - bookPtr[0];
  return T1K_OK;
}

// in: the caller's aln / n / text / textBytes / ops and the device's alleleOff.  Copies the three arrays into `buf` -- [aln | text | ops |
// what `extra(carve)` asks for, the caller's own pieces | the flag word, cleared] -- and leaves their device addresses in `in`
template <class Extra>
static inline int pileupStage(t1k_ctx *ctx, T1kDevBuf &buf, uint64_t opsBytes, Extra &&extra, PileupBatch &in) {
  T1kCarve piece;
  const size_t oAln = piece(sizeof(t1k_pileup_aln) * (size_t)in.n), oText = piece(in.textBytes), oOps = piece(opsBytes);
  extra(piece);
  const size_t oFlag = piece(4);
  int rc;
  if ((rc = t1k_ensure(ctx, buf, piece.off))) return rc;
  char *D = (char *)buf.p;
  hipStream_t st = ctx->stream;
  T1K_HIP(ctx, hipMemcpyAsync(D + oAln, in.aln, sizeof(t1k_pileup_aln) * (size_t)in.n, hipMemcpyHostToDevice, st));
  if (in.textBytes) T1K_HIP(ctx, hipMemcpyAsync(D + oText, in.text, in.textBytes, hipMemcpyHostToDevice, st));
  if (opsBytes) T1K_HIP(ctx, hipMemcpyAsync(D + oOps, in.ops, opsBytes, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oFlag, 0, 4, st));
  in.aln = (const t1k_pileup_aln *)(D + oAln); in.text = D + oText; in.ops = (const int8_t *)(D + oOps); in.flag = (uint32_t *)(D + oFlag);
  return T1K_OK;
}

// the message of a batch whose check walk came back with `flag` set; verb: what did not happen ("nothing booked")
static inline std::string pileupRefusal(const char *who, const char *verb, uint32_t flag) {
  return std::string(who) + ": " + verb + ":" + ((flag & PILEUP_BAD_OP) ? " an op outside 0 .. 3;" : "") + ((flag & PILEUP_BAD_ALLELE_WALK) ? " a walk leaves its allele;" : "") +
         ((flag & PILEUP_BAD_TEXT_WALK) ? " a walk leaves `text`;" : "") + ((flag & PILEUP_BAD_READ_WINDOW) ? " a read window leaves its read;" : "");
}
