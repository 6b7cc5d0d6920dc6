// Host harness of the selection's emit rule on an unsorted list (t1k_amd/csrc/t1k_select_rule.h, the functions k_select's CUT
// instantiations call): random lists are decided twice, by the rule's two order statistics as the kernel composes them (a min-reduction
// for the latch, its exact settlement among candidates of one class and allele, a max-reduction for `good`, the emit predicate) and by the
// positional rule of the sorted selection (sort by class and allele, then the seed coordinates, then the candidate number; the first
// candidate without separator whose extension failed is the latch; `good` is the seed match count of the first emitted candidate before
// it; behind it a candidate with a smaller seed match count is not tried unless KEEPCLIP).  The emit sets must be equal.  Then the
// bitmap prefix -> position mapping of the cut's compaction at word boundaries.  Built with -fsanitize=address,undefined.
//   select_emit_san <lists> <seed>   prints "ok <lists> lists: <no latch> <latch first> <good -1> <keepclip behind> <latch ties> <full ties> <bitmaps>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "t1k_select_rule.h"

struct Cand {
  uint64_t ca;       // class and allele: (MMAX - seed) << 16 | spans << 8 | allele
  int seed;
  uint32_t readSE;
  int32_t seqStart, seqEnd;
  uint32_t flags, idx;
};

// the selection's order, written out on the fields (not through SelTie)
static bool before(const Cand &a, const Cand &b) {
  if (a.ca != b.ca) return a.ca < b.ca;
  const int ars = a.readSE & 0xFFFF, are = a.readSE >> 16, brs = b.readSE & 0xFFFF, bre = b.readSE >> 16;
  if (ars != brs) return ars < brs;
  if (are != bre) return are < bre;
  if (a.seqStart != b.seqStart) return a.seqStart < b.seqStart;
  if (a.seqEnd != b.seqEnd) return a.seqEnd < b.seqEnd;
  return a.idx < b.idx;
}

struct Seen { long noLatch = 0, latchFirst = 0, goodNone = 0, keepBehind = 0, latchTie = 0, fullTie = 0; };

static std::vector<char> positional(const std::vector<Cand> &c, Seen &seen) {
  std::vector<Cand> s(c);
  std::sort(s.begin(), s.end(), before);
  const int n = (int)s.size();
  int latch = 0x7FFFFFFF, first = 0x7FFFFFFF;
  for (int i = 0; i < n; ++i)
    if (!(s[i].flags & SEL_F_SEPSEED) && !(s[i].flags & SEL_F_EXTOK)) { latch = i; break; }
  for (int i = 0; i < n && i < latch; ++i)
    if (!(s[i].flags & SEL_F_SEPSEED) && (s[i].flags & SEL_F_EXTOK)) { first = i; break; }
  const int good = first == 0x7FFFFFFF ? -1 : s[first].seed;
  std::vector<char> emit(n, 0);
  bool keepBehind = false;
  for (int i = 0; i < n; ++i) {
    if (s[i].flags & SEL_F_SEPSEED) continue;
    bool tried = true;
    if (i > latch && s[i].seed < good && !(s[i].flags & SEL_F_KEEPCLIP)) tried = false;
    if (i > latch && s[i].seed < good && (s[i].flags & SEL_F_KEEPCLIP) && (s[i].flags & SEL_F_EXTOK)) keepBehind = true;
    emit[s[i].idx] = tried && (s[i].flags & SEL_F_EXTOK);
  }
  if (latch == 0x7FFFFFFF) ++seen.noLatch;
  if (latch == 0) ++seen.latchFirst;
  if (latch != 0x7FFFFFFF && good == -1) ++seen.goodNone;
  if (keepBehind) ++seen.keepBehind;
  if (latch != 0x7FFFFFFF) {
    bool tie = false, full = false;
    for (int i = 0; i < n; ++i) {
      if (i == latch || s[i].ca != s[latch].ca || (s[i].flags & SEL_F_SEPSEED)) continue;
      tie = true;
      if (s[i].readSE == s[latch].readSE && s[i].seqStart == s[latch].seqStart && s[i].seqEnd == s[latch].seqEnd) full = true;
    }
    seen.latchTie += tie; seen.fullTie += full;
  }
  return emit;
}

// the rule as the kernel composes it, over the list in candidate order
static std::vector<char> byRule(const std::vector<Cand> &c, int iBits) {
  const uint32_t n = (uint32_t)c.size();
  const uint64_t iMask = (1ull << iBits) - 1;
  auto tieOf = [&](uint32_t i) { return selTieOf(c[i].readSE, c[i].seqStart, c[i].seqEnd, i); };
  uint64_t lKey = ~0ull;
  for (uint32_t i = 0; i < n; ++i)
    if (selLatchCand(c[i].flags)) lKey = std::min(lKey, c[i].ca << iBits | i);
  const bool hasL = lKey != ~0ull;
  const uint64_t caL = lKey >> iBits;
  uint32_t idxL = (uint32_t)(lKey & iMask);
  if (hasL) {
    bool tie = false;
    for (uint32_t i = 0; i < n; ++i) tie |= selLatchCand(c[i].flags) && c[i].ca == caL && i != idxL;
    if (tie) {
      uint64_t hi = ~0ull, lo = ~0ull;
      for (uint32_t i = 0; i < n; ++i)
        if (selLatchCand(c[i].flags) && c[i].ca == caL) hi = std::min(hi, tieOf(i).hi);
      for (uint32_t i = 0; i < n; ++i)
        if (selLatchCand(c[i].flags) && c[i].ca == caL && tieOf(i).hi == hi) lo = std::min(lo, tieOf(i).lo);
      idxL = (uint32_t)(lo & 0xFFFFFFFFull);
    }
  }
  SelTie tieL{0, 0};
  if (hasL) tieL = tieOf(idxL);
  std::vector<uint32_t> marks(n);
  int good = -1;
  for (uint32_t i = 0; i < n; ++i) {
    const bool bef = hasL ? selBeforeLatch(c[i].ca, caL, tieL, [&]() { return tieOf(i); }) : true;
    marks[i] = selMarks(c[i].flags, hasL, bef);
    if (selCountsForGood(marks[i])) good = std::max(good, c[i].seed);
  }
  std::vector<char> emit(n);
  for (uint32_t i = 0; i < n; ++i) emit[i] = selEmit(marks[i], c[i].seed, good);
  return emit;
}

static long bitmaps(std::mt19937_64 &rng) {
  long done = 0;
  for (uint32_t n : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 1000u, 1001u, 2048u, 2049u, 4095u, 4096u, 4097u}) {
    for (int pattern = 0; pattern < 6; ++pattern) {
      const uint32_t nWords = (n + 63) / 64;
      std::vector<uint64_t> bits(nWords, 0);
      std::vector<char> flag(n);
      for (uint32_t i = 0; i < n; ++i) {
        const bool f = pattern == 0 ? true : pattern == 1 ? (i & 63) == 63 : pattern == 2 ? (i & 63) == 0 : pattern == 3 ? (i & 63) == 0 || (i & 63) == 63 : (rng() % (pattern == 4 ? 2 : 9)) != 0;
        flag[i] = f;
        if (f) bits[i >> 6] |= 1ull << (i & 63);
      }
      std::vector<uint32_t> base(nWords);
      uint32_t run = 0;
      for (uint32_t w = 0; w < nWords; ++w) { base[w] = run; run += (uint32_t)__builtin_popcountll(bits[w]); }
      uint32_t want = 0;
      for (uint32_t i = 0; i < n; ++i) {
        if (!flag[i]) continue;
        if (selBitPos(bits.data(), base.data(), i) != want) { printf("bitmap n %u pattern %d candidate %u: place %u, want %u\n", n, pattern, i, selBitPos(bits.data(), base.data(), i), want); return -1; }
        ++want;
      }
      if (want != run) return -1;
      ++done;
    }
  }
  return done;
}

int main(int argc, char **argv) {
  const long lists = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? atoll(argv[2]) : 1);
  Seen seen;
  const int MMAX = 1023;
  for (long it = 0; it < lists; ++it) {
    const int shape = (int)(rng() % 6);
    const uint32_t n = 1 + (uint32_t)(rng() % (it % 50 == 0 ? 700 : 40));
    int iBits = 1;
    while ((1u << iBits) < n) ++iBits;
    const int seeds = 1 + (int)(rng() % 4), alleles = 1 + (int)(rng() % (shape == 5 ? 3 : 12)), coords = 1 + (int)(rng() % 3);
    const int failPct = shape == 0 ? 0 : 5 + (int)(rng() % 40), sepPct = (int)(rng() % 30), keepPct = (int)(rng() % 60);
    std::vector<Cand> c(n);
    for (uint32_t i = 0; i < n; ++i) {
      Cand &x = c[i];
      x.idx = i;
      x.seed = 200 + 10 * (int)(rng() % seeds);
      const uint32_t allele = (uint32_t)(rng() % alleles), spans = (uint32_t)(rng() % 2);
      x.ca = ((uint64_t)(MMAX - x.seed) << 16) | (uint64_t)spans << 8 | allele;
      const uint32_t rs = (uint32_t)(rng() % coords), rend = 100 + (uint32_t)(rng() % coords);
      x.readSE = rs | rend << 16;
      x.seqStart = (int32_t)(rng() % coords) - 1;  // (an allele start of -1 keeps the signed order honest)
      x.seqEnd = 150 + (int32_t)(rng() % coords);
      x.flags = ((int)(rng() % 100) < sepPct ? SEL_F_SEPSEED : 0u) | ((int)(rng() % 100) < failPct ? 0u : SEL_F_EXTOK) | ((int)(rng() % 100) < keepPct ? SEL_F_KEEPCLIP : 0u);
    }
    if (shape == 1) {  // the latch first: a failing candidate in front of every class
      c[rng() % n].ca = 0; for (auto &x : c) if (x.ca == 0) { x.flags &= ~(SEL_F_EXTOK | SEL_F_SEPSEED); x.seed = MMAX; }
    }
    if (shape == 2) {  // nothing emitted before the latch: whatever lies in the best class has a separator or fails
      uint64_t best = ~0ull;
      for (auto &x : c) best = std::min(best, x.ca >> 16);
      bool fail = false;
      for (auto &x : c) if ((x.ca >> 16) == best) { if (!fail) { x.flags &= ~(SEL_F_EXTOK | SEL_F_SEPSEED); fail = true; } else if (x.flags & SEL_F_EXTOK) x.flags |= SEL_F_SEPSEED; }
    }
    const std::vector<char> a = positional(c, seen), b = byRule(c, iBits);
    if (a != b) {
      printf("list %ld (n %u, shape %d): the emit sets differ\n", it, n, shape);
      for (uint32_t i = 0; i < n; ++i) printf("  %u: ca %llx seed %d readSE %x seq %d..%d flags %u  positional %d rule %d\n", i, (unsigned long long)c[i].ca, c[i].seed, c[i].readSE, c[i].seqStart, c[i].seqEnd, c[i].flags, a[i], b[i]);
      return 1;
    }
  }
  const long bm = bitmaps(rng);
  if (bm < 0) return 1;
  printf("ok %ld lists: %ld %ld %ld %ld %ld %ld %ld\n", lists, seen.noLatch, seen.latchFirst, seen.goodNone, seen.keepBehind, seen.latchTie, seen.fullTie, bm);
  return 0;
}
