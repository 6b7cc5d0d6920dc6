// tests/harness/ga_core_cmp.cpp -- the one-word gap-alignment sweeps (t1k_ga_matches_equal_w, t1k_ga_band_w<4>) against the int32 sweeps they
// replace (t1k_ga_matches_equal, t1k_ga_band<4, false>), compiled for the HOST under the address / undefined-behaviour sanitizers.
// tests/test_ga_core_cpu.py pastes the routines' text -- taken from t1k_amd/csrc/t1k_dev.h at test time, between the marker lines -- at the
// marker line below: device intrinsics are shimmed, everything else is the product's code.  Match count AND score must agree on every case
// within the one-word range; beyond it t1k_ga_count must return what the int32 sweeps return.  Signed overflow of a state word (a wrong
// range bound) is an error of its own under -fsanitize=undefined.
//   ga_core_cmp random <cases> <seed>     random pairs; prints "ok cases N inrange A beyond B offdiag C unequal D"
//   ga_core_cmp vectors <file>            lines "text<TAB>pattern<TAB>matches"; prints "ok vectors N"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <type_traits>
#include <vector>
#define __device__
#define __forceinline__ inline
#define T1K_EVEN 0x5555555555555555ull
static inline uint64_t t1k_get32(const uint64_t *w, int64_t pos) {
  int64_t wi = pos >> 5;
  int sh = (int)(pos & 31) * 2;
  return (w[wi] >> sh) | ((w[wi + 1] << 1) << (63 - sh));
}
static inline int t1k_base(const uint64_t *w, int64_t pos) { return (int)((w[pos >> 5] >> ((pos & 31) * 2)) & 3); }
static inline int t1k_bit(const uint64_t *w, int64_t pos) { return (int)((w[pos >> 5] >> ((pos & 31) * 2)) & 1); }
@@ROUTINE@@

struct Packed {  // one sequence at position `pos` of a stream of its own, random bases around it
  std::vector<uint64_t> b, n;
  int64_t pos;
  bool anyN = false;
  Packed(const std::string &s, int64_t at, std::mt19937_64 &rng) : b((at + s.size()) / 32 + 4), n((at + s.size()) / 32 + 4, 0), pos(at) {
    for (auto &w : b) w = rng();
    for (size_t i = 0; i < s.size(); ++i) {
      const int64_t p = at + (int64_t)i;
      const char c = s[i];
      const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
      b[p >> 5] &= ~(3ull << ((p & 31) * 2));
      if (code == 4) { n[p >> 5] |= 1ull << ((p & 31) * 2); anyN = true; } else b[p >> 5] |= (uint64_t)code << ((p & 31) * 2);
    }
  }
};

struct Result { int count, score; };
static Result oldRoutine(const T1kSeqView &T, int lt, const T1kSeqView &P, int lp) {
  Result r{0, 0};
  if (lt == lp) r.count = t1k_ga_matches_equal(T, P, lp, &r.score);
  else r.count = t1k_ga_band<4, false>(T, lt, P, lp, nullptr, 0, &r.score);
  return r;
}
static Result newRoutine(const T1kSeqView &T, int lt, const T1kSeqView &P, int lp) {
  Result r{0, 0};
  if (lt == lp) r.count = t1k_ga_matches_equal_w(T, P, lp, &r.score);
  else r.count = t1k_ga_band_w<4>(T, lt, P, lp, &r.score);
  return r;
}

// compares the routines on one pair; returns false (after printing the case) on a difference
static bool check(const std::string &text, const std::string &pat, int64_t tAt, int64_t pAt, std::mt19937_64 &rng, Result *out, bool *inRange) {
  Packed t(text, tAt, rng), p(pat, pAt, rng);
  const int lt = (int)text.size(), lp = (int)pat.size();
  T1kSeqView T{t.b.data(), t.n.data(), t.pos, t.anyN}, P{p.b.data(), p.n.data(), p.pos};   // a text without N is read without its mask
  T1kSeqView Tm{t.b.data(), t.n.data(), t.pos};
  const Result o = oldRoutine(Tm, lt, P, lp);
  *out = o;
  *inRange = t1k_ga_word_ok(lt, lp);
  Result g{0, 0};
  if (*inRange) {
    g = newRoutine(T, lt, P, lp);
    const Result g2 = newRoutine(Tm, lt, P, lp);   // and with the mask loaded
    if (g2.count != g.count || g2.score != g.score) g = Result{-1, -1};
  }
  Result d{0, 0};
  d.count = t1k_ga_count(T, lt, P, lp, &d.score);  // what the kernels call: either routine, by the range test
  const bool same = d.count == o.count && d.score == o.score && (!*inRange || (g.count == o.count && g.score == o.score));
  if (!same)
    printf("MISMATCH lt %d lp %d at %lld / %lld: int32 (%d, %d) one-word (%d, %d) dispatch (%d, %d)\n%s\n%s\n", lt, lp, (long long)tAt, (long long)pAt, o.count, o.score,
           g.count, g.score, d.count, d.score, text.c_str(), pat.c_str());
  return same;
}

static int ungappedScore(const std::string &a, const std::string &b) {
  int s = 0;
  for (size_t i = 0; i < a.size(); ++i) s += (a[i] == b[i] || a[i] == 'N' || b[i] == 'N') ? 2 : -2;
  return s;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::mt19937_64 rng(argc > 3 ? atoll(argv[3]) : 1);
  if (!strcmp(argv[1], "vectors")) {
    FILE *f = fopen(argv[2], "r");
    if (!f) return 2;
    static char line[1 << 16];
    long n = 0;
    while (fgets(line, sizeof line, f)) {
      char *t = strtok(line, "\t\n"), *p = strtok(nullptr, "\t\n"), *c = strtok(nullptr, "\t\n");
      if (!t || !p || !c) return 2;
      Result o; bool in;
      if (!check(t, p, (int64_t)(rng() % 70), (int64_t)(rng() % 70), rng, &o, &in)) return 1;
      if (o.count != atoi(c)) { printf("MISMATCH with the vector: %d, expected %s\n%s\n%s\n", o.count, c, t, p); return 1; }
      ++n;
    }
    fclose(f);
    printf("ok vectors %ld\n", n);
    return 0;
  }
  const long cases = atol(argv[2]);
  long inrange = 0, beyond = 0, offdiag = 0, unequal = 0;
  const char *ALPHA = "ACGT";
  for (long it = 0; it < cases; ++it) {
    // pattern length: mostly short (the boundary rows dominate), the whole range, and both sides of the one-word bound (510 for equal lengths)
    const unsigned pick = (unsigned)(rng() % 100);
    int lp = pick < 55 ? 2 + (int)(rng() % 79) : pick < 85 ? 2 + (int)(rng() % 499) : 504 + (int)(rng() % 12);
    const int d = (rng() % 3) == 0 ? 0 : (int)(rng() % 9) - 4;
    const bool twoLetter = (rng() % 5) == 0;  // two-letter sequences: many equal-score paths, the tie order decides
    const int subPct = (int)(rng() % 26);     // 0 .. 25 % substitutions
    std::string pat(lp, 'A');
    for (auto &c : pat) c = twoLetter ? "AC"[rng() & 1] : ALPHA[rng() & 3];
    // the text: the pattern with substitutions and indels, then trimmed or extended to the wanted length
    std::string text;
    const int nIndel = (int)(rng() % 4);
    std::vector<int> indelAt(nIndel);
    for (auto &x : indelAt) x = (int)(rng() % lp);
    for (int i = 0; i < lp; ++i) {
      bool skip = false;
      for (int x : indelAt)
        if (x == i) { if (rng() & 1) skip = true; else text.push_back(twoLetter ? "AC"[rng() & 1] : ALPHA[rng() & 3]); }
      if (skip) continue;
      char c = pat[i];
      if ((int)(rng() % 100) < subPct) c = twoLetter ? "AC"[rng() & 1] : ALPHA[rng() & 3];
      text.push_back(c);
    }
    int lt = lp + d;
    if (lt < 1) lt = 1;
    if (lt == lp && lp < 2) lt = lp = 2;
    while ((int)text.size() < lt) text.push_back(twoLetter ? "AC"[rng() & 1] : ALPHA[rng() & 3]);
    text.resize(lt);
    if ((int)pat.size() != lp) pat.resize(lp, 'A');
    if ((rng() % 6) == 0) text[rng() % lt] = 'N';
    if ((rng() % 6) == 0) pat[rng() % lp] = 'N';
    if ((rng() % 40) == 0) for (int k = 0; k < 6; ++k) { text[rng() % lt] = 'N'; pat[rng() % lp] = 'N'; }
    Result o; bool in;
    if (!check(text, pat, (int64_t)(rng() % 70), (int64_t)(rng() % 70), rng, &o, &in)) return 1;
    if (in) ++inrange; else ++beyond;
    if (lt != lp) ++unequal;
    else if (o.score > ungappedScore(text, pat)) ++offdiag;  // the optimum of an equal-length pair leaves the diagonal
  }
  printf("ok cases %ld inrange %ld beyond %ld offdiag %ld unequal %ld\n", cases, inrange, beyond, offdiag, unequal);
  return 0;
}
