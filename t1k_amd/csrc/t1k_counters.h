// t1k_amd/csrc/t1k_counters.h -- internal: the layout of the counter block (ctx->bCounters, T1K_COUNTER_WORDS 64-bit words), through which
// the assign pipeline and the pairing stage talk to the host.  Kernels and host index the block with the names below and nothing else.
//
//   [0, T1K_CTR_WORDS)              control words: cursors, the error word, hand-out words, statistics, measurement windows
//   [T1K_STAT_BASE, T1K_ARENA_BASE) the striped statistics: T1K_STAT_STRIPES stripes of T1K_STAT_KINDS words (t1k_stat_add); the host
//                                   folds them into control words (t1k_stat_slot)
//   [T1K_ARENA_BASE, T1K_TOTAL_BASE) the arena cursors: one per (arena, stripe), T1K_STRIPE_WORDS apart; they count past the capacity
//   [T1K_TOTAL_BASE, ...)           per arena the length of its dense list (k_arena_compact)
//
// The two stages share the block and REUSE control words: t1k_assign_range clears the whole block before every pass, the pairing launcher
// clears its own words (T1K_PCTR_*) before every launch pair, and neither reads the other's.  Words 22 and 24 mean different things in the
// two stages (below).  A new control word takes a number no enum of its stage holds; the static_asserts keep a stage's words apart.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#define T1K_CTR_WORDS 64  // control words in front of the statistics stripes

// ---- the assign pipeline (seeding .. selection, full alignments, truncation).  "host:" = written by the host into its copy only.
enum {
  T1K_CTR_CAND = 0,             // k_collect's candidate cursor: the demand when it passes cand_cap
  T1K_CTR_OVL = 1,              // overlaps kept (the selection's cursor: the demand when it passes ovl_cap)
  T1K_CTR_ERR = 2,              // the error word (ERR_* below); pairing uses the same word with its own bits
  T1K_CTR_LOOKUPS = 3,          // host: folded T1K_STAT_LOOKUPS
  T1K_CTR_POSTINGS = 4,         // host: folded T1K_STAT_POSTINGS
  T1K_CTR_HITS = 5,             // host: folded T1K_STAT_HITS
  T1K_CTR_GROUPS = 6,           // host: sum of the group arena's cursors
  T1K_CTR_DP = 7,               // k_chain_big's alignments + host: folded T1K_STAT_DP
  T1K_CTR_EQ_JOBS = 8,          // host: equal-span alignment queue (t1k_fullalign_phase)
  T1K_CTR_NEARBEST = 10,        // host: folded T1K_STAT_NEARBEST
  T1K_CTR_FAST = 11,            // host: folded T1K_STAT_FAST
  T1K_CTR_GENERAL = 12,         // host: folded T1K_STAT_GENERAL
  T1K_CTR_BIG_GROUPS = 13,      // groups k_chain_big chained
  T1K_CTR_EXTEND_DP = 14,       // host: folded T1K_STAT_EXTEND_DP
  T1K_CTR_BAND_JOBS = 15,       // host: band alignment queue
  T1K_CTR_JOB_TOTAL = 16,       // host (t1k_run_chain): memo jobs
  T1K_CTR_RETRY_TOTAL = 17,     // host: parked groups
  T1K_CTR_GENERAL_TOTAL = 18,   // host: multi-diagonal groups
  T1K_CTR_BIG_TOTAL = 19,       // host: big-scratch list
  T1K_CTR_WIDE_JOBS = 20,       // host: wide alignment queue
  T1K_CTR_EMITTED = 21,         // overlaps the packed selection emitted before the cut
  T1K_CTR_FINISH_TOTAL = 22,    // host: finish list (pairing: T1K_PCTR_OVERLAPS)
  T1K_CTR_DP_CELLS = 24,        // DP cells of the traced alignments (pairing: T1K_PCTR_BIG_CURSOR)
  T1K_CTR_COLLECT_HANDOUT = 27, // next read-end of k_collect
  T1K_CTR_TRUNC_HANDOUT = 30,   // next read-end of k_truncate: + 0 the 256-thread shape, + 1 the 1024-thread shape
  T1K_CTR_SELECT_HANDOUT = 56,  // + size class (3): next list position of the selection's launch
  T1K_CTR_SELECT_LEN = 59,      // + size class (3): length of the class's list (k_select_classes)
};
// ---- pairing (k_pair's two launches).  Its launcher clears exactly these words before every attempt.
enum {
  T1K_PCTR_ERR = T1K_CTR_ERR,   // PAIR_ERR_* below
  T1K_PCTR_ROWS = 9,            // row cursor / rows written
  T1K_PCTR_OVERLAPS = 22,       // overlap records read (statistic); assign: T1K_CTR_FINISH_TOTAL
  T1K_PCTR_LONG = 23,           // fragments left to the second launch
  T1K_PCTR_BIG_CURSOR = 24,     // their cursor in the big arena, counts past its capacity; assign: T1K_CTR_DP_CELLS
  T1K_PCTR_HANDOUT = 25,        // next fragment: + 0 the first launch, + 1 the second
  T1K_PCTR_CLEAR_FIRST = T1K_PCTR_OVERLAPS, T1K_PCTR_CLEAR_WORDS = 5,  // 22 .. 26 are cleared with one memset
};
// ---- measurement windows: {base, length}, written only by builds with the macro named
enum {
  T1K_WIN_PAIR_PROFILE = 32, T1K_WIN_PAIR_PROFILE_LEN = 8,    // -DT1K_PAIR_PROFILE: k_pair's phase clocks
  T1K_WIN_SEED_PROFILE = 48, T1K_WIN_SEED_PROFILE_LEN = 8,    // -DT1K_SEED_PROFILE: k_seed_groups' phase clocks
  T1K_WIN_SELECT_ROUTES = 40, T1K_WIN_SELECT_ROUTES_LEN = 12, // -DT1K_SELECT_ROUTES: 6 routes x (read-ends, candidates); route 0 by k_select_classes
  T1K_WIN_PAIR_ROUTES = 40, T1K_WIN_PAIR_ROUTES_LEN = 12,     // -DT1K_PAIR_ROUTES: 6 routes x (fragments, records); cleared by the pairing launcher
  T1K_WIN_NEAR_STATS = 40, T1K_WIN_NEAR_STATS_LEN = 8,        // -DT1K_NEAR_STATS: classes of the multi-diagonal groups
  T1K_WIN_WALK_STATS = 40, T1K_WIN_WALK_STATS_LEN = 3,        // -DT1K_WALK_STATS: classes of the gap walk
};
// classes of T1K_NEAR_STATS, as offsets into its window
enum { T1K_NEAR_FAR = 0, T1K_NEAR_SATURATED = 1, T1K_NEAR_FALLBACK = 2, T1K_NEAR_NOCHAIN_SMALL = 3, T1K_NEAR_CHAIN_SMALL = 5, T1K_NEAR_CHAIN_LARGE = 6, T1K_NEAR_NOCHAIN_LARGE = 7 };
// The three windows of the assign pipeline at word 40 are one build each, and the selection's routes reach into the seed profile:
#if defined(T1K_SELECT_ROUTES) + defined(T1K_NEAR_STATS) + defined(T1K_WALK_STATS) > 1
#error "T1K_SELECT_ROUTES, T1K_NEAR_STATS and T1K_WALK_STATS count in the same control words: one of them per build"
#endif
#if defined(T1K_SELECT_ROUTES) && defined(T1K_SEED_PROFILE)
#error "the window of T1K_SELECT_ROUTES overlaps the seed profile's: one of them per build"
#endif

constexpr int T1K_ASSIGN_CTR[] = {T1K_CTR_CAND, T1K_CTR_OVL, T1K_CTR_ERR, T1K_CTR_LOOKUPS, T1K_CTR_POSTINGS, T1K_CTR_HITS, T1K_CTR_GROUPS, T1K_CTR_DP, T1K_CTR_EQ_JOBS,
                                  T1K_CTR_NEARBEST, T1K_CTR_FAST, T1K_CTR_GENERAL, T1K_CTR_BIG_GROUPS, T1K_CTR_EXTEND_DP, T1K_CTR_BAND_JOBS, T1K_CTR_JOB_TOTAL,
                                  T1K_CTR_RETRY_TOTAL, T1K_CTR_GENERAL_TOTAL, T1K_CTR_BIG_TOTAL, T1K_CTR_WIDE_JOBS, T1K_CTR_EMITTED, T1K_CTR_FINISH_TOTAL, T1K_CTR_DP_CELLS,
                                  T1K_CTR_COLLECT_HANDOUT, T1K_CTR_TRUNC_HANDOUT, T1K_CTR_TRUNC_HANDOUT + 1, T1K_CTR_SELECT_HANDOUT, T1K_CTR_SELECT_HANDOUT + 1,
                                  T1K_CTR_SELECT_HANDOUT + 2, T1K_CTR_SELECT_LEN, T1K_CTR_SELECT_LEN + 1, T1K_CTR_SELECT_LEN + 2};
constexpr int T1K_PAIR_CTR[] = {T1K_PCTR_ERR, T1K_PCTR_ROWS, T1K_PCTR_OVERLAPS, T1K_PCTR_LONG, T1K_PCTR_BIG_CURSOR, T1K_PCTR_HANDOUT, T1K_PCTR_HANDOUT + 1};
template <int N>
constexpr bool t1k_ctr_apart(const int (&w)[N]) {  // inside the control words, no two the same
  for (int i = 0; i < N; ++i) {
    if (w[i] < 0 || w[i] >= T1K_CTR_WORDS) return false;
    for (int j = 0; j < i; ++j) if (w[i] == w[j]) return false;
  }
  return true;
}
template <int N>
constexpr bool t1k_ctr_window_free(const int (&w)[N], int base, int len) {  // inside the control words, on none of the stage's
  if (base < 0 || base + len > T1K_CTR_WORDS) return false;
  for (int i = 0; i < N; ++i) if (w[i] >= base && w[i] < base + len) return false;
  return true;
}
static_assert(t1k_ctr_apart(T1K_ASSIGN_CTR), "two control words of the assign pipeline collide");
static_assert(t1k_ctr_apart(T1K_PAIR_CTR), "two control words of pairing collide");
static_assert(T1K_PCTR_CLEAR_FIRST == T1K_PCTR_OVERLAPS && T1K_PCTR_LONG == T1K_PCTR_OVERLAPS + 1 && T1K_PCTR_BIG_CURSOR == T1K_PCTR_OVERLAPS + 2 &&
              T1K_PCTR_HANDOUT == T1K_PCTR_OVERLAPS + 3 && T1K_PCTR_CLEAR_WORDS == 5, "the pairing launcher clears words 22 .. 26 with one memset");
static_assert(t1k_ctr_window_free(T1K_ASSIGN_CTR, T1K_WIN_SEED_PROFILE, T1K_WIN_SEED_PROFILE_LEN), "seed profile on a control word");
static_assert(t1k_ctr_window_free(T1K_ASSIGN_CTR, T1K_WIN_SELECT_ROUTES, T1K_WIN_SELECT_ROUTES_LEN), "selection routes on a control word");
static_assert(t1k_ctr_window_free(T1K_ASSIGN_CTR, T1K_WIN_NEAR_STATS, T1K_WIN_NEAR_STATS_LEN), "near statistics on a control word");
static_assert(t1k_ctr_window_free(T1K_ASSIGN_CTR, T1K_WIN_WALK_STATS, T1K_WIN_WALK_STATS_LEN), "gap-walk statistics on a control word");
static_assert(t1k_ctr_window_free(T1K_PAIR_CTR, T1K_WIN_PAIR_PROFILE, T1K_WIN_PAIR_PROFILE_LEN), "pair profile on a control word");
static_assert(t1k_ctr_window_free(T1K_PAIR_CTR, T1K_WIN_PAIR_ROUTES, T1K_WIN_PAIR_ROUTES_LEN), "pair routes on a control word");
// (the selection's route 0 is written by k_select_classes with a plain store, in builds with T1K_SELECT_ROUTES only: it is the first word of
// that build's own window, which the assert above keeps off every control word)

// ---- statistics stripes: counters whose value only the end-of-batch report reads.  Every workgroup adds to the stripe of its index.
#define T1K_STAT_STRIPES 256
#define T1K_STAT_KINDS 8
#define T1K_STAT_BASE T1K_CTR_WORDS
enum { T1K_STAT_DP = 0, T1K_STAT_FAST = 1, T1K_STAT_GENERAL = 2, T1K_STAT_EXTEND_DP = 3, T1K_STAT_NEARBEST = 4, T1K_STAT_LOOKUPS = 5, T1K_STAT_POSTINGS = 6, T1K_STAT_HITS = 7 };
constexpr int t1k_stat_slot(int kind) {  // the control word t1k_fetch_counters folds a statistic into
  switch (kind) {
    case T1K_STAT_DP: return T1K_CTR_DP;
    case T1K_STAT_FAST: return T1K_CTR_FAST;
    case T1K_STAT_GENERAL: return T1K_CTR_GENERAL;
    case T1K_STAT_EXTEND_DP: return T1K_CTR_EXTEND_DP;
    case T1K_STAT_NEARBEST: return T1K_CTR_NEARBEST;
    case T1K_STAT_LOOKUPS: return T1K_CTR_LOOKUPS;
    case T1K_STAT_POSTINGS: return T1K_CTR_POSTINGS;
    case T1K_STAT_HITS: return T1K_CTR_HITS;
  }
  return -1;
}

// ---- arenas: striped work lists; the cursors keep counting past a stripe's capacity, which is how the host sees the demand
#define T1K_NSTRIPE 32
enum { T1K_AR_GROUPS = 0, T1K_AR_JOBS, T1K_AR_RETRY, T1K_AR_FINISH, T1K_AR_GENERAL, T1K_AR_BIG, T1K_AR_GENCAND, T1K_AR_EQ, T1K_AR_BAND, T1K_AR_WIDE, T1K_AR_GENHITS, T1K_AR_GENJOBS, T1K_AR_WAVE, T1K_AR_EXTJOBS, T1K_AR_EXTRETRY, T1K_AR_SLOW, T1K_NARENA };
#define T1K_ARENA_BASE (T1K_STAT_BASE + T1K_STAT_STRIPES * T1K_STAT_KINDS)
#ifndef T1K_STRIPE_WORDS
#define T1K_STRIPE_WORDS 8   // 64-bit words between the cursors of two stripes of an arena (8: 64 bytes apart; 16: a 128-byte cache line each)
#endif
// behind the cursors: one word per arena = the number of entries of its DENSE list (sum over the stripes of min(cursor, segCap)), written by
// k_arena_compact where it makes the list dense -- the list's consumers read their item count there instead of from a launch argument, so
// the host does not have to fetch the cursors between a producer and its consumers (t1k_run_chain: one counter fetch per range)
#define T1K_TOTAL_BASE (T1K_ARENA_BASE + T1K_NARENA * T1K_NSTRIPE * T1K_STRIPE_WORDS)
#define T1K_COUNTER_WORDS (T1K_TOTAL_BASE + ((T1K_NARENA + 7) & ~7))
// an arena's cursors in a fetched block (ctx->hRaw): one stripe's, the fullest stripe's, their sum
inline unsigned long long t1k_cursor(const std::vector<unsigned long long> &raw, int arena, int stripe) {
  return raw[T1K_ARENA_BASE + ((size_t)arena * T1K_NSTRIPE + stripe) * T1K_STRIPE_WORDS];
}
inline unsigned long long t1k_cursor_max(const std::vector<unsigned long long> &raw, int arena) {
  unsigned long long m = 0;
  for (int s = 0; s < T1K_NSTRIPE; ++s) m = m > t1k_cursor(raw, arena, s) ? m : t1k_cursor(raw, arena, s);
  return m;
}
inline unsigned long long t1k_cursor_sum(const std::vector<unsigned long long> &raw, int arena) {
  unsigned long long t = 0;
  for (int s = 0; s < T1K_NSTRIPE; ++s) t += t1k_cursor(raw, arena, s);
  return t;
}

// ---- the error word.  Assign pipeline:
enum { ERR_HITCAP = 1, ERR_STAGECAP = 2, ERR_CANDCAP = 4, ERR_BIGGROUP = 8, ERR_OVLCAP = 16, ERR_SORTCAP = 32, ERR_SLOWCAP = 64, ERR_ROWCAP = 128, ERR_GROUPCAP = 256,
       ERR_MEMO = 512,     // an alignment memo entry was left pending (internal, unless a full job list explains it: ERR_GROUPCAP drops it)
       ERR_PACK = 1024 };  // a record does not fit the packed form of the overlap store (internal)
// pairing writes two bits of its own into the same word:
enum { PAIR_ERR_ROWS = 128,        // row_cap, the rowset's chunk or a fragment's scratch is full (the value of ERR_ROWCAP)
       PAIR_ERR_BIGARENA = 1024 }; // the big arena is too small: the launcher grows it to T1K_PCTR_BIG_CURSOR and runs the call again
// the arenas whose overflow t1k_assign_range answers by growing a working capacity and running the range again
constexpr unsigned long long ERR_RETRYABLE = ERR_GROUPCAP | ERR_CANDCAP | ERR_OVLCAP | ERR_SLOWCAP | ERR_STAGECAP;
// the capacity bits and their words in the T1K_ERR_CAPACITY message, in the message's order
struct T1kErrName { unsigned long long bit; const char *text; };
constexpr T1kErrName T1K_CAPACITY_NAMES[] = {{ERR_HITCAP, " hit_cap"}, {ERR_STAGECAP, " candidate staging"}, {ERR_CANDCAP, " cand_cap"}, {ERR_BIGGROUP, " group too large"},
                                             {ERR_OVLCAP, " ovl_cap"}, {ERR_SORTCAP, " sort capacity"}, {ERR_SLOWCAP, " slow-alignment queue"}, {ERR_ROWCAP, " row_cap"},
                                             {ERR_GROUPCAP, " group_cap"}};
constexpr unsigned long long t1k_capacity_bits() {
  unsigned long long m = 0;
  for (const T1kErrName &e : T1K_CAPACITY_NAMES) m |= e.bit;
  return m;
}
static_assert((t1k_capacity_bits() | ERR_MEMO | ERR_PACK) == 2 * ERR_PACK - 1 && !(t1k_capacity_bits() & (ERR_MEMO | ERR_PACK)), "every bit of the error word is a named capacity or a named internal error");
static_assert(!(ERR_RETRYABLE & ~t1k_capacity_bits()), "only capacities are grown");
inline std::string t1k_capacity_message(unsigned long long flags) {
  std::string m = "device arena overflow:";
  for (const T1kErrName &e : T1K_CAPACITY_NAMES) if (flags & e.bit) m += e.text;
  return m;
}
