// t1k_amd/csrc/host/bootstrap.cpp -- genotyper --bootstrap: the driver of the replicates' EMs.  The SQUAREM steps, the masking
// rule and the table are genotype.cpp's (plain host code); what calls the device lives here, so that genotype.cpp stays buildable with the EM's
// entry points alone.
#include <cmath>
#include <cstdlib>
#include <thread>
#include "t1k_host.h"

#include <chrono>

namespace {
double hostNowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// fn(r) for every replicate r < n on the host threads (the replicates' host steps are independent of each other)
template <class F>
void forReplicates(size_t n, F fn) {
  unsigned T = std::thread::hardware_concurrency();
  if (T > 32) T = 32;
  if (T < 2 || n < 2) { for (size_t i = 0; i < n; ++i) fn(i); return; }
  std::vector<std::thread> th;
  const size_t chunk = (n + T - 1) / T;
  for (unsigned t = 0; t < T; ++t) {
    const size_t b = t * chunk, e = std::min(n, b + chunk);
    if (b >= e) break;
    th.emplace_back([b, e, &fn] { for (size_t i = b; i < e; ++i) fn(i); });
  }
  for (auto &x : th) x.join();
}
}  // namespace

namespace t1k {

extern "C" void t1k_em_times(const t1k_ctx *ctx, double *ms4);  // (t1k_em.hip: debug clocks of the updates)
int Genotyper::bootstrap(t1k_ctx *ctx, int B, uint64_t seed, BootResult &out, std::string &err) const {
  const double t0 = hostNowMs();
  const RefSet &R = *ref;
  const size_t E = ecAlleles.size(), G = nGroups(), A = R.al.size(), nRep = (size_t)B + 1;
  const bool serial = getenv("T1K_BOOTSTRAP_SERIAL") && atoi(getenv("T1K_BOOTSTRAP_SERIAL")) != 0;
  const bool identity = getenv("T1K_BOOTSTRAP_IDENTITY") && atoi(getenv("T1K_BOOTSTRAP_IDENTITY")) != 0;
  out = BootResult();
  out.B = B; out.nAlleles = A; out.serial = serial;
  out.abundance.assign(nRep * A, 0.0);
  out.rounds.assign(nRep, 0);
  out.valid.assign(nRep, 0);
  if (emEcLen.size() != E || emCount.size() != G) { err = "bootstrap: quantify has not run"; return -1; }
  auto fail = [&] { err = t1k_last_error(ctx); t1k_boot_end(ctx); return -1; };
  if (t1k_boot_begin(ctx, (uint32_t)B, seed, identity ? 1 : 0) != T1K_OK) return fail();
  const size_t Rpad = t1k_boot_stride((uint32_t)B);
  std::vector<uint8_t> nonEmpty(Rpad, 0);
  if (t1k_boot_nonempty(ctx, nonEmpty.data()) != T1K_OK) return fail();
  std::vector<double> start(E);  // quantify's start vector
  for (size_t e = 0; e < E; ++e) {
    start[e] = 0;
    for (int a : ecAlleles[e]) start[e] += R.al[a].weight;
  }
  const std::function<void(EmRun &)> mask = [this](EmRun &run) { maskInto(run); };
  auto finish = [&](size_t r, const EmRun &run) {  // the abundances a run ends with (quantify's last setAbundance)
    Abundances ab;
    abundanceInto(run.n, run.stride, ab);
    bool finite = true;
    for (size_t a = 0; a < A; ++a) { out.abundance[r * A + a] = ab.abundance[a]; finite = finite && std::isfinite(ab.abundance[a]); }
    out.rounds[r] = run.rounds;
    out.valid[r] = finite ? 1 : 0;
  };
  if (!serial) {
    std::vector<double> x0(E * Rpad, 0.0), x1(E * Rpad, 0.0), x2(E * Rpad, 0.0), x3(E * Rpad, 0.0), n(E * Rpad, 0.0), diff(Rpad, 0.0);
    std::vector<EmRun> runs(nRep);
    std::vector<uint8_t> active(Rpad, 0);
    size_t nActive = 0;
    for (size_t r = 0; r < nRep; ++r) {
      EmRun &run = runs[r];
      run.x0 = x0.data() + r; run.x1 = x1.data() + r; run.x2 = x2.data() + r; run.x3 = x3.data() + r; run.n = n.data() + r;
      run.stride = Rpad;
      for (size_t e = 0; e < E; ++e) x0[e * Rpad + r] = start[e];
      active[r] = nonEmpty[r];
      nActive += active[r];
    }
    auto update = [&](std::vector<double> &from, std::vector<double> &to) {
      ++out.updates;
      return t1k_boot_update(ctx, active.data(), from.data(), to.data(), n.data(), diff.data()) == T1K_OK;
    };
    // the replicates run in lockstep: all active ones are at the same step of their own round; one that is done goes inactive
    while (nActive) {
      if (!update(x0, x1) || !update(x1, x2)) return fail();
      forReplicates(nRep, [&](size_t r) { if (active[r]) emExtrapolate(runs[r]); });
      if (!update(x3, x1)) return fail();
      forReplicates(nRep, [&](size_t r) { if (active[r]) emCloseRound(runs[r], mask); });
      for (size_t r = 0; r < nRep; ++r)
        if (active[r] && runs[r].done) { active[r] = 0; --nActive; }
    }
    forReplicates(nRep, [&](size_t r) { if (nonEmpty[r]) finish(r, runs[r]); });
    double ms[3];
    t1k_boot_times(ctx, ms);
    out.rowMs = ms[0]; out.colMs = ms[1]; out.kernelMs = ms[0] + ms[1];
  } else {
    // the slow, obviously right way and the timing baseline: today's kernels, one replicate after the other
    std::vector<double> counts(G * Rpad);
    if (t1k_boot_counts(ctx, nullptr, counts.data()) != T1K_OK) return fail();
    if (t1k_em_shard(ctx, 0, (uint32_t)G, nullptr) != T1K_OK) return fail();  // (a rank of a sharded job: the whole row pass, no collective)
    double u0[4], u1[4];
    t1k_em_times(ctx, u0);
    std::vector<double> x0(E), x1(E), x2(E), x3(E), n(E), mine(G);
    for (size_t r = 0; r < nRep; ++r) {
      if (!nonEmpty[r]) continue;
      for (size_t g = 0; g < G; ++g) mine[g] = counts[g * Rpad + r];
      if (t1k_em_set_count(ctx, mine.data()) != T1K_OK) return fail();
      EmRun run;
      run.x0 = x0.data(); run.x1 = x1.data(); run.x2 = x2.data(); run.x3 = x3.data(); run.n = n.data();
      x0 = start;
      std::fill(n.begin(), n.end(), 0.0);
      double diff = 0;
      auto em = [&](std::vector<double> &from, std::vector<double> &to) {
        ++out.updates;
        return E == 0 || t1k_em_update(ctx, from.data(), to.data(), n.data(), &diff) == T1K_OK;
      };
      while (!run.done) {
        if (!em(x0, x1) || !em(x1, x2)) return fail();
        emExtrapolate(run);
        if (!em(x3, x1)) return fail();
        emCloseRound(run, mask);
      }
      finish(r, run);
    }
    if (t1k_em_set_count(ctx, emCount.data()) != T1K_OK) return fail();  // the job's own counts again
    t1k_em_times(ctx, u1);
    out.kernelMs = u1[1] - u0[1];  // (waiting for the device: the two kernels and the copy back)
  }
  t1k_boot_end(ctx);
  out.totalMs = hostNowMs() - t0;
  return 0;
}

}  // namespace t1k
