// tests/harness/boot_host_harness.cpp -- TEST INFRASTRUCTURE (CPU): the host side of genotyper --bootstrap (t1k_amd/csrc/host/genotype.cpp,
// plain C++) on tables written by hand, for tests/test_boot_cpu.py to compare with the restatement tests/boot_ref.py:
//   text   Genotyper::calledSeries + bootstrapText on a replicate matrix                          -> the table on stdout
//   em     the SQUAREM step functions (emExtrapolate, emCloseRound, maskInto, abundanceInto) around a plain E-step + M-step written here
//          (Genotyper::EMupdate: the device stage is not run) -> "rounds", then ecReadCount and the per-allele abundances as hex doubles
// Input: one file of whitespace-separated tokens (doubles as C hex floats):
//   frac nGenes nSeries nAlleles | gene names | series names | per allele: series gene ec effLen weight | mode ...
//   text: B | per gene: k, then k x (allele rank quality) | valid[B + 1] | matrix[(B + 1)][nAlleles]
//   em:   G | rowPtr[G + 1] | ecIdx[nnz] | count[G]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "../../t1k_amd/csrc/host/t1k_host.h"

// Genotyper::quantify drives the device E-step; this harness never calls it
extern "C" {
int t1k_em_setup(t1k_ctx *, const uint64_t *, const uint32_t *, const double *, const int32_t *, uint32_t, uint32_t, t1k_allreduce_fn, void *) { abort(); }
int t1k_em_update(t1k_ctx *, const double *, double *, double *, double *) { abort(); }
int t1k_em_shard(t1k_ctx *, uint32_t, uint32_t, t1k_comm *) { abort(); }
void t1k_em_times(const t1k_ctx *, double *) { abort(); }
int t1k_comm_size(const t1k_comm *) { abort(); }
int t1k_comm_rank(const t1k_comm *) { abort(); }
const char *t1k_last_error(const t1k_ctx *) { return "no device in this harness"; }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: boot_host_harness input\n"); return 2; }
  std::ifstream f(argv[1]);
  auto word = [&] { std::string s; if (!(f >> s)) { fprintf(stderr, "input ends early\n"); exit(1); } return s; };
  auto num = [&] { return strtod(word().c_str(), nullptr); };
  auto integer = [&] { return atol(word().c_str()); };
  t1k::RefSet R;
  t1k::Genotyper gt;
  gt.ref = &R;
  gt.prm = t1k_job_params();  // (squarem_min_alpha 0: no lower limit on alpha, the executable's default)
  gt.prm.filter_frac = num();
  const long nGenes = integer(), nSeries = integer(), A = integer();
  for (long g = 0; g < nGenes; ++g) R.geneName.push_back(word());
  for (long m = 0; m < nSeries; ++m) R.majorName.push_back(word());
  R.al.resize(A);
  int E = 0;
  for (long a = 0; a < A; ++a) {
    t1k::AlleleMeta &m = R.al[a];
    m.name = "a" + std::to_string(a);
    m.major = (int)integer(); m.gene = (int)integer(); m.ec = (int)integer(); m.effLen = (int)integer(); m.weight = (int)integer();
    E = std::max(E, m.ec + 1);
  }
  gt.ecAlleles.assign(E, {});
  for (long a = 0; a < A; ++a)
    if (R.al[a].ec >= 0) gt.ecAlleles[R.al[a].ec].push_back((int)a);
  gt.emEcLen.assign(E, 0);
  for (int e = 0; e < E; ++e) {
    int len = R.al[gt.ecAlleles[e][0]].effLen;
    for (int a : gt.ecAlleles[e]) len = std::min(len, R.al[a].effLen);
    gt.emEcLen[e] = len;
  }
  const std::string mode = word();
  if (mode == "text") {
    t1k::Genotyper::BootResult boot;
    boot.B = (int)integer();
    boot.nAlleles = (size_t)A;
    gt.selected.assign(nGenes, {});
    for (long g = 0; g < nGenes; ++g) {
      const long k = integer();
      for (long i = 0; i < k; ++i) {
        const int a = (int)integer(), rank = (int)integer(), quality = (int)integer();
        gt.selected[g].push_back({a, rank});
        R.al[a].rank = rank; R.al[a].quality = quality;
      }
    }
    for (int r = 0; r <= boot.B; ++r) boot.valid.push_back((uint8_t)integer());
    for (long i = 0; i < (boot.B + 1) * A; ++i) boot.abundance.push_back(num());
    boot.rounds.assign(boot.B + 1, 0);
    // the abundances of the job's own quantify: replicate 0 (SetAlleleAbundance's sums)
    for (long a = 0; a < A; ++a) R.al[a].abundance = boot.abundance[a];
    gt.setAbundance(nullptr, gt.emEcLen);
    fputs(gt.bootstrapText(boot).c_str(), stdout);
    return 0;
  }
  if (mode != "em") { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
  const long G = integer();
  std::vector<uint64_t> rowPtr(G + 1);
  for (auto &v : rowPtr) v = (uint64_t)integer();
  std::vector<uint32_t> ecIdx(rowPtr[G]);
  for (auto &v : ecIdx) v = (uint32_t)integer();
  std::vector<double> count(G);
  for (auto &v : count) v = num();
  std::vector<double> x0(E), x1(E), x2(E), x3(E), n(E);
  for (int e = 0; e < E; ++e) {
    x0[e] = 0;
    for (int a : gt.ecAlleles[e]) x0[e] += R.al[a].weight;
  }
  auto em = [&](const std::vector<double> &from, std::vector<double> &to) {  // Genotyper::EMupdate (372-421)
    std::fill(n.begin(), n.end(), 0.0);
    for (long g = 0; g < G; ++g) {
      double psum = 0;
      for (uint64_t p = rowPtr[g]; p < rowPtr[g + 1]; ++p) psum += from[ecIdx[p]];
      if (psum == 0) psum = 1;
      for (uint64_t p = rowPtr[g]; p < rowPtr[g + 1]; ++p) n[ecIdx[p]] += count[g] * (from[ecIdx[p]] / psum);
    }
    double norm = 0;
    for (int e = 0; e < E; ++e) norm += n[e] / gt.emEcLen[e];
    for (int e = 0; e < E; ++e) to[e] = n[e] / gt.emEcLen[e] / norm;
  };
  t1k::Genotyper::EmRun run;
  run.x0 = x0.data(); run.x1 = x1.data(); run.x2 = x2.data(); run.x3 = x3.data(); run.n = n.data();
  const std::function<void(t1k::Genotyper::EmRun &)> mask = [&](t1k::Genotyper::EmRun &r) { gt.maskInto(r); };
  while (!run.done) {
    em(x0, x1);
    em(x1, x2);
    gt.emExtrapolate(run);
    em(x3, x1);
    gt.emCloseRound(run, mask);
  }
  t1k::Genotyper::Abundances ab;
  gt.abundanceInto(n.data(), 1, ab);
  printf("%d\n", run.rounds);
  for (int e = 0; e < E; ++e) printf("%a\n", n[e]);
  for (long a = 0; a < A; ++a) printf("%a\n", ab.abundance[a]);
  return 0;
}
