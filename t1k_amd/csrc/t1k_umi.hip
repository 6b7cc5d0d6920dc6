// t1k_amd/csrc/t1k_umi.hip -- UMI collapse of the per-barcode allele lists (analyzer --umi): fragments become molecules
// and the per-barcode table counts molecules.
//
// Everything is a sort, a run table or a lane per item; no float atomic, no order of arrival in any result:
//   k_umi_keys     a lane per fragment: key = bucket << 32 | code, bucket = ((row * nGenes + gene) << 4) | (length - 1); all ones = no UMI
//   sort           t1k_sort_pairs over the 64 bits (stable, value = the fragment)
//   run table      t1k_run_table (t1k_sort.hip): the distinct UMIs of every bucket in code order, their first position (counts are
//                  differences of consecutive starts).  A fragment without a UMI is a run of its own (the table's lone key).
//   k_umi_parent   a lane per distinct UMI: its bucket's range by two binary searches, then its 3 * L neighbours by binary search inside
//                  that range; writes its own parent only, from counts nobody changes
//   k_umi_root     a lane per distinct UMI follows the parents (read only)
//   sort           by root index (stable): the fragments of a key are consecutive; second run table = the keys
//   k_umi_mol      a lane per key, run twice: <false> sizes its molecules (one with the intersection, or one per distinct list when the
//                  intersection is empty), exclusive scans place them, <true> writes them
//   k_umi_triples  a lane per molecule: (row * nAlleles + allele) << nb | |S_m| for every allele of its list; sort; third run table =
//                  K(r, a, n) as run lengths, n ascending inside a cell
//   k_umi_table    the lane of a cell's first run adds (double)K / (double)n over its runs, in that order
// One kernel shape each: keys and molecules are a few fragments long (a UMI is a molecule), so a lane per key is the whole story; a key
// of n fragments whose intersection is empty costs its lane n * n list comparisons.
#include <algorithm>
#include <cstring>
#include "t1k_dev.h"
#include "t1k_launch.h"

static constexpr unsigned long long kNoUmi = ~0ull;
enum { UMI_C_CORRECTED = 0, UMI_C_SPLIT = 1, UMI_C_NOUMI = 2, UMI_C_WORDS = 4 };

struct UmiArgs {
  // input (lists rebased to the slice)
  const uint32_t *row, *listPtr, *list, *gene;
  const unsigned long long *umi;
  uint32_t nFrag, nGenes, nAlleles, mismatch;
  // sorting
  unsigned long long *keyA, *keyB;
  uint32_t *valA, *valB;
  // run tables (one after the other: distinct UMIs, keys, (cell, n) runs)
  uint32_t *flag, *scan, *runStart;
  unsigned long long *runKey;
  uint32_t *parent, *root;
  // molecules
  uint32_t *kMol, *kLen;           // per key: molecules and list entries, then their exclusive sums
  uint32_t *fragMol, *molRow, *molFrags, *molStart, *molList;
  // table
  double *frac;
  int32_t *uniq;
  uint32_t nb;                     // bits of |S_m| in a triple
  uint32_t *counters;
};

// one more to the counter from every active lane that asks for it: one atomic per wavefront
__device__ __forceinline__ void umiCount(uint32_t *counter, bool mine) {
  const uint64_t m = __ballot(mine ? 1 : 0);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void k_umi_keys(UmiArgs P) {
  for (uint32_t f = blockIdx.x * 256u + threadIdx.x; f < P.nFrag; f += gridDim.x * 256u) {
    const unsigned long long u = P.umi[f];
    unsigned long long key = kNoUmi;
    if (u != kNoUmi) {
      const uint32_t len = (uint32_t)(u >> 32) & 31u;
      const unsigned long long bucket = (((unsigned long long)P.row[f] * P.nGenes + P.gene[P.list[P.listPtr[f]]]) << 4) | (len - 1);
      key = (bucket << 32) | (u & 0xFFFFFFFFull);
    }
    umiCount(P.counters + UMI_C_NOUMI, u == kNoUmi);
    P.keyA[f] = key;
    P.valA[f] = f;
  }
}

__device__ __forceinline__ uint32_t umiLowerBound(const unsigned long long *a, uint32_t lo, uint32_t hi, unsigned long long x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_umi_parent(UmiArgs P, uint32_t nU) {
  for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < nU; u += gridDim.x * 256u) {
    const unsigned long long key = P.runKey[u];
    uint32_t best = u;
    if (P.mismatch && key != kNoUmi) {
      const unsigned long long bucket = key >> 32;
      const uint32_t code = (uint32_t)key, len = ((uint32_t)bucket & 15u) + 1;
      const uint32_t cu = P.runStart[u + 1] - P.runStart[u];
      // the bucket's distinct UMIs: [lo, hi); u itself lies inside
      const uint32_t lo = umiLowerBound(P.runKey, 0, u, bucket << 32);
      const uint32_t end = umiLowerBound(P.runKey, u + 1, nU, (bucket + 1) << 32);  // (row * nGenes + gene < 2^28 - 1: no carry out of the key)
      uint32_t bestCnt = 0, bestCode = 0;
      for (uint32_t p = 0; p < len; ++p)
        for (uint32_t x = 1; x < 4; ++x) {
          const uint32_t v = code ^ (x << (2 * p));
          const unsigned long long want = (bucket << 32) | v;
          const uint32_t w = umiLowerBound(P.runKey, lo, end, want);
          if (w >= end || P.runKey[w] != want) continue;
          const uint32_t cv = P.runStart[w + 1] - P.runStart[w];
          if ((unsigned long long)cv + 1 < 2ull * cu) continue;                   // c(v) >= 2 c(u) - 1
          if (!(cv > cu || (cv == cu && v < code))) continue;
          if (best == u || cv > bestCnt || (cv == bestCnt && v < bestCode)) { best = w; bestCnt = cv; bestCode = v; }
        }
    }
    P.parent[u] = best;
    umiCount(P.counters + UMI_C_CORRECTED, best != u);
  }
}

__global__ __launch_bounds__(256) void k_umi_root(UmiArgs P, uint32_t nU) {
  for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < nU; u += gridDim.x * 256u) {
    uint32_t x = u;
    for (uint32_t p = P.parent[x]; p != x; p = P.parent[x]) x = p;  // (count, then smaller code) rises strictly along the chain: it ends
    P.root[u] = x;
  }
}

// sorted position i -> (root of its distinct UMI, its fragment)
__global__ __launch_bounds__(256) void k_umi_root_keys(UmiArgs P) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < P.nFrag; i += gridDim.x * 256u) {
    P.keyA[i] = P.root[P.scan[i] + P.flag[i] - 1];
    P.valA[i] = P.valB[i];
  }
}

__device__ __forceinline__ bool umiHas(const uint32_t *l, uint32_t n, uint32_t a) {
  for (uint32_t j = 0; j < n && l[j] <= a; ++j)
    if (l[j] == a) return true;
  return false;
}
__device__ __forceinline__ bool umiSameList(const uint32_t *a, uint32_t na, const uint32_t *b, uint32_t nb) {
  if (na != nb) return false;
  for (uint32_t j = 0; j < na; ++j)
    if (a[j] != b[j]) return false;
  return true;
}

// key k = the fragments valB[runStart[k] .. runStart[k + 1]).  WRITE = false: kMol[k], kLen[k] = its molecules and their list entries;
// WRITE = true (kMol / kLen hold the exclusive sums): the molecules themselves and fragMol
template <bool WRITE>
__global__ __launch_bounds__(256) void k_umi_mol(UmiArgs P, uint32_t nKeys) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nKeys; k += gridDim.x * 256u) {
    const uint32_t s = P.runStart[k], e = P.runStart[k + 1];
    const uint32_t f0 = P.valB[s];
    const uint32_t *l0 = P.list + P.listPtr[f0];
    const uint32_t n0 = P.listPtr[f0 + 1] - P.listPtr[f0];
    uint32_t m = 0, at = 0;
    if (WRITE) { m = P.kMol[k]; at = P.kLen[k]; }
    uint32_t nInter = 0;
    for (uint32_t j = 0; j < n0; ++j) {
      const uint32_t a = l0[j];
      bool all = true;
      for (uint32_t q = s + 1; q < e && all; ++q) {
        const uint32_t f = P.valB[q];
        all = umiHas(P.list + P.listPtr[f], P.listPtr[f + 1] - P.listPtr[f], a);
      }
      if (!all) continue;
      if (WRITE) P.molList[at + nInter] = a;
      ++nInter;
    }
    if (nInter) {
      if (WRITE) {
        P.molRow[m] = P.row[f0]; P.molFrags[m] = e - s; P.molStart[m] = at;
        for (uint32_t q = s; q < e; ++q) P.fragMol[P.valB[q]] = m;
      } else { P.kMol[k] = 1; P.kLen[k] = nInter; }
      continue;
    }
    // a collision of different alleles: one molecule per distinct list, in the order of the lists' first fragments
    uint32_t nM = 0, nL = 0;
    for (uint32_t q = s; q < e; ++q) {
      const uint32_t f = P.valB[q];
      const uint32_t *l = P.list + P.listPtr[f];
      const uint32_t n = P.listPtr[f + 1] - P.listPtr[f];
      bool seen = false;
      for (uint32_t r = s; r < q && !seen; ++r) {
        const uint32_t g = P.valB[r];
        seen = umiSameList(l, n, P.list + P.listPtr[g], P.listPtr[g + 1] - P.listPtr[g]);
      }
      if (seen) continue;
      if (WRITE) {
        uint32_t cnt = 0;
        for (uint32_t r = q; r < e; ++r) {
          const uint32_t g = P.valB[r];
          if (umiSameList(l, n, P.list + P.listPtr[g], P.listPtr[g + 1] - P.listPtr[g])) { ++cnt; P.fragMol[g] = m + nM; }
        }
        P.molRow[m + nM] = P.row[f]; P.molFrags[m + nM] = cnt; P.molStart[m + nM] = at + nL;
        for (uint32_t j = 0; j < n; ++j) P.molList[at + nL + j] = l[j];
      }
      ++nM; nL += n;
    }
    if (!WRITE) { P.kMol[k] = nM; P.kLen[k] = nL; }
    if (!WRITE) umiCount(P.counters + UMI_C_SPLIT, true);
  }
}

// molStart[nMol] = all list entries (the caller sets it before this launch)
__global__ __launch_bounds__(256) void k_umi_triples(UmiArgs P, uint32_t nMol) {
  for (uint32_t m = blockIdx.x * 256u + threadIdx.x; m < nMol; m += gridDim.x * 256u) {
    const uint32_t b = P.molStart[m], e = P.molStart[m + 1];
    const unsigned long long cell0 = (unsigned long long)P.molRow[m] * P.nAlleles;
    for (uint32_t j = b; j < e; ++j) P.keyA[j] = ((cell0 + P.molList[j]) << P.nb) | (unsigned long long)(e - b);
  }
}

// run r of the third table = K(row, allele, n) equal triples; the runs of a cell are consecutive, n ascending
__global__ __launch_bounds__(256) void k_umi_table(UmiArgs P, uint32_t nRuns) {
  const unsigned long long nMask = (1ull << P.nb) - 1;
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nRuns; r += gridDim.x * 256u) {
    const unsigned long long cell = P.runKey[r] >> P.nb;
    if (r && (P.runKey[r - 1] >> P.nb) == cell) continue;
    double sum = 0;
    int32_t uq = 0;
    for (uint32_t q = r; q < nRuns && (P.runKey[q] >> P.nb) == cell; ++q) {
      const uint32_t K = P.runStart[q + 1] - P.runStart[q];
      const uint32_t n = (uint32_t)(P.runKey[q] & nMask);
      sum += (double)K / (double)n;
      if (n == 1) uq = (int32_t)K;
    }
    P.frac[cell] = sum;
    P.uniq[cell] = uq;
  }
}

extern "C" {

int t1k_umi_collapse(t1k_ctx *ctx, uint32_t nFrag, const uint32_t *fragRow, const uint64_t *fragUmi, const uint64_t *listPtr, const uint32_t *listAllele, uint32_t nRows,
                     const uint32_t *alleleGene, uint32_t nAlleles, uint32_t nGenes, int32_t mismatch, uint32_t *fragMol, uint32_t *nMolOut, uint32_t *molRow, uint32_t *molFrags,
                     uint64_t *molListPtr, uint32_t *molList, double *frac, int32_t *uniq, t1k_umi_stats *stats) {
  if (!ctx) return T1K_ERR_ARG;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (nMolOut) *nMolOut = 0;
  if (mismatch != 0 && mismatch != 1) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: mismatch must be 0 or 1");
  if (!nMolOut || !molListPtr) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: bad arguments (NULL outputs)");
  if (nFrag >= (1u << 31)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_umi_collapse: more than 2^31 fragments in one call");
  // the key layout: 28 bits of row * nGenes + gene beside 4 of length and 32 of code; a table cell beside the list length in 64 bits
  if ((unsigned long long)nRows * nGenes >= (1ull << 28)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_umi_collapse: nRows * nGenes does not fit the key (2^28)");
  const unsigned long long nCells = (unsigned long long)nRows * nAlleles;
  if (nCells >= (1ull << 40)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_umi_collapse: nRows * nAlleles does not fit the table (2^40)");
  if (nCells && (!frac || !uniq)) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: bad arguments (NULL table)");
  if (nAlleles && !alleleGene) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: bad arguments (NULL alleleGene)");
  for (uint32_t a = 0; a < nAlleles; ++a)
    if (alleleGene[a] >= nGenes) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: an allele's gene is out of range");
  if (frac) std::fill(frac, frac + nCells, 0.0);
  if (uniq) std::fill(uniq, uniq + nCells, 0);
  molListPtr[0] = 0;
  if (nFrag == 0) return T1K_OK;
  if (!fragRow || !fragUmi || !listPtr || !listAllele || !fragMol || !molRow || !molFrags || !molList) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: bad arguments (NULL arrays)");
  // the slice: lists rebased to its first entry; every fragment has a list, strictly ascending and known
  const uint64_t eB = listPtr[0];
  uint32_t maxList = 1;
  for (uint32_t f = 0; f < nFrag; ++f) {
    if (listPtr[f + 1] <= listPtr[f]) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: a fragment has no list (or the list offsets decrease)");
    if (listPtr[f + 1] - eB >= (1ull << 32)) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_umi_collapse: more than 2^32 list entries in one call");
    if (fragRow[f] >= nRows) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: a fragment's row is out of range");
    const uint64_t u = fragUmi[f];
    if (u != kNoUmi) {
      const uint32_t len = (uint32_t)(u >> 32);
      if (len < 1 || len > 16 || (len < 16 && (u & 0xFFFFFFFFull) >> (2 * len))) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: a UMI word is neither 1 - 16 bases nor all ones");
    }
    for (uint64_t j = listPtr[f]; j < listPtr[f + 1]; ++j)
      if (listAllele[j] >= nAlleles || (j > listPtr[f] && listAllele[j] <= listAllele[j - 1])) return t1k_fail(ctx, T1K_ERR_ARG, "t1k_umi_collapse: a list is not ascending, or names an unknown allele");
    maxList = std::max(maxList, (uint32_t)(listPtr[f + 1] - listPtr[f]));
  }
  const uint64_t nE = listPtr[nFrag] - eB;
  const int nb = t1k_bits(maxList), cellBits = t1k_bits(nCells ? nCells - 1 : 0);
  if (nb + cellBits > 64) return t1k_fail(ctx, T1K_ERR_CAPACITY, "t1k_umi_collapse: a table cell and a list length do not fit 64 bits");
  std::vector<uint32_t> lp(nFrag + 1);
  for (uint32_t f = 0; f <= nFrag; ++f) lp[f] = (uint32_t)(listPtr[f] - eB);
  // device: one block, 256-byte aligned pieces, sized by the upper bounds (molecules <= fragments, their entries <= the fragments')
  const uint64_t M = std::max<uint64_t>(nFrag, nE);
  T1kCarve piece;
  const size_t oRow = piece(4ull * nFrag), oUmi = piece(8ull * nFrag), oLp = piece(4ull * (nFrag + 1)), oList = piece(4 * nE), oGene = piece(4ull * nAlleles),
               oKeyA = piece(8 * M), oKeyB = piece(8 * M), oValA = piece(4 * M), oValB = piece(4 * M), oFlag = piece(4 * (M + 1)), oScan = piece(4 * (M + 1)),
               oRunStart = piece(4 * (M + 1)), oRunKey = piece(8 * M), oParent = piece(4ull * nFrag), oRoot = piece(4ull * nFrag), oKMol = piece(4ull * (nFrag + 1)),
               oKLen = piece(4ull * (nFrag + 1)), oFragMol = piece(4ull * nFrag), oMolRow = piece(4ull * nFrag), oMolFrags = piece(4ull * nFrag),
               oMolStart = piece(4ull * (nFrag + 1)), oMolList = piece(4 * nE), oFrac = piece(8 * nCells), oUniq = piece(4 * nCells), oCnt = piece(4 * UMI_C_WORDS);
  T1K_HIP(ctx, hipSetDevice(ctx->device));
  T1kCallBlock blk;
  int rc;
  if ((rc = blk.alloc(ctx, piece.off))) return rc;
  hipStream_t st = ctx->stream;
  char *D = (char *)blk.buf.p;
  T1K_HIP(ctx, hipMemcpyAsync(D + oRow, fragRow, 4ull * nFrag, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oUmi, fragUmi, 8ull * nFrag, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oLp, lp.data(), 4ull * (nFrag + 1), hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oList, listAllele + eB, 4 * nE, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemcpyAsync(D + oGene, alleleGene, 4ull * nAlleles, hipMemcpyHostToDevice, st));
  T1K_HIP(ctx, hipMemsetAsync(D + oCnt, 0, 4 * UMI_C_WORDS, st));
  if (nCells) {
    T1K_HIP(ctx, hipMemsetAsync(D + oFrac, 0, 8 * nCells, st));
    T1K_HIP(ctx, hipMemsetAsync(D + oUniq, 0, 4 * nCells, st));
  }
  UmiArgs a{};
  a.row = (const uint32_t *)(D + oRow); a.listPtr = (const uint32_t *)(D + oLp); a.list = (const uint32_t *)(D + oList); a.gene = (const uint32_t *)(D + oGene);
  a.umi = (const unsigned long long *)(D + oUmi);
  a.nFrag = nFrag; a.nGenes = nGenes; a.nAlleles = nAlleles; a.mismatch = (uint32_t)mismatch;
  a.keyA = (unsigned long long *)(D + oKeyA); a.keyB = (unsigned long long *)(D + oKeyB); a.valA = (uint32_t *)(D + oValA); a.valB = (uint32_t *)(D + oValB);
  a.flag = (uint32_t *)(D + oFlag); a.scan = (uint32_t *)(D + oScan); a.runStart = (uint32_t *)(D + oRunStart); a.runKey = (unsigned long long *)(D + oRunKey);
  a.parent = (uint32_t *)(D + oParent); a.root = (uint32_t *)(D + oRoot); a.kMol = (uint32_t *)(D + oKMol); a.kLen = (uint32_t *)(D + oKLen);
  a.fragMol = (uint32_t *)(D + oFragMol); a.molRow = (uint32_t *)(D + oMolRow); a.molFrags = (uint32_t *)(D + oMolFrags); a.molStart = (uint32_t *)(D + oMolStart);
  a.molList = (uint32_t *)(D + oMolList); a.frac = (double *)(D + oFrac); a.uniq = (int32_t *)(D + oUniq); a.nb = (uint32_t)nb; a.counters = (uint32_t *)(D + oCnt);
  T1K_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  // distinct UMIs
  hipLaunchKernelGGL(k_umi_keys, dim3(t1k_grid(ctx, nFrag, 256)), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_sort_pairs(ctx, a.keyA, a.keyB, a.valA, a.valB, nFrag, 64))) return rc;
  uint32_t nU = 0, nKeys = 0, nRuns = 0;
  if ((rc = t1k_run_table(ctx, a.keyB, nFrag, &kNoUmi, a.flag, a.scan, a.runStart, a.runKey, &nU))) return rc;
  if (nU == 0 || nU > nFrag) return t1k_fail(ctx, T1K_ERR_INTERNAL, "t1k_umi_collapse: the distinct UMIs do not add up");
  hipLaunchKernelGGL(k_umi_parent, dim3(t1k_grid(ctx, nU, 256)), dim3(256), 0, st, a, nU);
  T1K_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_umi_root, dim3(t1k_grid(ctx, nU, 256)), dim3(256), 0, st, a, nU);
  T1K_HIP(ctx, hipGetLastError());
  // keys: the fragments by the root of their UMI
  hipLaunchKernelGGL(k_umi_root_keys, dim3(t1k_grid(ctx, nFrag, 256)), dim3(256), 0, st, a);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_sort_pairs(ctx, a.keyA, a.keyB, a.valA, a.valB, nFrag, t1k_bits(nU - 1)))) return rc;
  if ((rc = t1k_run_table(ctx, a.keyB, nFrag, nullptr, a.flag, a.scan, a.runStart, a.runKey, &nKeys))) return rc;
  if (nKeys == 0 || nKeys > nU) return t1k_fail(ctx, T1K_ERR_INTERNAL, "t1k_umi_collapse: the keys do not add up");
  // molecules: size, place, write
  hipLaunchKernelGGL(k_umi_mol<false>, dim3(t1k_grid(ctx, nKeys, 256)), dim3(256), 0, st, a, nKeys);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipMemsetAsync(a.kMol + nKeys, 0, 4, st));
  T1K_HIP(ctx, hipMemsetAsync(a.kLen + nKeys, 0, 4, st));
  if ((rc = t1k_exclusive_sum32(ctx, a.kMol, a.kMol, (uint64_t)nKeys + 1))) return rc;
  if ((rc = t1k_exclusive_sum32(ctx, a.kLen, a.kLen, (uint64_t)nKeys + 1))) return rc;
  uint32_t nMol = 0, nLen = 0;
  T1K_HIP(ctx, hipMemcpyAsync(&nMol, a.kMol + nKeys, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(&nLen, a.kLen + nKeys, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  if (nMol < nKeys || nMol > nFrag || nLen < nMol || nLen > nE) return t1k_fail(ctx, T1K_ERR_INTERNAL, "t1k_umi_collapse: the molecules exceed their upper bounds");
  hipLaunchKernelGGL(k_umi_mol<true>, dim3(t1k_grid(ctx, nKeys, 256)), dim3(256), 0, st, a, nKeys);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipMemcpyAsync(a.molStart + nMol, &nLen, 4, hipMemcpyHostToDevice, st));
  // the table
  hipLaunchKernelGGL(k_umi_triples, dim3(t1k_grid(ctx, nMol, 256)), dim3(256), 0, st, a, nMol);
  T1K_HIP(ctx, hipGetLastError());
  if ((rc = t1k_sort_pairs(ctx, a.keyA, a.keyB, a.valA, a.valB, nLen, nb + cellBits))) return rc;  // (the values ride along unread)
  if ((rc = t1k_run_table(ctx, a.keyB, nLen, nullptr, a.flag, a.scan, a.runStart, a.runKey, &nRuns))) return rc;
  if (nRuns == 0 || nRuns > nLen) return t1k_fail(ctx, T1K_ERR_INTERNAL, "t1k_umi_collapse: the table's runs do not add up");
  hipLaunchKernelGGL(k_umi_table, dim3(t1k_grid(ctx, nRuns, 256)), dim3(256), 0, st, a, nRuns);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  // results
  std::vector<uint32_t> ms(nMol + 1);
  uint32_t cnt[UMI_C_WORDS] = {};
  T1K_HIP(ctx, hipMemcpyAsync(fragMol, a.fragMol, 4ull * nFrag, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(molRow, a.molRow, 4ull * nMol, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(molFrags, a.molFrags, 4ull * nMol, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(ms.data(), a.molStart, 4ull * (nMol + 1), hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipMemcpyAsync(molList, a.molList, 4ull * nLen, hipMemcpyDeviceToHost, st));
  if (nCells) {
    T1K_HIP(ctx, hipMemcpyAsync(frac, a.frac, 8 * nCells, hipMemcpyDeviceToHost, st));
    T1K_HIP(ctx, hipMemcpyAsync(uniq, a.uniq, 4 * nCells, hipMemcpyDeviceToHost, st));
  }
  T1K_HIP(ctx, hipMemcpyAsync(cnt, a.counters, 4 * UMI_C_WORDS, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  for (uint32_t m = 0; m <= nMol; ++m) molListPtr[m] = ms[m];
  *nMolOut = nMol;
  if (stats) {
    stats->keys = nKeys - cnt[UMI_C_NOUMI];
    stats->corrected = cnt[UMI_C_CORRECTED];
    stats->split = cnt[UMI_C_SPLIT];
    stats->no_umi = cnt[UMI_C_NOUMI];
    stats->distinct = nU - cnt[UMI_C_NOUMI];
    float ms_ = 0;
    if (hipEventElapsedTime(&ms_, ctx->ev[0], ctx->ev[1]) == hipSuccess) stats->kernel_ms = ms_;
  }
  return T1K_OK;
}

}  // extern "C"
