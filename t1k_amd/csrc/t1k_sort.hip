// t1k_amd/csrc/t1k_sort.hip -- device-wide ordering primitives: stable radix sort of (64-bit key, 32-bit value) pairs and
// prefix sums over 32-/64-bit counters, and the run table over sorted keys that the analyzer's stages build from them.  They ORDER
// and NUMBER work items (alignment queues, read-end hashes, fragment pattern hashes, group offsets); they are not part of the
// genotyper's arithmetic.  rocPRIM (the ROCm-native device primitives) directly.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include "t1k_dev.h"
#include "t1k_launch.h"

int t1k_sort_pairs(t1k_ctx *ctx, const unsigned long long *keysIn, unsigned long long *keysOut, const uint32_t *valsIn, uint32_t *valsOut, uint32_t n, int endBit) {
  if (!n) return T1K_OK;
  (void)hipGetLastError();  // rocPRIM reports the thread's last HIP error after its launches: a stale one (left by another library, e.g. RCCL's device probing) is not ours
  size_t bytes = 0;
  T1K_HIP(ctx, rocprim::radix_sort_pairs(nullptr, bytes, keysIn, keysOut, valsIn, valsOut, (size_t)n, 0u, (unsigned)endBit, ctx->stream));
  int rc = t1k_ensure(ctx, ctx->bSortTmp, bytes + 256);
  if (rc) return rc;
  T1K_HIP(ctx, rocprim::radix_sort_pairs(ctx->bSortTmp.p, bytes, keysIn, keysOut, valsIn, valsOut, (size_t)n, 0u, (unsigned)endBit, ctx->stream));
  return T1K_OK;
}

// every prefix sum below: out[i] = in[0] + .. + in[i] (INCLUSIVE) or in[0] + .. + in[i - 1], summed in Out
template <bool INCLUSIVE, class In, class Out>
static int scanSum(t1k_ctx *ctx, const In *in, Out *out, uint64_t n) {
  if (!n) return T1K_OK;
  (void)hipGetLastError();  // rocPRIM reports the thread's last HIP error after its launches: a stale one (left by another library, e.g. RCCL's device probing) is not ours
  size_t bytes = 0;
  auto scan = [&](void *tmp) {
    if constexpr (INCLUSIVE) return rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<Out>(), ctx->stream);
    else return rocprim::exclusive_scan(tmp, bytes, in, out, Out(0), (size_t)n, rocprim::plus<Out>(), ctx->stream);
  };
  T1K_HIP(ctx, scan(nullptr));  // the size query
  int rc = t1k_ensure(ctx, ctx->bSortTmp, bytes + 256);
  if (rc) return rc;
  T1K_HIP(ctx, scan(ctx->bSortTmp.p));
  return T1K_OK;
}

int t1k_inclusive_sum(t1k_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n) { return scanSum<true>(ctx, in, out, n); }
// the exclusive sums: in == out is allowed (every tile is read before it is written)
int t1k_exclusive_sum32(t1k_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n) { return scanSum<false>(ctx, in, out, n); }
int t1k_exclusive_sum64(t1k_ctx *ctx, const uint32_t *in, unsigned long long *out, uint32_t n) { return scanSum<false>(ctx, in, out, n); }
int t1k_exclusive_sum_u64(t1k_ctx *ctx, const unsigned long long *in, unsigned long long *out, uint64_t n) { return scanSum<false>(ctx, in, out, n); }

// flag[i] = position i starts a run of equal keys (alone: a key equal to `lone` never joins a run); flag[n] = 0 for the scan's total
__global__ __launch_bounds__(256) void k_run_heads(const unsigned long long *keys, uint32_t n, int hasLone, unsigned long long lone, uint32_t *flag) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= n; i += gridDim.x * 256u) {
    uint32_t h = 0;
    if (i < n) {
      const unsigned long long k = keys[i];
      h = (i == 0 || keys[i - 1] != k || (hasLone && k == lone)) ? 1u : 0u;
    }
    flag[i] = h;
  }
}

// scan[i] = runs before position i (scan[n] = all of them): run r starts at runStart[r], runStart[runs] = n
__global__ __launch_bounds__(256) void k_run_starts(const unsigned long long *keys, uint32_t n, const uint32_t *flag, const uint32_t *scan, uint32_t *runStart, unsigned long long *runKey) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= n; i += gridDim.x * 256u) {
    if (i == n) runStart[scan[n]] = n;
    else if (flag[i]) { runStart[scan[i]] = i; runKey[scan[i]] = keys[i]; }
  }
}

int t1k_run_table(t1k_ctx *ctx, const unsigned long long *keys, uint32_t n, const unsigned long long *lone, uint32_t *flag, uint32_t *scan, uint32_t *runStart,
                  unsigned long long *runKey, uint32_t *runs) {
  hipStream_t st = ctx->stream;
  const unsigned grid = t1k_grid(ctx, (uint64_t)n + 1, 256);
  hipLaunchKernelGGL(k_run_heads, dim3(grid), dim3(256), 0, st, keys, n, lone ? 1 : 0, lone ? *lone : 0ull, flag);
  T1K_HIP(ctx, hipGetLastError());
  int rc = t1k_exclusive_sum32(ctx, flag, scan, (uint64_t)n + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_run_starts, dim3(grid), dim3(256), 0, st, keys, n, (const uint32_t *)flag, (const uint32_t *)scan, runStart, runKey);
  T1K_HIP(ctx, hipGetLastError());
  T1K_HIP(ctx, hipMemcpyAsync(runs, scan + n, 4, hipMemcpyDeviceToHost, st));
  T1K_HIP(ctx, hipStreamSynchronize(st));
  return T1K_OK;
}
