// l2hmc_order_stats -- exact order statistics of every coordinate of a recorded history X (S, d) that stays where the sampler
// wrote it: values[r, k] = the element a full ascending sort of coordinate k would put at position ranks[r, k].
// l2hmc_amd/quantiles.py turns them into quantiles, tail-ESS and quantile MCSE; include/l2hmc.h states the contract.
//
// Most-significant-digit radix select on the monotone key of a float32 (bits ^ 0xFFFFFFFF for a negative value, bits | 0x80000000
// otherwise; every NaN takes the key 0xFFFFFFFF and sorts last, like numpy), kRadixPasses = 4 passes of kRadixBits = 8 bits; the
// key and the advance step are radix_select.hpp's, shared with loo.hip.  A pass:
//
//   count    order_count_kernel: for every (r, k) the histogram of the next digit of the keys whose higher digits equal the
//            pair's prefix.  In pass 0 the prefix is empty and the R histograms of a coordinate are equal: one is counted and
//            flushed R times.  A block is 256 threads over rpc = 256 / sg consecutive rows of one GROUP of sg <= 64 coordinates
//            (thread <-> (row tid / sg, coordinate tid % sg); with sg = d the block reads 256 - 256 % d contiguous floats), and
//            walks the rows b rpc, (b + nb) rpc, ...: a thread's coordinate never changes, so the prefixes of its RG ranks are RG
//            registers with compile-time indices.  The LDS histogram is [256 bins][NS columns] uint32, bin-major, with
//            NS = copies x sg x RG <= 64 columns: column = (copy, coordinate, rank) and copy = (tid / sg) % copies, so lane l of
//            a wave owns column l % (copies sg) -- with copies sg = 64 no two lanes of a wave ever add to one address, and lanes
//            that hit the SAME bin (the first digit of a float key is sign and high exponent: nearly every draw of a coordinate
//            lands in one to three bins) sit in neighbouring banks.  That is the answer to same-bin contention here; the
//            alternative -- count runs of equal bins in a register, one atomic per run -- is kept as a variant of pass 0
//            (L2HMC_ORDER_STATS_RUNS=1) so that both can be measured.
//            After the loop the copies are added and the NON-ZERO bins go to the global int64 histogram with vector atomicAdd.
//            Integer addition does not depend on arrival order: the histogram is bitwise reproducible and the same however
//            the draws are sharded.  When a group cannot hold every coordinate and rank (sg RG <= 64), blockIdx.y / z walk the
//            coordinate / rank groups and the history is read once per group.
//   advance  radix_advance_kernel (radix_select.hpp), one wave per (r, k); after the last pass it writes the value the prefix
//            encodes.  A rank at or past the number of draws takes the maximum.
// Nothing returns to the host between passes, and the library allocates nothing.
#include <stdlib.h>

#include "radix_select.hpp"

namespace l2hmc {

constexpr int kOsThreads = 256;
constexpr int kOsCols = 64;        // columns of the LDS histogram: 256 bins x 64 x 4 B = 64 KiB, two blocks per CU
constexpr int kOsMaxRanks = 32;
constexpr int kOsBlocks = 1024;    // blocks the planner aims for over all groups
constexpr int kOsUnroll = 8;       // independent loads in flight per thread

struct OrderStatsPlan {
  int sg, rg, ngk, ngr;            // coordinates / ranks per group (rg is the kernel's template argument), groups of each
  int copies, rpc, ns;             // histogram copies, rows per block step, LDS columns = copies sg rg
  long long nb;                    // blocks along x
};

// the host's plan of a count pass; false (with the message set) when the arguments are not a valid request
static bool order_stats_plan(const char* who, int64_t n_draws, int32_t d, int32_t n_ranks, int32_t pass, OrderStatsPlan& p) {
  if (n_draws < 1 || d < 1) { fail(L2HMC_ERR_ARG, "%s: n_draws and d must be >= 1", who); return false; }
  if (d > 512) { fail(L2HMC_ERR_ARG, "%s: d <= 512 (got %lld)", who, d); return false; }
  if (n_ranks < 1 || n_ranks > kOsMaxRanks) { fail(L2HMC_ERR_ARG, "%s: 1 <= n_ranks <= 32 (got %lld)", who, n_ranks); return false; }
  if (pass < 0 || pass >= kRadixPasses) { fail(L2HMC_ERR_ARG, "%s: 0 <= pass <= 3 (got %lld)", who, pass); return false; }
  if (n_draws > (1LL << 40) / d) { fail(L2HMC_ERR_ARG, "%s: history too large (n_draws d > 2^40)", who); return false; }
  // fewest groups = fewest reads of the history; among equals the widest coordinate group (the longest contiguous runs)
  int best_rg = 1;
  long long best = -1;
  for (int rg = 1; rg <= kOsMaxRanks; rg *= 2) {
    if (pass == 0 && rg > 1) break;                   // one histogram per coordinate
    const int sgmax = kOsCols / rg < d ? kOsCols / rg : d;
    const long long ngk = (d + sgmax - 1) / sgmax, ngr = pass == 0 ? 1 : (n_ranks + rg - 1) / rg;
    if (best < 0 || ngk * ngr < best) { best = ngk * ngr; best_rg = rg; }
    if (rg >= n_ranks) break;
  }
  p.rg = best_rg;
  const int sgmax = kOsCols / p.rg < d ? kOsCols / p.rg : d;
  p.ngk = (d + sgmax - 1) / sgmax;
  p.sg = (d + p.ngk - 1) / p.ngk;                     // groups of equal width
  p.ngr = pass == 0 ? 1 : (n_ranks + p.rg - 1) / p.rg;
  p.rpc = kOsThreads / p.sg;
  p.copies = kOsCols / (p.sg * p.rg);
  if (p.copies > p.rpc) p.copies = p.rpc;
  p.ns = p.copies * p.sg * p.rg;
  const long long chunks = (n_draws + p.rpc - 1) / p.rpc;
  p.nb = kOsBlocks / ((long long)p.ngk * p.ngr);
  if (p.nb < 64) p.nb = 64;
  if (p.nb > chunks) p.nb = chunks;
  // a column of a block's LDS histogram is a uint32 and counts at most the rows the block walks
  if (chunks / p.nb >= (1LL << 32) / p.rpc) { fail(L2HMC_ERR_ARG, "%s: history too large", who); return false; }
  return true;
}

// RG: rank slots per thread (compile-time register indices); kPass0: empty prefix, one histogram per coordinate, NaNs counted;
// kRuns (pass 0 only): runs of equal bins are counted in a register and cost one atomic per run
template <int RG, bool kPass0, bool kRuns>
__global__ __launch_bounds__(kOsThreads) void order_count_kernel(const float* __restrict__ X, long long S, int d, int n_ranks,
                                                                 int shift, const uint32_t* __restrict__ prefix,
                                                                 unsigned long long* __restrict__ hist,
                                                                 unsigned long long* __restrict__ n_nan, int sg, int copies) {
  extern __shared__ uint32_t os_h[];                  // [kRadixBins][ns]
  const int tid = threadIdx.x;
  const int rpc = kOsThreads / sg, ns = copies * sg * RG;
  const int kk = tid % sg, rowin = tid / sg;
  const int k = blockIdx.y * sg + kk;
  const int r0 = kPass0 ? 0 : blockIdx.z * RG;
  const int nr = kPass0 ? 1 : (n_ranks - r0 < RG ? n_ranks - r0 : RG);
  const bool active = rowin < rpc && k < d;
  const int col0 = ((rowin % copies) * sg + kk) * RG;

  for (int i = tid; i < kRadixBins * ns; i += kOsThreads) os_h[i] = 0u;
  uint32_t pre[RG];
#pragma unroll
  for (int r = 0; r < RG; ++r) pre[r] = (!kPass0 && active && r < nr) ? prefix[(long long)(r0 + r) * d + k] >> (shift + kRadixBits) : 0u;
  __syncthreads();

  unsigned nan_count = 0u;
  int run_bin = 0;
  unsigned run_len = 0u;
  auto count = [&](float v) {
    const uint32_t key = radix_key(v);
    if (v != v) ++nan_count;
    if (kPass0) {
      const int bin = (int)(key >> 24);
      if (kRuns) {
        if (bin != run_bin && run_len) { atomicAdd(&os_h[run_bin * ns + col0], run_len); run_len = 0u; }
        run_bin = bin;
        ++run_len;
      } else {
        atomicAdd(&os_h[bin * ns + col0], 1u);
      }
    } else {
      const uint32_t hi = key >> (shift + kRadixBits);
      const int at = (int)((key >> shift) & (kRadixBins - 1)) * ns + col0;
#pragma unroll
      for (int r = 0; r < RG; ++r)
        if (r < nr && hi == pre[r]) atomicAdd(&os_h[at + r], 1u);
    }
  };

  if (active) {
    const long long step = (long long)gridDim.x * rpc;
    long long i = (long long)blockIdx.x * rpc + rowin;
    const float* p = X + i * d + k;
    const long long pstep = step * d;
    // software-pipelined: the next batch of loads is issued before the current one is counted, so loads stay in flight
    // through the compare-and-add work (two to three waves per SIMD cannot hide it otherwise)
    float v[kOsUnroll], w[kOsUnroll];
    bool have = i + (kOsUnroll - 1) * step < S;
    if (have) {
#pragma unroll
      for (int u = 0; u < kOsUnroll; ++u) v[u] = p[u * pstep];
    }
    while (have) {
      i += kOsUnroll * step;
      p += kOsUnroll * pstep;
      have = i + (kOsUnroll - 1) * step < S;
      if (have) {
#pragma unroll
        for (int u = 0; u < kOsUnroll; ++u) w[u] = p[u * pstep];
      }
#pragma unroll
      for (int u = 0; u < kOsUnroll; ++u) count(v[u]);
#pragma unroll
      for (int u = 0; u < kOsUnroll; ++u) v[u] = w[u];
    }
    for (; i < S; i += step, p += pstep) count(*p);
    if (kRuns && run_len) atomicAdd(&os_h[run_bin * ns + col0], run_len);
    if (kPass0 && nan_count && n_nan) atomicAdd(&n_nan[k], (unsigned long long)nan_count);
  }
  __syncthreads();

  // the copies added, non-zero bins only to the global histogram (n_ranks, d, kRadixBins)
  const int per_bin = sg * RG;
  for (int i = tid; i < kRadixBins * per_bin; i += kOsThreads) {
    const int bin = i / per_bin, rem = i - bin * per_bin;
    const int fk = rem / RG, r = rem - fk * RG;
    const int gk = blockIdx.y * sg + fk;
    if (gk >= d || r >= nr) continue;
    unsigned long long c = 0ull;
    for (int cp = 0; cp < copies; ++cp) c += os_h[bin * ns + (cp * sg + fk) * RG + r];
    if (!c) continue;
    if (kPass0) {
      for (int q = 0; q < n_ranks; ++q) atomicAdd(&hist[((long long)q * d + gk) * kRadixBins + bin], c);
    } else {
      atomicAdd(&hist[((long long)(r0 + r) * d + gk) * kRadixBins + bin], c);
    }
  }
}

template <int RG>
static void order_count_launch(const OrderStatsPlan& p, bool runs, hipStream_t s, const float* X, int64_t S, int32_t d,
                               int32_t n_ranks, int32_t pass, const uint32_t* prefix, int64_t* hist, int64_t* n_nan) {
  const dim3 grid((unsigned)p.nb, (unsigned)p.ngk, (unsigned)p.ngr), block(kOsThreads);
  const size_t lds = (size_t)kRadixBins * p.ns * sizeof(uint32_t);
  const int shift = 32 - kRadixBits * (pass + 1);
  unsigned long long* h = (unsigned long long*)hist;
  unsigned long long* nn = (unsigned long long*)n_nan;
  if (pass == 0) {
    if constexpr (RG == 1) {
      if (runs) hipLaunchKernelGGL((order_count_kernel<1, true, true>), grid, block, lds, s, X, (long long)S, (int)d, (int)n_ranks, shift, prefix, h, nn, p.sg, p.copies);
      else hipLaunchKernelGGL((order_count_kernel<1, true, false>), grid, block, lds, s, X, (long long)S, (int)d, (int)n_ranks, shift, prefix, h, nn, p.sg, p.copies);
    }
  } else {
    hipLaunchKernelGGL((order_count_kernel<RG, false, false>), grid, block, lds, s, X, (long long)S, (int)d, (int)n_ranks, shift, prefix, h, nn, p.sg, p.copies);
  }
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int32_t l2hmc_order_stats_passes(void) { return kRadixPasses; }
int32_t l2hmc_order_stats_bins(void) { return kRadixBins; }

int64_t l2hmc_order_stats_workspace_bytes(int32_t d, int32_t n_ranks) {
  OrderStatsPlan p;
  if (!order_stats_plan("l2hmc_order_stats_workspace_bytes", 1, d, n_ranks, 0, p)) return L2HMC_ERR_ARG;
  // histogram (n_ranks, d, bins) int64 | remaining (n_ranks, d) int64 | prefix (n_ranks, d) uint32, rounded to 16 bytes
  const int64_t n = (int64_t)n_ranks * d;
  return (n * (kRadixBins * 8 + 8 + 4) + 15) / 16 * 16;
}

int l2hmc_order_stats_count(const float* X, int64_t n_draws, int32_t d, int32_t n_ranks, int32_t pass, const uint32_t* prefix,
                            int64_t* hist, int64_t* n_nan, void* stream) {
  OrderStatsPlan p;
  if (!order_stats_plan("l2hmc_order_stats_count", n_draws, d, n_ranks, pass, p)) return L2HMC_ERR_ARG;
  if (!X || !hist || (pass > 0 && !prefix) || (pass == 0 && !n_nan))
    return fail(L2HMC_ERR_ARG, "l2hmc_order_stats_count: X, hist, prefix (pass > 0) and n_nan (pass 0) are required%s");
  static const bool runs = [] { const char* e = getenv("L2HMC_ORDER_STATS_RUNS"); return e && e[0] && e[0] != '0'; }();
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_ranks * d * kRadixBins * sizeof(int64_t), s);
  if (e == hipSuccess && pass == 0) e = hipMemsetAsync(n_nan, 0, (size_t)d * sizeof(int64_t), s);
  if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
  switch (p.rg) {
    case 1: order_count_launch<1>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
    case 2: order_count_launch<2>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
    case 4: order_count_launch<4>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
    case 8: order_count_launch<8>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
    case 16: order_count_launch<16>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
    default: order_count_launch<32>(p, runs, s, X, n_draws, d, n_ranks, pass, prefix, hist, n_nan); break;
  }
  return launched();
}

int l2hmc_order_stats_advance(const int64_t* hist, int64_t* remaining, uint32_t* prefix, int32_t d, int32_t n_ranks,
                              int32_t pass, float* values, void* stream) {
  OrderStatsPlan p;
  if (!order_stats_plan("l2hmc_order_stats_advance", 1, d, n_ranks, pass, p)) return L2HMC_ERR_ARG;
  if (!hist || !remaining || !prefix || (pass == kRadixPasses - 1 && !values))
    return fail(L2HMC_ERR_ARG, "l2hmc_order_stats_advance: hist, remaining, prefix and values (last pass) are required%s");
  const int n = n_ranks * d;
  hipLaunchKernelGGL(radix_advance_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream,
                     (const long long*)hist, (long long*)remaining, prefix, n, 32 - kRadixBits * (pass + 1),
                     pass == kRadixPasses - 1 ? values : (float*)nullptr);
  return launched();
}

int l2hmc_order_stats(const float* X, int64_t n_draws, int32_t d, const int64_t* ranks, int32_t n_ranks, float* values,
                      int64_t* n_nan, void* workspace, void* stream) {
  OrderStatsPlan p;
  if (!order_stats_plan("l2hmc_order_stats", n_draws, d, n_ranks, 0, p)) return L2HMC_ERR_ARG;
  if (!X || !ranks || !values || !n_nan || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_order_stats: X, ranks, values, n_nan and workspace are required%s");
  const int64_t n = (int64_t)n_ranks * d;
  int64_t* hist = (int64_t*)workspace;
  int64_t* remaining = hist + n * kRadixBins;
  uint32_t* prefix = (uint32_t*)(remaining + n);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(remaining, ranks, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(prefix, 0, (size_t)n * sizeof(uint32_t), s);
  if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "l2hmc_order_stats: %s", hipGetErrorString(e));
  for (int pass = 0; pass < kRadixPasses; ++pass) {
    int rc = l2hmc_order_stats_count(X, n_draws, d, n_ranks, pass, prefix, hist, pass == 0 ? n_nan : nullptr, stream);
    if (rc != L2HMC_OK) return rc;
    rc = l2hmc_order_stats_advance(hist, remaining, prefix, d, n_ranks, pass, pass == kRadixPasses - 1 ? values : nullptr, stream);
    if (rc != L2HMC_OK) return rc;
  }
  return L2HMC_OK;
}

}  // extern "C"
