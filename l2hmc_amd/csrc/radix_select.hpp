// The most-significant-digit radix select on float32 values, stated once: kRadixPasses = 4 passes of kRadixBits = 8 bits.
//   key      radix_key / radix_unkey: the monotone key (order_stats.hip, loo.hip, glm.hip, loglik_tails.hip);
//   count    the count pass of a workgroup that keeps one LDS histogram [rows][kRadixBins] uint32 of the next digit of the keys
//            on their row's prefix (loo_kernel<*, 0>, glm_loo_kernel<*, *, 0>): radix_hist_clear, radix_count_first,
//            radix_count_next, radix_hist_flush.  Integer LDS atomics, flushed -- non-zero bins only -- to the global int64
//            histogram (n, kRadixBins) with integer atomics: counts do not depend on arrival order.  order_stats.hip counts per
//            rank and column in registers and keeps its own kernel;
//   advance  radix_advance_kernel: the step between two count passes;
//   driver   radix_select_passes: memset, count, advance, four times, with the caller's count launch.
#pragma once
#include "l2hmc_kernels.hpp"

namespace l2hmc {

constexpr int kRadixBits = 8;
constexpr int kRadixBins = 1 << kRadixBits;
constexpr int kRadixPasses = 32 / kRadixBits;

// the monotone key of a float32: unsigned order of the keys = ascending order of the values, -0 before +0; every NaN takes the
// last key and sorts last, like numpy
__device__ __forceinline__ uint32_t radix_key(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return v != v ? 0xFFFFFFFFu : k;
}
__device__ __forceinline__ float radix_unkey(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// one wave per selection i (its 256-bin histogram of the digit at `shift`, the rank remaining on its prefix): lane l holds bins
// 4 l .. 4 l + 3, a wave prefix sum finds the lane and that lane the digit in which the rank falls; the prefix is extended, the
// counts below the digit are subtracted and, with `values`, the value the prefix now encodes is written.  A rank at or past the
// number counted takes the maximum.  (static: one copy per including unit)
static __global__ __launch_bounds__(64) void radix_advance_kernel(const long long* __restrict__ hist,
                                                                  long long* __restrict__ remaining,
                                                                  uint32_t* __restrict__ prefix, int n, int shift,
                                                                  float* __restrict__ values) {
  static_assert(kRadixBins == 4 * 64, "four bins per lane");
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const long long* h = hist + (long long)i * kRadixBins + 4 * lane;
  long long c[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) c[b] = h[b];
  const long long mine = c[0] + c[1] + c[2] + c[3];
  long long incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o *= 2) {
    const long long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const long long total = __shfl(incl, 63, 64);
  long long rem = remaining[i];
  if (rem < 0) rem = 0;
  if (rem >= total) rem = total - 1;
  // nothing counted: cannot happen -- l2hmc_order_stats* and l2hmc_logistic_loo_tails refuse n_draws < 1 before anything is
  // launched, and every draw of a selection is counted in its first pass
  if (total <= 0) {
    if (lane == 0) { remaining[i] = 0; if (values) values[i] = __uint_as_float(~prefix[i]); }
    return;
  }
  long long below = incl - mine;
  if (rem < below || rem >= incl) return;             // exactly one lane holds the rank
  int digit = 4 * lane;
#pragma unroll
  for (int b = 0; b < 3; ++b)
    if (rem >= below + c[b] && digit == 4 * lane + b) { below += c[b]; ++digit; }
  const uint32_t key = prefix[i] | ((uint32_t)digit << shift);
  prefix[i] = key;
  remaining[i] = rem - below;
  if (values) values[i] = radix_unkey(key);
}

// ---- the count pass over a workgroup's LDS histogram hl[rows][kRadixBins] -------------------------------------------------------
template <int ROWS, int THREADS>
__device__ __forceinline__ void radix_hist_clear(uint32_t* hl) {
  for (int i = threadIdx.x; i < ROWS * kRadixBins; i += THREADS) hl[i] = 0u;
}

// pass 0: every key counts and the top digit (sign and high exponent) concentrates in a few bins -- the 16 draw lanes c of a row
// would add to one address.  They compare their bin with the first lane's; those that agree are counted by a ballot and added
// by that lane in ONE atomic, the others add for themselves.
__device__ __forceinline__ void radix_count_first(uint32_t* hrow, uint32_t key, bool ok, int lane, int c) {
  const int bin = (int)(key >> 24);
  const int lead = __shfl(bin, lane & 48, 64);
  const bool same = ok && bin == lead;
  const unsigned long long bal = __ballot(same);
  const int cnt = __popc((unsigned)((bal >> (lane & 48)) & 0xFFFFull));
  if (c == 0) { if (cnt) atomicAdd(&hrow[lead], (uint32_t)cnt); }
  else if (ok && !same) atomicAdd(&hrow[bin], 1u);
}

// later passes: only the keys on the row's prefix (pre_key = prefix >> (shift + kRadixBits)) count: few, plain atomics
__device__ __forceinline__ void radix_count_next(uint32_t* hrow, uint32_t key, bool ok, int shift, uint32_t pre_key) {
  if (ok && (key >> (shift + kRadixBits)) == pre_key) atomicAdd(&hrow[(key >> shift) & (kRadixBins - 1)], 1u);
}

// once every wave has counted: the non-zero bins of rows 16 b0 .. 16 b0 + ROWS - 1 below n go to hist (n, kRadixBins)
template <int ROWS, int THREADS>
__device__ __forceinline__ void radix_hist_flush(const uint32_t* hl, int b0, int n, unsigned long long* __restrict__ hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < ROWS * kRadixBins; i += THREADS) {
    const uint32_t cnt = hl[i];
    const int row = 16 * b0 + (i >> kRadixBits);
    if (cnt && row < n) atomicAdd(&hist[(long long)row * kRadixBins + (i & (kRadixBins - 1))], (unsigned long long)cnt);
  }
}

// ---- the four passes, on the host ----------------------------------------------------------------------------------------------
// per pass: hist (n, kRadixBins) zeroed, count(shift, first) -- the caller's launch of its count kernel -- and the advance; the
// last advance writes the cutoffs.  L2HMC_OK, or the memset's error with the message set.
template <class Count>
int radix_select_passes(unsigned long long* hist, long long* remaining, uint32_t* prefix, int n, float* cutoff, hipStream_t s,
                        Count&& count) {
  for (int pass = 0; pass < kRadixPasses; ++pass) {
    const int shift = 32 - kRadixBits * (pass + 1);
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * kRadixBins * sizeof(long long), s);
    if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    count(shift, pass == 0);
    hipLaunchKernelGGL(radix_advance_kernel, dim3((unsigned)n), dim3(64), 0, s, (const long long*)hist, remaining, prefix, n, shift,
                       pass == kRadixPasses - 1 ? cutoff : (float*)nullptr);
  }
  return L2HMC_OK;
}

}  // namespace l2hmc
