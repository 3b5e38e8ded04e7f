// The most-significant-digit radix select both order_stats.hip and loo.hip run on float32 values, stated once: the monotone key
// and the advance step between two count passes.  kRadixPasses = 4 passes of kRadixBits = 8 bits.
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

}  // namespace l2hmc
