// l2hmc_chain_stats -- the raw sums behind split R-hat and the per-coordinate effective sample size (Vehtari, Gelman, Simpson,
// Carpenter, Buerkner 2021, without rank normalisation) of a recorded history X (steps, N, d) that stays where the sampler
// wrote it.  l2hmc_amd/diagnostics.py turns the sums into numbers; include/l2hmc.h states the contract.
//
// A history row is J = N d contiguous floats and series j = (chain n, coordinate k = j mod d) is column j of the (steps, J)
// matrix, so in both passes thread <-> column: the 256 threads of a block read 1 KiB of a row, fully coalesced, for any d.  With
// `split` every column is two series (rows [0, Mh) and [steps - Mh, steps)): blockIdx.z is the half.
//
//   pass 1  chain_moments_kernel: m and M2 = sum (x - m)^2 of every series, float64 throughout, one thread per series
//           (no cross-thread sum at all).
//   pass 2  chain_lagsum_kernel: G[k, t] = sum over the series of coordinate k of sum_i (x_i - m)(x_{i+t} - m).  A block is 256
//           columns x one tile of 32 lags.  Every thread keeps the 32 centred values x_{t+tau0} .. x_{t+tau0+31} in registers as a
//           ring with compile-time indices (the step loop is unrolled by 32), so a step costs one load for the ring (issued 32
//           steps before its first use), one for x_t (none in the first tile, where x_t is the ring's head) and 32 FMAs -- the
//           row is loaded once per lag TILE.  Values are centred in float64 and rounded to float32 once; products accumulate in
//           float32 over 32 steps and are then folded into float64 (error <= 32 * 2^-24 of sum |products| <= G[k, 0]).
//           Values past the end of the series enter as 0, which is all the "i < Mh - t" bound needs.
//           The per-coordinate reduction happens ONCE per block, after the loop: a block walks the column chunks b, b + nb,
//           b + 2 nb, ... where nb is a multiple of the period of (256 b) mod d, so a thread's coordinate never changes and its
//           32 float64 sums stay in registers across chunks; at the end the block adds, through LDS and in a fixed order, the
//           threads that share a coordinate and writes one partial per (slot = first column of that coordinate, lag) to the
//           workspace.
//   pass 3  chain_lagsum_reduce_kernel: G[k, t] = the blocks' partials added in block order.  No floating-point atomics anywhere:
//           the result is bitwise reproducible.
//
// l2hmc_chain_stats_below: the same three passes on the indicator series y = [x <= thresholds[coordinate]] (the effective sample
// size of a quantile estimate, l2hmc_amd/quantiles.py).  The device functions take the transform as a functor (CsValue, CsBelow);
// chain_moments_below_kernel and chain_lagsum_below_kernel are kernels of their own, pass 3 is shared as it is.
//
// l2hmc_chain_stats_exp: a third functor, CsExp -- the series y = (float) exp((double) x - shift[coordinate]), the likelihoods
// of a log-likelihood history (l2hmc_amd/psis.py `relative_eff_from_log_lik`; the shift, the column's maximum, only keeps e^x
// inside float32: the effective sample size does not move with it).  The double `exp` is evaluated as the value is loaded,
// once per pass and lag tile: chain_moments_exp_kernel and chain_lagsum_exp_kernel, pass 3 shared again.
#include <math.h>
#include "l2hmc_kernels.hpp"

namespace l2hmc {

constexpr int kCsThreads = 256;   // columns per block
constexpr int kCsLags = 32;       // lags per block = length of the register ring
constexpr int kCsLdsLags = 8;     // lags per round of the block-end reduction (8 x 256 doubles = 16 KiB of LDS)
constexpr int kCsBlocks = 1024;   // blocks the planner aims for (about one resident set of the 256 CUs)

struct ChainStatsPlan {
  long long Mh, C, J, row0[2];    // series length, series per coordinate, columns, first row of each half
  int halves, nslot;              // 1 or 2; coordinates a block can hold = min(d, 256)
  long long nchunks, nb, ntile;   // column chunks, blocks along x (chunk b, b + nb, ...), lag tiles
};

// the host's plan of a call; false (with the message set) when the arguments are not a valid request
static bool chain_stats_plan(const char* who, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                             ChainStatsPlan& p) {
  if (steps < 1 || n_chains < 1 || d < 1 || (split != 0 && split != 1)) {
    fail(L2HMC_ERR_ARG, "%s: steps, n_chains, d must be >= 1 and split 0 or 1", who);
    return false;
  }
  if (d > 512) { fail(L2HMC_ERR_ARG, "%s: d <= 512 (got %lld)", who, d); return false; }
  p.halves = split ? 2 : 1;
  p.Mh = split ? steps / 2 : steps;
  p.C = n_chains * p.halves;
  if (p.Mh < 4 || p.C < 2) {
    fail(L2HMC_ERR_ARG, "%s: needs >= 4 steps per (split) chain and >= 2 chains (got %lld, %lld)", who, p.Mh, p.C);
    return false;
  }
  if (max_lag < 0 || max_lag > p.Mh - 1) {
    fail(L2HMC_ERR_ARG, "%s: 0 <= max_lag <= steps per chain - 1 = %lld (got %lld)", who, p.Mh - 1, max_lag);
    return false;
  }
  if (n_chains > (1LL << 40) / d || steps > (1LL << 31)) { fail(L2HMC_ERR_ARG, "%s: history too large", who); return false; }
  p.J = n_chains * d;
  p.row0[0] = 0;
  p.row0[1] = steps - p.Mh;
  p.nslot = d < kCsThreads ? d : kCsThreads;
  p.nchunks = (p.J + kCsThreads - 1) / kCsThreads;
  p.ntile = ((long long)max_lag + kCsLags) / kCsLags;
  // (256 b) mod d repeats with period d / gcd(256, d): chunks a multiple of it apart map threads to the same coordinates
  long long g = d, r = kCsThreads;
  while (r) { const long long t = g % r; g = r; r = t; }
  const long long period = d / g;
  const long long want = (kCsBlocks + p.ntile * p.halves - 1) / (p.ntile * p.halves);
  p.nb = ((want + period - 1) / period) * period;
  if (p.nb > p.nchunks) p.nb = p.nchunks;             // one chunk per block: nothing to keep aligned
  if (p.nchunks > 0x7fffffffLL || p.ntile > 65535) { fail(L2HMC_ERR_ARG, "%s: history too large", who); return false; }
  return true;
}

// What a series is made of: the recorded value itself, or (l2hmc_chain_stats_below) the indicator of "at or below the
// coordinate's threshold", applied as the value is loaded.  The comparison is in float64: an indicator flips discretely.
struct CsValue {
  __device__ __forceinline__ float operator()(float v) const { return v; }
};
struct CsBelow {
  double thr;
  __device__ __forceinline__ float operator()(float v) const { return (double)v <= thr ? 1.f : 0.f; }
};
struct CsExp {
  double shift;
  __device__ __forceinline__ float operator()(float v) const { return (float)exp((double)v - shift); }
};

// ---- pass 1 ---------------------------------------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void cs_moments(const float* __restrict__ X, long long J, long long Mh, long long row1, long long j,
                                           double* __restrict__ mean_out, double* __restrict__ m2_out, const F f) {
  const float* col = X + (blockIdx.y ? row1 : 0) * J + j;
  double s = 0.0;
  long long t = 0;
  for (; t + 8 <= Mh; t += 8) {                       // 8 independent loads in flight per thread, added in row order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = f(col[(t + u) * J]);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (double)v[u];
  }
  for (; t < Mh; ++t) s += (double)f(col[t * J]);
  const double m = s / (double)Mh;
  double q = 0.0;
  for (t = 0; t + 8 <= Mh; t += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = f(col[(t + u) * J]);
#pragma unroll
    for (int u = 0; u < 8; ++u) { const double c = (double)v[u] - m; q = fma(c, c, q); }
  }
  for (; t < Mh; ++t) { const double c = (double)f(col[t * J]) - m; q = fma(c, c, q); }
  const long long o = (long long)blockIdx.y * J + j;  // (C, d) with chain = half * N + n
  mean_out[o] = m;
  m2_out[o] = q;
}

__global__ __launch_bounds__(kCsThreads) void chain_moments_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                   long long row1, double* __restrict__ mean_out,
                                                                   double* __restrict__ m2_out) {
  const long long j = (long long)blockIdx.x * kCsThreads + threadIdx.x;
  if (j >= J) return;
  cs_moments(X, J, Mh, row1, j, mean_out, m2_out, CsValue());
}

__global__ __launch_bounds__(kCsThreads) void chain_moments_below_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                         long long row1, int d,
                                                                         const double* __restrict__ thresholds,
                                                                         double* __restrict__ mean_out,
                                                                         double* __restrict__ m2_out) {
  const long long j = (long long)blockIdx.x * kCsThreads + threadIdx.x;
  if (j >= J) return;
  cs_moments(X, J, Mh, row1, j, mean_out, m2_out, CsBelow{thresholds[j % d]});
}

__global__ __launch_bounds__(kCsThreads) void chain_moments_exp_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                       long long row1, int d, const double* __restrict__ shift,
                                                                       double* __restrict__ mean_out,
                                                                       double* __restrict__ m2_out) {
  const long long j = (long long)blockIdx.x * kCsThreads + threadIdx.x;
  if (j >= J) return;
  cs_moments(X, J, Mh, row1, j, mean_out, m2_out, CsExp{shift[j % d]});
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------
// centred in float64, rounded to float32 once; `keep` is 1 for a row of the series and 0 past its end
__device__ __forceinline__ float cs_centre(float v, double m, float keep) { return (float)((double)v - m) * keep; }

// One series against one lag tile.  The ring w holds x_{t + tau0 + l} at w[(u + l) % 32] in step t = tb + u; o0 walks the rows
// of x_t and o1 those of the ring's refill x_{t + tau0 + 32}, one row per step, and both stop at the last row of the series, so
// every load is in bounds.  A value past the end enters as 0 through a wave-uniform factor, not a branch: the loads of a whole
// block of 32 steps are independent of its arithmetic and can all be in flight.  (A series with a non-finite last row is NaN
// with or without the factor.)  kFirst: tau0 = 0, x_t is the ring's head and is not loaded again.
template <bool kFirst, class F>
__device__ __forceinline__ void cs_series(const float* __restrict__ X, long long o, long long J, long long tau0, long long Mh,
                                          double m, double (&dacc)[kCsLags], const F f) {
  float w[kCsLags], acc[kCsLags];
  const long long last = Mh - 1;
  long long o0 = o, o1 = o + (tau0 < last ? tau0 : last) * J;
#pragma unroll
  for (int l = 0; l < kCsLags; ++l) {
    const long long r = tau0 + l;
    w[l] = cs_centre(f(X[o1]), m, r < Mh ? 1.f : 0.f);
    o1 += r < last ? J : 0;
    asm volatile("" : "+v"(o1));
    if (l % 8 == 7) __builtin_amdgcn_sched_barrier(0);       // 8 loads in flight at a time, not 32 addresses and values
    acc[l] = 0.f;
  }
  for (long long tb = 0; tb < Mh - tau0; tb += kCsLags) {    // x_t with t >= Mh - tau0 only meets zeros
#pragma unroll
    for (int u = 0; u < kCsLags; ++u) {
      const long long t = tb + u, t1 = t + tau0 + kCsLags;
      float x0;
      if (kFirst) {
        x0 = w[u];
      } else {
        x0 = cs_centre(f(X[o0]), m, t < Mh ? 1.f : 0.f);
        o0 += t < last ? J : 0;
      }
#pragma unroll
      for (int l = 0; l < kCsLags; ++l) acc[l] = fmaf(x0, w[(u + l) % kCsLags], acc[l]);
      w[u] = cs_centre(f(X[o1]), m, t1 < Mh ? 1.f : 0.f);
      o1 += t1 < last ? J : 0;
      // keep the walk a vector add per step: left alone, the compiler forms 64 row offsets u J in scalar registers, runs out of
      // them and moves them through lanes of a vector register inside the loop
      asm volatile("" : "+v"(o0), "+v"(o1));
    }
#pragma unroll
    for (int l = 0; l < kCsLags; ++l) { dacc[l] += (double)acc[l]; acc[l] = 0.f; }
  }
}

// kSeries 1: the series are indicators of "at or below thresholds[coordinate]" (a thread's coordinate never changes across
// chunks); 2: they are exp(x - thresholds[coordinate]), the argument then being the shift; 0: the values themselves
template <int kSeries>
__device__ __forceinline__ void cs_lagsum(const float* __restrict__ X, long long J, long long Mh, long long row1, int d, int nslot,
                                          long long nchunks, int max_lag, const double* __restrict__ mean,
                                          const double* __restrict__ thresholds, double* __restrict__ part) {
  __shared__ double sm[kCsLdsLags][kCsThreads];
  const int tid = threadIdx.x;
  const long long nb = gridDim.x, tau0 = (long long)blockIdx.y * kCsLags;
  const int half = blockIdx.z;
  const float* base = X + (half ? row1 : 0) * J;
  double dacc[kCsLags];
#pragma unroll
  for (int l = 0; l < kCsLags; ++l) dacc[l] = 0.0;

  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += nb) {
    const long long j = chunk * kCsThreads + tid;
    if (j >= J) continue;
    const double m = mean[(long long)half * J + j];
    // the end-of-series factors and row steps of a series depend on (tau0, Mh) alone; seen as loop invariants they are hoisted
    // out of this loop and held in ~100 vector registers across it.  They cost a scalar compare each: recompute them per chunk.
    long long mh = Mh;
    asm volatile("" : "+s"(mh));
    if constexpr (kSeries == 1) {
      const CsBelow f{thresholds[j % d]};
      if (tau0 == 0) cs_series<true>(base, j, J, tau0, mh, m, dacc, f);
      else cs_series<false>(base, j, J, tau0, mh, m, dacc, f);
    } else if constexpr (kSeries == 2) {
      const CsExp f{thresholds[j % d]};
      if (tau0 == 0) cs_series<true>(base, j, J, tau0, mh, m, dacc, f);
      else cs_series<false>(base, j, J, tau0, mh, m, dacc, f);
    } else {
      if (tau0 == 0) cs_series<true>(base, j, J, tau0, mh, m, dacc, CsValue());
      else cs_series<false>(base, j, J, tau0, mh, m, dacc, CsValue());
    }
  }

  // threads tid, tid + d, tid + 2 d, ... hold the same coordinate: add them in that order, 8 lags per round
  const long long blk = (long long)half * nb + blockIdx.x;
  const long long nlag = (long long)max_lag + 1;
#pragma unroll
  for (int g = 0; g < kCsLags / kCsLdsLags; ++g) {
    __syncthreads();
#pragma unroll
    for (int l = 0; l < kCsLdsLags; ++l) sm[l][tid] = dacc[g * kCsLdsLags + l];
    __syncthreads();
    for (int p = tid; p < nslot * kCsLdsLags; p += kCsThreads) {
      const int l = p / nslot, slot = p - l * nslot;
      double a = sm[l][slot];
      for (int o = slot + d; o < kCsThreads; o += d) a += sm[l][o];
      const long long lag = tau0 + g * kCsLdsLags + l;
      if (lag < nlag) part[(blk * nslot + slot) * nlag + lag] = a;
    }
  }
}

__global__ __launch_bounds__(kCsThreads) void chain_lagsum_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                  long long row1, int d, int nslot, long long nchunks,
                                                                  int max_lag, const double* __restrict__ mean,
                                                                  double* __restrict__ part) {
  cs_lagsum<0>(X, J, Mh, row1, d, nslot, nchunks, max_lag, mean, nullptr, part);
}

__global__ __launch_bounds__(kCsThreads) void chain_lagsum_below_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                        long long row1, int d, int nslot, long long nchunks,
                                                                        int max_lag, const double* __restrict__ mean,
                                                                        const double* __restrict__ thresholds,
                                                                        double* __restrict__ part) {
  cs_lagsum<1>(X, J, Mh, row1, d, nslot, nchunks, max_lag, mean, thresholds, part);
}

__global__ __launch_bounds__(kCsThreads) void chain_lagsum_exp_kernel(const float* __restrict__ X, long long J, long long Mh,
                                                                      long long row1, int d, int nslot, long long nchunks,
                                                                      int max_lag, const double* __restrict__ mean,
                                                                      const double* __restrict__ shift,
                                                                      double* __restrict__ part) {
  cs_lagsum<2>(X, J, Mh, row1, d, nslot, nchunks, max_lag, mean, shift, part);
}

// ---- pass 3 ---------------------------------------------------------------------------------------------------------------
// G[k, lag] = sum over (half, block) in that order of the partial of the slot that holds coordinate k in that block
__global__ void chain_lagsum_reduce_kernel(const double* __restrict__ part, long long nblk, long long nb, int d, int nslot,
                                           long long nlag, double* __restrict__ G) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)d * nlag) return;
  const int k = (int)(i / nlag);
  const long long lag = i - (long long)k * nlag;
  double a = 0.0;
#pragma unroll 8
  for (long long b = 0; b < nblk; ++b) {
    // slot s of block b starts at column 256 (b mod nb) + s, whose coordinate is (256 (b mod nb) + s) mod d
    const int first = (int)(((b % nb) * kCsThreads) % d);
    const int slot = k >= first ? k - first : k - first + d;
    a += slot < nslot ? part[(b * nslot + slot) * nlag + lag] : 0.0;
  }
  G[i] = a;
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_chain_stats_workspace_doubles(int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split) {
  ChainStatsPlan p;
  if (!chain_stats_plan("l2hmc_chain_stats_workspace_doubles", steps, n_chains, d, max_lag, split, p)) return L2HMC_ERR_ARG;
  return p.nb * p.halves * p.nslot * ((int64_t)max_lag + 1);
}

int l2hmc_chain_stats(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                      double* mean_out, double* m2_out, double* G_out, double* workspace, void* stream) {
  ChainStatsPlan p;
  if (!chain_stats_plan("l2hmc_chain_stats", steps, n_chains, d, max_lag, split, p)) return L2HMC_ERR_ARG;
  if (!X || !mean_out || !m2_out || !G_out || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_chain_stats: X, mean_out, m2_out, G_out and workspace are required%s");
  hipStream_t s = (hipStream_t)stream;
  const long long nlag = (long long)max_lag + 1;
  hipLaunchKernelGGL(chain_moments_kernel, dim3((unsigned)p.nchunks, (unsigned)p.halves), dim3(kCsThreads), 0, s, X, p.J, p.Mh,
                     p.row0[1], mean_out, m2_out);
  hipLaunchKernelGGL(chain_lagsum_kernel, dim3((unsigned)p.nb, (unsigned)p.ntile, (unsigned)p.halves), dim3(kCsThreads), 0, s, X,
                     p.J, p.Mh, p.row0[1], (int)d, p.nslot, p.nchunks, (int)max_lag, (const double*)mean_out, workspace);
  hipLaunchKernelGGL(chain_lagsum_reduce_kernel, dim3((unsigned)((d * nlag + 255) / 256)), dim3(256), 0, s,
                     (const double*)workspace, p.nb * p.halves, p.nb, (int)d, p.nslot, nlag, G_out);
  return launched();
}

int l2hmc_chain_stats_below(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                            const double* thresholds, double* mean_out, double* m2_out, double* G_out, double* workspace,
                            void* stream) {
  ChainStatsPlan p;
  if (!chain_stats_plan("l2hmc_chain_stats_below", steps, n_chains, d, max_lag, split, p)) return L2HMC_ERR_ARG;
  if (!X || !thresholds || !mean_out || !m2_out || !G_out || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_chain_stats_below: X, thresholds, mean_out, m2_out, G_out and workspace are required%s");
  hipStream_t s = (hipStream_t)stream;
  const long long nlag = (long long)max_lag + 1;
  hipLaunchKernelGGL(chain_moments_below_kernel, dim3((unsigned)p.nchunks, (unsigned)p.halves), dim3(kCsThreads), 0, s, X, p.J,
                     p.Mh, p.row0[1], (int)d, thresholds, mean_out, m2_out);
  hipLaunchKernelGGL(chain_lagsum_below_kernel, dim3((unsigned)p.nb, (unsigned)p.ntile, (unsigned)p.halves), dim3(kCsThreads), 0,
                     s, X, p.J, p.Mh, p.row0[1], (int)d, p.nslot, p.nchunks, (int)max_lag, (const double*)mean_out, thresholds,
                     workspace);
  hipLaunchKernelGGL(chain_lagsum_reduce_kernel, dim3((unsigned)((d * nlag + 255) / 256)), dim3(256), 0, s,
                     (const double*)workspace, p.nb * p.halves, p.nb, (int)d, p.nslot, nlag, G_out);
  return launched();
}

int l2hmc_chain_stats_exp(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                          const double* shift, double* mean_out, double* m2_out, double* G_out, double* workspace,
                          void* stream) {
  ChainStatsPlan p;
  if (!chain_stats_plan("l2hmc_chain_stats_exp", steps, n_chains, d, max_lag, split, p)) return L2HMC_ERR_ARG;
  if (!X || !shift || !mean_out || !m2_out || !G_out || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_chain_stats_exp: X, shift, mean_out, m2_out, G_out and workspace are required%s");
  hipStream_t s = (hipStream_t)stream;
  const long long nlag = (long long)max_lag + 1;
  hipLaunchKernelGGL(chain_moments_exp_kernel, dim3((unsigned)p.nchunks, (unsigned)p.halves), dim3(kCsThreads), 0, s, X, p.J,
                     p.Mh, p.row0[1], (int)d, shift, mean_out, m2_out);
  hipLaunchKernelGGL(chain_lagsum_exp_kernel, dim3((unsigned)p.nb, (unsigned)p.ntile, (unsigned)p.halves), dim3(kCsThreads), 0,
                     s, X, p.J, p.Mh, p.row0[1], (int)d, p.nslot, p.nchunks, (int)max_lag, (const double*)mean_out, shift,
                     workspace);
  hipLaunchKernelGGL(chain_lagsum_reduce_kernel, dim3((unsigned)((d * nlag + 255) / 256)), dim3(256), 0, s,
                     (const double*)workspace, p.nb * p.halves, p.nb, (int)d, p.nslot, nlag, G_out);
  return launched();
}

}  // extern "C"
