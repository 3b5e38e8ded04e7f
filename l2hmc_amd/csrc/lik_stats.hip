// l2hmc_logistic_lik_stats -- the raw sums behind the per-row RELATIVE EFFICIENCY of PSIS-LOO (Vehtari, Gelman, Gabry 2017:
// r_eff_i = ESS(p(y_i | theta)) / S) of Bayesian logistic regression, from a history W (steps, N, d) that stays where the sampler
// wrote it.  The series are the likelihoods lik_{t,c,i} = sigmoid(t_{t,c,i}), t = (2 y_i - 1) x_i . w_{t,c} the signed logit of
// row i under the draw of chain c at step t, and the outputs are those of l2hmc_chain_stats (chain_stats.hip) for that derived
// history with "coordinate" = data row: mean and M2 per (chain, row), lag sums G per (row, lag).  l2hmc_amd/diagnostics.py
// `reduce_sums` / `finish` take them unchanged; include/l2hmc.h states the contract.  The (steps, N, n) array of likelihoods is
// never written: the logit contraction of draw_tiles.hpp is fused with chain_stats' two passes.
//
// Work unit = one WAVE: 16 consecutive chains x ONE 16-row data block, walking the steps.  The draw tile of step t is the 16 d
// contiguous floats at draw t N + c0 (tile_load_at: chains at or past N enter as 0 and are masked below, as a draw past S is in
// predict_kernel).  The logits come from tile_logits ALONE -- the bits the LOO passes see -- and the likelihood from
// BernoulliLogit::lik (glm_family.hpp), the function loo_kernel's gather calls.  Lane (c, q) holds the four series (chain
// c0 + c, rows 4 q + r).
//
//   pass 1  lik_moments_kernel: two walks over the steps, float64 throughout: m = sum lik / Mh, then M2 = sum (lik - m)^2 (fma).
//           Every lane writes its own four (chain, row) entries: no cross-lane sum at all.
//   pass 2  lik_lagsum_kernel: a wave is (chain blocks xb, xb + nbx, ..., one data block, one tile of kLsLags = 8 lags, one
//           half).  Per series a register ring holds the centred values x_{t + tau0} .. x_{t + tau0 + 7} with compile-time indices
//           (the step loop is unrolled by 8).  Values are centred in float64 and rounded to float32 once; products accumulate in
//           float32 over 8 steps and are then folded into float64 (error <= 8 * 2^-24 of sum |products| <= G[i, 0], inside the
//           32 * 2^-24 that chain_stats.hip states).  A step costs one contraction for the ring's refill x_{t + tau0 + 8} and one
//           for x_t (none in the first tile, where x_t is the ring's head): the contraction is redone per lag tile.  A step past
//           the end of the series loads the last step again and enters as 0 through a select: the step loop has no branch and
//           the MFMAs always run with every lane.
//           The float64 sums stay in registers across the wave's chain blocks; at the end the 16 chain lanes are added through
//           LDS in the order c = 0 .. 15 and one partial per (half, xb, row, lag) goes to the workspace.
//   pass 3  chunk_reduce_kernel: G[i, lag] = the partials added in (half, xb) order.  No floating-point atomics anywhere.
// nbx = min(chain blocks, kLsWalks) depends on N ALONE, and a row's numbers on that row and the draws alone (an MFMA output
// element is the dot product of its own row and column): the results are bitwise reproducible and do not depend on how the
// caller groups rows.
//
// Occupancy by design: 1 wave per SIMD in pass 2 (one workgroup of four independent waves per CU).  A lane holds 4 series x 8
// lags of ring, float32 sums and float64 sums (32 + 32 + 64 registers), the fragments and two tiles in flight, and the compiler
// keeps the unrolled steps' staging addresses and values beside them: 300 .. 490 registers by its listing, more than the 256 of
// two waves per SIMD, so the kernel is given the whole unified file of 512.  It must use NO scratch, and pass 1 must stay within
// 256 registers (both held by tests/test_lik_stats_cpu.py from the compiler's listing).  A 16-lag ring spilled at every geometry.
// LDS: 4 x at most 8448 bytes.  Geometries <NTM feature tiles compiled>: 1, 2, 4, 8.
#include "draw_tiles.hpp"
#include "glm_family.hpp"

namespace l2hmc {

constexpr int kLsThreads = 256;   // 4 independent waves
constexpr int kLsLags = 8;        // lags per wave = length of the register ring
constexpr int kLsWalks = 16;      // chain-block walkers per (data block, lag tile, half) at most: the workspace's depth

struct LikStatsPlan {
  int NT, NTM, nblk, halves;
  long long Mh, row1, ncb, nbx, ntile, nlag;
};

// the argument errors of chain_stats_plan (chain_stats.hip) and of logistic_history_args_ok; false with the message set
static bool lik_stats_plan(const char* who, int64_t steps, int64_t n_chains, int32_t d, int32_t n_data, int32_t max_lag,
                           int32_t split, LikStatsPlan& p) {
  if (steps < 1 || n_chains < 1 || d < 1 || (split != 0 && split != 1)) {
    fail(L2HMC_ERR_ARG, "%s: steps, n_chains, d must be >= 1 and split 0 or 1", who);
    return false;
  }
  if (steps > (1LL << 31) || n_chains > (1LL << 40) / steps) { fail(L2HMC_ERR_ARG, "%s: history too large", who); return false; }
  if (!logistic_history_args_ok(who, steps * n_chains, n_data, d)) return false;
  p.halves = split ? 2 : 1;
  p.Mh = split ? steps / 2 : steps;
  if (p.Mh < 4 || n_chains * p.halves < 2) {
    fail(L2HMC_ERR_ARG, "%s: needs >= 4 steps per (split) chain and >= 2 chains (got %lld, %lld)", who, p.Mh, n_chains * p.halves);
    return false;
  }
  if (max_lag < 0 || max_lag > p.Mh - 1) {
    fail(L2HMC_ERR_ARG, "%s: 0 <= max_lag <= steps per chain - 1 = %lld (got %lld)", who, p.Mh - 1, max_lag);
    return false;
  }
  p.row1 = steps - p.Mh;
  p.NT = tiles_of(d);
  p.NTM = draw_ntm(p.NT);
  p.nblk = (n_data + 15) / 16;
  p.ncb = (n_chains + 15) / 16;
  p.nbx = p.ncb < kLsWalks ? p.ncb : kLsWalks;            // a function of n_chains alone
  p.nlag = (long long)max_lag + 1;
  p.ntile = (p.nlag + kLsLags - 1) / kLsLags;
  if (p.ntile > 65535) { fail(L2HMC_ERR_ARG, "%s: max_lag too large (more than 65535 lag tiles)", who); return false; }
  return true;
}

// the likelihoods of the loaded tile: lane (c, q) gets sigmoid(t) of chain c, rows 4 q + r of data block b -- the logits of
// tile_logits through BernoulliLogit::lik, as loo_kernel's gather forms them
template <int NTM>
__device__ __forceinline__ f4 lik_of_tile(float* lds, const float (&pre)[4 * NTM], const TileWalk& walk, int lane,
                                          const f4 (&xa)[1][NTM], const f4& yv, int NT, int b, int nblk) {
  tile_stage<NTM>(lds, pre, walk, lane);
  wave_lds_fence();
  f4 T[1];
  tile_logits<NTM, 1>(lds, xa, lane & 15, lane >> 4, NT, b, nblk, T);
  wave_lds_fence();
  f4 out;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[r] = BernoulliLogit::lik(BernoulliLogit::signed_logit(T[0][r], yv[r]));
  return out;
}

// ---- pass 1 ---------------------------------------------------------------------------------------------------------------
template <int NTM>
__global__ __launch_bounds__(kLsThreads) void lik_moments_kernel(const float* __restrict__ W, long long N, int d,
                                                                 const float* __restrict__ P, int n, int NT, long long Mh,
                                                                 long long row1, long long ncb, int halves,
                                                                 double* __restrict__ mean_out, double* __restrict__ m2_out) {
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int nblk = (n + 15) >> 4;
  const long long u = (long long)blockIdx.x * 4 + w;
  if (u >= ncb * nblk * halves) return;                      // (no workgroup barrier anywhere: a wave may leave alone)
  float* lds = lds_all + w * REGION;
  tile_region_clear<NTM>(lds, lane);
  const int b = (int)(u % nblk);
  const long long cb = (u / nblk) % ncb;
  const int half = (int)(u / nblk / ncb);
  const long long c0 = cb * 16, first = (half ? row1 : 0) * N + c0;
  const int live = N - c0 < 16 ? (int)(N - c0) : 16;

  f4 xa[1][NTM], yv[1];
  block_fragments<NTM, 1>(P, NT, b, nblk, lane, xa, yv);
  const TileWalk walk = tile_walk(lane, d, 0);
  float pre[4 * NTM];
  double s[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0}, m[4];

  tile_load_at<NTM>(W, first, live, walk, lane, pre);
#pragma unroll 1
  for (long long t = 0; t < Mh; ++t) {
    const f4 lik = lik_of_tile<NTM>(lds, pre, walk, lane, xa, yv[0], NT, b, nblk);
    tile_load_at<NTM>(W, first + (t + 1 < Mh ? t + 1 : t) * N, live, walk, lane, pre);    // in flight during the arithmetic
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] += (double)lik[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) m[r] = s[r] / (double)Mh;
  tile_load_at<NTM>(W, first, live, walk, lane, pre);
#pragma unroll 1
  for (long long t = 0; t < Mh; ++t) {
    const f4 lik = lik_of_tile<NTM>(lds, pre, walk, lane, xa, yv[0], NT, b, nblk);
    tile_load_at<NTM>(W, first + (t + 1 < Mh ? t + 1 : t) * N, live, walk, lane, pre);
#pragma unroll
    for (int r = 0; r < 4; ++r) { const double z = (double)lik[r] - m[r]; m2[r] = fma(z, z, m2[r]); }
  }
  if (c < live) {
    const long long o = ((long long)half * N + c0 + c) * n;  // (C, n) with chain = half * N + chain
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * b + 4 * q + r;
      if (row < n) { mean_out[o + row] = m[r]; m2_out[o + row] = m2[r]; }
    }
  }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------
// centred in float64, rounded to float32 once; `keep`: a step of the series and a chain of the history
__device__ __forceinline__ float ls_centre(float lik, double m, bool keep) { return keep ? (float)((double)lik - m) : 0.f; }

// The four series of a lane (one chain block) against one lag tile.  Stream B refills the ring (step t + tau0 + kLsLags), stream
// A supplies x_t; both keep one tile in flight and share the wave's LDS region in turn.  `first` is the draw of (step 0, chain
// c0) of the half.  A step past the end of the series loads the last step again and enters as 0 through a select, not a
// branch: the step loop is straight-line code.  kFirst: tau0 = 0, x_t is the ring's head and stream A does not exist.
template <int NTM, bool kFirst>
__device__ __forceinline__ void lik_series(const float* __restrict__ W, long long N, long long first, int live, bool chain_ok,
                                           long long Mh, long long tau0, const double (&m)[4], float* lds, const TileWalk& walk,
                                           int lane, const f4 (&xa)[1][NTM], const f4& yv, int NT, int b, int nblk,
                                           double (&dacc)[4][kLsLags]) {
  float ring[4][kLsLags], acc[4][kLsLags], preA[4 * NTM], preB[4 * NTM];
  const long long last = Mh - 1;
  tile_load_at<NTM>(W, first + tau0 * N, live, walk, lane, preB);                       // tau0 <= Mh - 1
#pragma unroll
  for (int l = 0; l < kLsLags; ++l) {
    const long long sb = tau0 + l, nx = sb + 1 < last ? sb + 1 : last;
    const f4 lik = lik_of_tile<NTM>(lds, preB, walk, lane, xa, yv, NT, b, nblk);
    tile_load_at<NTM>(W, first + nx * N, live, walk, lane, preB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ring[r][l] = ls_centre(lik[r], m[r], sb < Mh && chain_ok);
      acc[r][l] = 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);                       // one step's loads and values in flight, not the unrolled loop's
  }
  if (!kFirst) tile_load_at<NTM>(W, first, live, walk, lane, preA);
  for (long long tb = 0; tb < Mh - tau0; tb += kLsLags) {    // x_t with t >= Mh - tau0 only meets zeros
#pragma unroll
    for (int u = 0; u < kLsLags; ++u) {
      const long long t = tb + u, t1 = t + tau0 + kLsLags;
      float x0[4];
      if (kFirst) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x0[r] = ring[r][u];
      } else {
        const f4 lik = lik_of_tile<NTM>(lds, preA, walk, lane, xa, yv, NT, b, nblk);
        tile_load_at<NTM>(W, first + (t + 1 < last ? t + 1 : last) * N, live, walk, lane, preA);
#pragma unroll
        for (int r = 0; r < 4; ++r) x0[r] = ls_centre(lik[r], m[r], t < Mh && chain_ok);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int l = 0; l < kLsLags; ++l) acc[r][l] = fmaf(x0[r], ring[r][(u + l) % kLsLags], acc[r][l]);
      const f4 lik = lik_of_tile<NTM>(lds, preB, walk, lane, xa, yv, NT, b, nblk);
      tile_load_at<NTM>(W, first + (t1 + 1 < last ? t1 + 1 : last) * N, live, walk, lane, preB);
#pragma unroll
      for (int r = 0; r < 4; ++r) ring[r][u] = ls_centre(lik[r], m[r], t1 < Mh && chain_ok);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int l = 0; l < kLsLags; ++l) { dacc[r][l] += (double)acc[r][l]; acc[r][l] = 0.f; }
  }
}

template <int NTM>
__global__ __launch_bounds__(kLsThreads) void lik_lagsum_kernel(const float* __restrict__ W, long long N, int d,
                                                                const float* __restrict__ P, int n, int NT, long long Mh,
                                                                long long row1, long long ncb, long long nbx, long long nlag,
                                                                const double* __restrict__ mean, double* __restrict__ part) {
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int nblk = (n + 15) >> 4;
  const long long u = (long long)blockIdx.x * 4 + w;
  if (u >= nbx * nblk) return;                               // (no workgroup barrier anywhere)
  float* lds = lds_all + w * REGION;
  tile_region_clear<NTM>(lds, lane);
  const int b = (int)(u % nblk), half = blockIdx.z;
  const long long xb = u / nblk, tau0 = (long long)blockIdx.y * kLsLags;

  f4 xa[1][NTM], yv[1];
  block_fragments<NTM, 1>(P, NT, b, nblk, lane, xa, yv);
  const TileWalk walk = tile_walk(lane, d, 0);
  double dacc[4][kLsLags];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int l = 0; l < kLsLags; ++l) dacc[r][l] = 0.0;

  for (long long cb = xb; cb < ncb; cb += nbx) {
    const long long c0 = cb * 16, first = (half ? row1 : 0) * N + c0;
    const int live = N - c0 < 16 ? (int)(N - c0) : 16;
    const bool chain_ok = c < live;
    double m[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * b + 4 * q + r;
      m[r] = (chain_ok && row < n) ? mean[((long long)half * N + c0 + c) * n + row] : 0.0;
    }
    if (tau0 == 0) lik_series<NTM, true>(W, N, first, live, chain_ok, Mh, tau0, m, lds, walk, lane, xa, yv[0], NT, b, nblk, dacc);
    else lik_series<NTM, false>(W, N, first, live, chain_ok, Mh, tau0, m, lds, walk, lane, xa, yv[0], NT, b, nblk, dacc);
  }

  // the 16 chain lanes of every (row, lag), added in the order c = 0 .. 15; rows at or past n and lags past max_lag are not written
  double* red = reinterpret_cast<double*>(lds);
#pragma unroll
  for (int l = 0; l < kLsLags; ++l) {
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 4; ++r) red[c * 16 + 4 * q + r] = dacc[r][l];
    wave_lds_fence();
    if (lane < 16) {
      double a = red[lane];
#pragma unroll
      for (int cc = 1; cc < 16; ++cc) a += red[cc * 16 + lane];
      const int row = 16 * b + lane;
      const long long lag = tau0 + l;
      if (row < n && lag < nlag) part[(((long long)half * nbx + xb) * n + row) * nlag + lag] = a;
    }
  }
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_logistic_lik_stats_workspace_bytes(int64_t steps, int64_t n_chains, int32_t d, int32_t n_data, int32_t max_lag,
                                                 int32_t split) {
  LikStatsPlan p;
  if (!lik_stats_plan("l2hmc_logistic_lik_stats_workspace_bytes", steps, n_chains, d, n_data, max_lag, split, p))
    return L2HMC_ERR_ARG;
  return p.halves * p.nbx * (int64_t)n_data * p.nlag * 8;
}

int l2hmc_logistic_lik_stats(const float* draws, int64_t steps, int64_t n_chains, int32_t d, const float* packed, int32_t n_data,
                             int32_t max_lag, int32_t split, double* mean, double* m2, double* G, void* workspace,
                             void* stream) {
  LikStatsPlan p;
  if (!lik_stats_plan("l2hmc_logistic_lik_stats", steps, n_chains, d, n_data, max_lag, split, p)) return L2HMC_ERR_ARG;
  if (!draws || !packed || !mean || !m2 || !G || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_logistic_lik_stats: draws, packed, mean, m2, G and workspace are required%s");
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)mean & 7) || ((uintptr_t)m2 & 7) || ((uintptr_t)G & 7) ||
      ((uintptr_t)workspace & 7))
    return fail(L2HMC_ERR_ARG, "l2hmc_logistic_lik_stats: draws must be 4-byte, packed 16-byte, mean, m2, G and workspace 8-byte "
                               "aligned%s");
  hipStream_t s = (hipStream_t)stream;
  const long long N = n_chains, units1 = p.ncb * p.nblk * p.halves, units2 = p.nbx * p.nblk;
  const dim3 block(kLsThreads), grid1((unsigned)((units1 + 3) / 4)),
      grid2((unsigned)((units2 + 3) / 4), (unsigned)p.ntile, (unsigned)p.halves);
  if (units1 > 4LL * 0x7fffffffLL) return fail(L2HMC_ERR_ARG, "l2hmc_logistic_lik_stats: history too large%s");
  on_feature_tiles(p.NTM, [&](auto ntm) {
    constexpr int NTM = decltype(ntm)::value;
    hipLaunchKernelGGL((lik_moments_kernel<NTM>), grid1, block, 0, s, draws, N, (int)d, packed, (int)n_data, p.NT, p.Mh, p.row1,
                       p.ncb, p.halves, mean, m2);
    hipLaunchKernelGGL((lik_lagsum_kernel<NTM>), grid2, block, 0, s, draws, N, (int)d, packed, (int)n_data, p.NT, p.Mh, p.row1,
                       p.ncb, p.nbx, p.nlag, (const double*)mean, (double*)workspace);
  });
  chunk_reduce_launch((const double*)workspace, p.halves * p.nbx, (long long)n_data * p.nlag, G, s);
  return launched();
}

}  // extern "C"
