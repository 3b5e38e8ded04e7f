// l2hmc_logistic_predict -- the per-row sums behind the posterior predictive, the lppd and WAIC of Bayesian logistic regression
// over every recorded draw, from a history that stays where the sampler wrote it.  For draws W (S, d) and the data packed by
// l2hmc_pack_logistic (rows x_i, labels y_i), with l = x_i . w_s, z = (2 y_i - 1) l:
//     p1 = sigmoid(l)    lik = sigmoid(z)    ll = log lik = min(z, 0) - log(1 + exp(-|l|))
//     sums (4, n) float64 = sum_s p1, sum_s lik, sum_s ll, sum_s ll^2
// l2hmc_amd/predictive.py turns the sums into numbers; include/l2hmc.h states the contract.  The (S, n) matrix of log-likelihoods
// is never written: the logit contraction (f32-input MFMA, the operand layouts of regression_grad in l2hmc_kernels.hpp) is fused
// with the reduction over draws.
//
// Work unit = one WAVE: a group of NB consecutive 16-row data blocks x a chunk of consecutive 16-draw tiles.  The wave keeps the
// XA fragments and labels of its data blocks in registers for the whole launch and streams the draw tiles past them; the tile
// loop -- load one tile ahead, stage into the wave's own LDS region, contract, and the end-of-wave reduction -- is the one of
// draw_tiles.hpp, and p1, lik and ll come from BernoulliLogit::sums (glm_family.hpp).  Here, per tile:
//   sum      each of p1, lik, ll is converted to float64 and added to the lane's own sum of (draw lane c, row 4 q + r); ll^2 is
//            formed and added in float64 (one fma).  A draw at or past S is EXCLUDED by a select on the lane (a zero draw would
//            add p1 = 0.5 and ll = -log 2).  No float32 partial sums anywhere.
// The main loop has no workgroup barrier and the four waves of a workgroup are independent units.
//   end      the 16 NB rows x 4 sums go to workspace[chunk][4][n]; rows at or past n are never written.
//   pass 2   chunk_reduce_kernel: sums[k][i] = the chunks' partials added in chunk order.  No floating-point atomics: two
//            calls give identical bits.
// Units are ordered (chunk, group) with the group fastest, so the waves of a workgroup read the same draws.  The plan is
// draw_plan's (draw_tiles.hpp), aiming for kDrawUnits waves: at S large / n small the chunks supply them, at n large / S small
// the data-block groups do.
//
// Occupancy by design: 2 waves per SIMD (8 per CU) -- the main kernel must stay within 256 registers (held by
// tests/test_predictive_cpu.py from the compiler's listing); its LDS (at most 4 x 8448 bytes per workgroup) never limits that.
// Geometries <NTM feature tiles compiled, NB data blocks per wave>: <1, 4>, <2, 4>, <4, 2>, <8, 2> -- 32 NB registers of
// float64 sums and 4 NTM NB of fragments per lane.
#include "draw_tiles.hpp"
#include "glm_family.hpp"

namespace l2hmc {

constexpr int kPredictThreads = 256;      // 4 independent waves

// data blocks per wave: 4 at NTM <= 2 feature tiles (d <= 32), else 2
constexpr int predict_nb(int d) { return d <= 32 ? 4 : 2; }

template <int NTM, int NB>
__global__ __launch_bounds__(kPredictThreads) void predict_kernel(const float* __restrict__ W, long long S, int d,
                                                                  const float* __restrict__ P, int n, int NT, int ngroups,
                                                                  long long nchunks, long long tpc,
                                                                  double* __restrict__ part) {
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
  // (the wave index through readfirstlane: the unit, its group and chunk and every test on them are then scalar)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const long long u = (long long)blockIdx.x * 4 + w;
  if (u >= (long long)ngroups * nchunks) return;             // (no workgroup barrier anywhere: a wave may leave alone)
  float* lds = lds_all + w * REGION;
  tile_region_clear<NTM>(lds, lane);

  const int group = (int)(u % ngroups);
  const long long chunk = u / ngroups;
  const int nblk = (n + 15) >> 4, b0 = group * NB;
  f4 xa[NB][NTM], yv[NB];
  block_fragments<NTM, NB>(P, NT, b0, nblk, lane, xa, yv);
  double acc[NB][4][4];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][k][r] = 0.0;

  const long long ntiles = (S + 15) >> 4;
  const long long t0 = chunk * tpc, t1 = t0 + tpc < ntiles ? t0 + tpc : ntiles;
  const TileWalk walk = tile_walk(lane, d, S);
  float pre[4 * NTM];
  tile_load<NTM>(W, t0, walk, lane, pre);

  for (long long t = t0; t < t1; ++t) {
    tile_stage<NTM>(lds, pre, walk, lane);
    wave_lds_fence();
    f4 Lg[NB];
    tile_logits<NTM, NB>(lds, xa, c, q, NT, b0, nblk, Lg);
    wave_lds_fence();
    if (t + 1 < t1) tile_load<NTM>(W, t + 1, walk, lane, pre);           // in flight during this tile's arithmetic
    const bool valid = 16 * t + c < S;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (b0 + j < nblk) {
        const f4 L = Lg[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p1, lik, ll;
          BernoulliLogit::sums(L[r], yv[j][r], p1, lik, ll);
          const double dll = (double)(valid ? ll : 0.f);
          acc[j][0][r] += (double)(valid ? p1 : 0.f);
          acc[j][1][r] += (double)(valid ? lik : 0.f);
          acc[j][2][r] += dll;
          acc[j][3][r] = fma(dll, dll, acc[j][3][r]);
        }
      }
    }
  }

  tile_sums_out<NB, 4>(lds, acc, lane, b0, nblk, n, chunk, part);
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_logistic_predict_workspace_doubles(int64_t n_draws, int32_t n_data, int32_t d) {
  DrawPlan p;
  if (!draw_plan("l2hmc_logistic_predict_workspace_doubles", n_draws, n_data, d, predict_nb(d), false, p)) return L2HMC_ERR_ARG;
  return p.nchunks * 4 * (int64_t)n_data;
}

int l2hmc_logistic_predict(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data, double* sums,
                           double* workspace, void* stream) {
  DrawPlan p;
  if (!draw_plan("l2hmc_logistic_predict", n_draws, n_data, d, predict_nb(d), false, p)) return L2HMC_ERR_ARG;
  if (!draws || !packed || !sums || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_logistic_predict: draws, packed, sums and workspace are required%s");
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7))
    return fail(L2HMC_ERR_ARG, "l2hmc_logistic_predict: draws must be 4-byte, packed 16-byte, sums and workspace 8-byte aligned%s");
  hipStream_t s = (hipStream_t)stream;
  const long long units = (long long)p.ngroups * p.nchunks;
  const dim3 grid((unsigned)((units + 3) / 4)), block(kPredictThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    constexpr int NTM = decltype(ntm)::value, NB = predict_nb(16 * NTM);
    hipLaunchKernelGGL((predict_kernel<NTM, NB>), grid, block, 0, s, draws, (long long)n_draws, (int)d, packed, (int)n_data, p.NT,
                       p.ngroups, p.nchunks, p.tpc, workspace);
  });
  chunk_reduce_launch(workspace, p.nchunks, 4LL * n_data, sums, s);
  return launched();
}

}  // extern "C"
