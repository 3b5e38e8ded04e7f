// l2hmc_logistic_loo_tails -- the per-row raw material of Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari,
// Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024) of Bayesian logistic regression over every recorded draw, from a
// history that stays where the sampler wrote it.  For draws W (S, d) and the data packed by l2hmc_pack_logistic, the log
// importance ratio of row i under draw s is lambda = softplus(-t) with t = (2 y_i - 1) x_i . w_s the SIGNED logit; lambda
// decreases in t, so the M largest ratios are the M smallest t.  Per row, with M = min(S / 5, ceil(3 sqrt S)):
//     cutoff   c = the element of rank M (0-based) of an ascending order of {t_s}   (the total order of the monotone key of
//              order_stats.hip: -0 before +0, every NaN last)
//     tail     the t strictly before c in that order, L <= M of them in any order; slots L .. M - 1 hold +inf
//     body     sum over the draws NOT in the tail of e^m + e^(m - t), m = min(c, 0): every term lies in (0, 2]
//     sum_lik  sum over all draws of sigmoid(t)
// l2hmc_amd/predictive.py `loo_finish` turns them into elpd_loo and the Pareto k-hat; include/l2hmc.h states the contract.  The
// (S, n) matrix is never written and nothing is sorted: a most-significant-digit radix select (radix_select.hpp), kRadixPasses =
// 4 passes of 8 bits, finds c per row, and one more pass gathers.  Every pass forms t again from W.
//
// THE INVARIANT THE SELECT AND THE GATHER RELY ON: every pass computes t by ONE device function, tile_logits of draw_tiles.hpp
// (staged by tile_stage), which adds the feature tiles tg = 0 .. NT - 1 in that order, four f32-input MFMAs each, onto a zero
// accumulator; the label's sign is applied afterwards (exact).  The bits of t_si therefore depend on (W, X, y) alone -- not on
// the pass, the chunk, the plan or the row grouping of the caller.  A key counted in one pass is the key compared in the next,
// and exactly the keys below the selected one reach the tail.
//
// The tile loop and the plan are draw_tiles.hpp's (a draw at or past S, a row at or past n never counts), the signed logit and
// the likelihood BernoulliLogit's (glm_family.hpp).  Work unit = one wave: NB = 2 consecutive 16-row data blocks x a chunk of
// tpc 16-draw tiles, planned by draw_plan(by_draws): tpc depends on S ALONE, so the order in which float64 terms are added does
// not depend on how many rows a call holds.  A workgroup is four waves on the SAME data blocks and four consecutive chunks;
// blockIdx.x = quad * ngroups + group.
//
//   count    loo_kernel<NTM, 0>: the count pass of radix_select.hpp over one LDS histogram [32 rows][256 bins] (32 KiB).
//   advance  radix_advance_kernel; radix_select_passes drives the four passes, and after the last the cutoff is written.
//   gather   loo_kernel<NTM, 1>: a key below the cutoff's key takes slot atomicAdd(n_tail[row], 1) (an integer atomic) of the
//            row's tail; a slot at or past M is not written and raises the error word of the workspace (it cannot happen while
//            the invariant holds).  Every other live draw adds its body term, every live draw its sigmoid, converted to float64
//            BEFORE the addition, to the lane's own sums; once per wave the 16 draw lanes are added in the order c = 0 .. 15 and
//            the wave's partials go to workspace[chunk][2][n].
//   reduce   chunk_reduce_kernel: sums[k][i] = the chunks' partials added in chunk order.
//   mc       l2hmc_logistic_loo_tails_mc (a run of autocorrelated draws: `predictive.loo(r_eff=...)`): every row has its OWN tail
//            length tail_len_row[i] <= tail_stride -- `remaining` starts there, the tail's row stride is tail_stride -- and the
//            gather is loo_kernel<NTM, 2>: MODE 1 with a third sum, body_sq = the sum over the draws not in the tail of
//            (e^m + e^(m - t))^2, each float32 term squared exactly in float64 (in (0, 4]).  The first two sums are MODE 1's
//            operations in MODE 1's order: with every length equal to M the old entry's bits come back.
// No floating-point atomics anywhere: integer counts do not depend on arrival order, the tail is a set, the sums have a fixed
// tree.  Every outward write is an ordinary vector store or atomic from plain C++.
//
// Counts: a bin of the LDS histogram is a uint32 and a workgroup adds at most 4 waves x tpc x 16 draws to one bin of a row.
// tpc <= 2^40 / 16 / 1024 = 2^26 at the largest n_draws the entry accepts, i.e. at most 2^32 -- one more than a bin holds, and
// only if every draw of a 2^40-draw, d = 1 history (4 TB) fell into one bin; any history that fits a device stays far below.
//
// Occupancy by design: 2 workgroups per CU (2 waves per SIMD) -- every geometry must stay within 256 registers (held by
// tests/test_loo_cpu.py from the compiler's listing) and its LDS, 32 KiB of histogram plus at most 33 KiB of staging, within
// 80 KiB: two resident workgroups use at most 130 KiB of the 160 KiB of a CU.  Geometries <NTM feature tiles compiled>: 1, 2, 4, 8.
// MODE 2 states the two waves per SIMD in its launch bounds (its third sum needs it at NTM = 8); MODE 0 and 1 compile as before.
// Both entries share loo_run, and the kernels of the old entry take a NULL len_row: its outputs are bit for bit what they were.
#include <math.h>

#include "draw_tiles.hpp"
#include "glm_family.hpp"
#include "radix_select.hpp"

namespace l2hmc {

constexpr int kLooThreads = 256;          // 4 waves on the same rows
constexpr int kLooNB = 2;                 // 16-row data blocks per wave
constexpr int kLooRows = 16 * kLooNB;     // rows of a workgroup's histogram

struct LooPlan : DrawPlan {
  long long M;                            // the tail's length (its row stride in the mc entry)
};

// M = min(floor(S / 5), ceil(3 sqrt S)) in integers
static long long loo_tail_len(long long S) {
  if (S < 1) return 0;
  long long k = (long long)ceil(3.0 * sqrt((double)S));
  while (k > 0 && (k - 1) * (k - 1) >= 9 * S) --k;
  while (k * k < 9 * S) ++k;
  const long long f = S / 5;
  return f < k ? f : k;
}

static bool loo_plan(const char* who, int64_t n_draws, int32_t n_data, int32_t d, LooPlan& p) {
  if (!draw_plan(who, n_draws, n_data, d, kLooNB, true, p)) return false;
  p.M = loo_tail_len(n_draws);
  if (p.M * n_data > (1LL << 31)) { fail(L2HMC_ERR_ARG, "%s: tail too large (tail_len n_data > 2^31): fewer rows per call", who); return false; }
  return true;
}

// workspace: error word (8 B) | hist (n, 256) int64 | remaining (n) int64 | prefix (n) uint32, padded to 8 B | partials
struct LooWorkspace {
  unsigned long long* err;
  unsigned long long* hist;
  long long* remaining;
  uint32_t* prefix;
  double* part;
  int64_t bytes;
};

static LooWorkspace loo_workspace(void* base, const LooPlan& p, int32_t n, int nsums = 2) {
  LooWorkspace w;
  Carve c{(char*)base};
  w.err = c.take<unsigned long long>(1);
  w.hist = c.take<unsigned long long>((int64_t)n * kRadixBins);
  w.remaining = c.take<long long>(n);
  w.prefix = c.take<uint32_t>(n);
  c.pad(8);
  w.part = c.take<double>(p.nchunks * nsums * (int64_t)n);
  w.bytes = c.off;
  return w;
}

// MODE 0: count the digit at `shift` of the keys on their row's prefix (first: no prefix, every key).  MODE 1: gather.
// MODE 2: gather with a tail length per row (len_row; M is the tail's row stride) and the third sum body_sq.
template <int NTM, int MODE>
// (MODE 2 alone asks for the two waves per SIMD of the header explicitly: its third sum took <8, 2> to 268 registers without;
// MODE 0 and 1 keep the bounds, and with them the register allocation, they had before MODE 2 existed)
__global__ __launch_bounds__(kLooThreads, MODE == 2 ? 2 : 1) void loo_kernel(const float* __restrict__ W, long long S, int d,
                                                          const float* __restrict__ P, int n, int NT, int ngroups,
                                                          long long nchunks, long long tpc, const uint32_t* __restrict__ prefix,
                                                          int shift, int first, unsigned long long* __restrict__ hist,
                                                          unsigned long long* __restrict__ n_tail, float* __restrict__ tail,
                                                          long long M, unsigned long long* __restrict__ err,
                                                          double* __restrict__ part,
                                                          const long long* __restrict__ len_row) {
  constexpr int K = MODE == 2 ? 3 : 2;
  constexpr int NB = kLooNB;
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
  __shared__ uint32_t hl[MODE == 0 ? kLooRows * kRadixBins : 1];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int group = (int)(blockIdx.x % (unsigned)ngroups);
  const long long chunk = (long long)(blockIdx.x / (unsigned)ngroups) * 4 + w;
  const bool live_wave = chunk < nchunks;                    // (wave-uniform; a dead wave still meets the barriers below)
  float* lds = lds_all + w * REGION;
  tile_region_clear<NTM>(lds, lane);
  if (MODE == 0) {
    radix_hist_clear<kLooRows, kLooThreads>(hl);
    __syncthreads();
  }

  const int nblk = (n + 15) >> 4, b0 = group * NB;
  if (live_wave) {
    f4 xa[NB][NTM], yv[NB];
    block_fragments<NTM, NB>(P, NT, b0, nblk, lane, xa, yv);
    uint32_t pre_key[NB][4];          // count: the row's prefix above the digit; gather: the cutoff's key
    float em[NB][4], mm[NB][4];       // gather: e^m and m = min(cutoff, 0)
    bool row_ok[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * (b0 + j) + 4 * q + r;
        row_ok[j][r] = b0 + j < nblk && row < n;
        const uint32_t key = (row_ok[j][r] && !(MODE == 0 && first)) ? prefix[row] : 0u;
        if (MODE == 0) {
          pre_key[j][r] = first ? 0u : key >> (shift + kRadixBits);
          em[j][r] = mm[j][r] = 0.f;
        } else {
          pre_key[j][r] = key;
          mm[j][r] = fminf(radix_unkey(key), 0.f);             // (a NaN cutoff gives 0)
          em[j][r] = (float)exp((double)mm[j][r]);
        }
      }
    }
    double acc[NB][K][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k)
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
      f4 T[NB];
      tile_logits<NTM, NB>(lds, xa, c, q, NT, b0, nblk, T);
      wave_lds_fence();
      if (t + 1 < t1) tile_load<NTM>(W, t + 1, walk, lane, pre);         // in flight during this tile's arithmetic
      const bool valid = 16 * t + c < S;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (b0 + j < nblk) {                                 // wave-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float tv = BernoulliLogit::signed_logit(T[j][r], yv[j][r]);
            const uint32_t key = radix_key(tv);
            const bool ok = valid && row_ok[j][r];
            if (MODE == 0) {
              uint32_t* hrow = hl + (16 * j + 4 * q + r) * kRadixBins;
              if (first) radix_count_first(hrow, key, ok, lane, c);
              else radix_count_next(hrow, key, ok, shift, pre_key[j][r]);
            } else {
              const bool in_tail = ok && key < pre_key[j][r];
              if (in_tail) {
                const int row = 16 * (b0 + j) + 4 * q + r;
                const unsigned long long slot = atomicAdd(&n_tail[row], 1ull);
                const long long room_ = MODE == 2 ? (len_row[row] < M ? len_row[row] : M) : M;       // (never past the row's stride)
                const unsigned long long room = (unsigned long long)(room_ < 0 ? 0 : room_);
                if (slot < room) tail[(long long)row * M + (long long)slot] = tv;
                else atomicOr(err, 1ull);
              }
              const float lik = BernoulliLogit::lik(tv);
              const float body = em[j][r] + fexp(mm[j][r] - tv);
              acc[j][0][r] += (double)((ok && !in_tail) ? body : 0.f);
              acc[j][1][r] += (double)(ok ? lik : 0.f);
              if (MODE == 2) { const double b = (double)((ok && !in_tail) ? body : 0.f); acc[j][2][r] += b * b; }
            }
          }
        }
      }
    }

    if (MODE != 0) tile_sums_out<NB, K>(lds, acc, lane, b0, nblk, n, chunk, part);
  }

  if (MODE == 0) radix_hist_flush<kLooRows, kLooThreads>(hl, b0, n, hist);
}

__global__ void loo_init_kernel(long long* __restrict__ remaining, uint32_t* __restrict__ prefix,
                                unsigned long long* __restrict__ n_tail, float* __restrict__ tail, int n, long long M,
                                unsigned long long* __restrict__ err, const long long* __restrict__ len_row) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *err = 0ull;
  if (i < n) {
    long long rank = len_row ? len_row[i] : M;               // (a length outside 0 .. M is clamped: the tail has M slots)
    rank = rank < 0 ? 0 : rank > M ? M : rank;
    remaining[i] = rank; prefix[i] = 0u; n_tail[i] = 0ull;
  }
  if (i < (long long)n * M) tail[i] = __builtin_inff();
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_logistic_loo_tail_len(int64_t n_draws) { return loo_tail_len(n_draws); }

int64_t l2hmc_logistic_loo_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d) {
  LooPlan p;
  if (!loo_plan("l2hmc_logistic_loo_workspace_bytes", n_draws, n_data, d, p)) return L2HMC_ERR_ARG;
  return loo_workspace(nullptr, p, n_data).bytes;
}

// the passes of both entries: len_row = nullptr is l2hmc_logistic_loo_tails (one length p.M, two sums)
static int loo_run(const char* who, const LooPlan& p, const float* draws, int64_t n_draws, int32_t d, const float* packed,
                   int32_t n_data, const int64_t* len_row, float* cutoff, int64_t* n_tail, float* tail, double* sums,
                   void* workspace, void* stream) {
  if (!draws || !packed || !cutoff || !n_tail || (!tail && p.M > 0) || !sums || !workspace)
    return fail(L2HMC_ERR_ARG, "%s: draws, packed, cutoff, n_tail, tail, sums and workspace are required", who);
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)cutoff & 3) || ((uintptr_t)n_tail & 7) ||
      ((uintptr_t)tail & 3) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)len_row & 7))
    return fail(L2HMC_ERR_ARG, "%s: draws, cutoff and tail must be 4-byte, packed 16-byte, n_tail, tail_len_row, sums and "
                               "workspace 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int nsums = len_row ? 3 : 2;
  const LooWorkspace ws = loo_workspace(workspace, p, n_data, nsums);
  const long long* lens = (const long long*)len_row;
  const long long n = n_data, cells = n * p.M > n ? n * p.M : n;
  hipLaunchKernelGGL(loo_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, ws.remaining, ws.prefix,
                     (unsigned long long*)n_tail, tail, (int)n_data, p.M, ws.err, lens);
  const dim3 grid((unsigned)(p.quads * p.ngroups)), block(kLooThreads);
  auto pass = [&](auto mode, int shift, bool first) {
    on_feature_tiles(p.NTM, [&](auto ntm) {
      hipLaunchKernelGGL((loo_kernel<decltype(ntm)::value, decltype(mode)::value>), grid, block, 0, s, draws, (long long)n_draws,
                         (int)d, packed, (int)n_data, p.NT, p.ngroups, p.nchunks, p.tpc, (const uint32_t*)ws.prefix, shift,
                         (int)first, ws.hist, (unsigned long long*)n_tail, tail, p.M, ws.err, ws.part, lens);
    });
  };
  const int rc = radix_select_passes(ws.hist, ws.remaining, ws.prefix, (int)n_data, cutoff, s,
                                     [&](int shift, bool first) { pass(ic<0>{}, shift, first); });
  if (rc) return rc;
  if (len_row) pass(ic<2>{}, 0, false);
  else pass(ic<1>{}, 0, false);
  chunk_reduce_launch(ws.part, p.nchunks, (long long)nsums * n_data, sums, s);
  return launched();
}

// the plan of the mc entry: loo_plan with the caller's tail stride in the place of M
static bool loo_plan_mc(const char* who, int64_t n_draws, int32_t n_data, int32_t d, int64_t tail_stride, LooPlan& p) {
  if (!loo_plan(who, n_draws, n_data, d, p)) return false;
  if (tail_stride < 0 || tail_stride >= n_draws) {
    fail(L2HMC_ERR_ARG, "%s: 0 <= tail_stride < n_draws (got %lld)", who, tail_stride);
    return false;
  }
  p.M = tail_stride;
  if (p.M * n_data > (1LL << 31)) { fail(L2HMC_ERR_ARG, "%s: tail too large (tail_stride n_data > 2^31): fewer rows per call", who); return false; }
  return true;
}

int l2hmc_logistic_loo_tails(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data, float* cutoff,
                             int64_t* n_tail, float* tail, double* sums, void* workspace, void* stream) {
  LooPlan p;
  if (!loo_plan("l2hmc_logistic_loo_tails", n_draws, n_data, d, p)) return L2HMC_ERR_ARG;
  return loo_run("l2hmc_logistic_loo_tails", p, draws, n_draws, d, packed, n_data, nullptr, cutoff, n_tail, tail, sums, workspace,
                 stream);
}

int64_t l2hmc_logistic_loo_mc_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d) {
  LooPlan p;
  if (!loo_plan("l2hmc_logistic_loo_mc_workspace_bytes", n_draws, n_data, d, p)) return L2HMC_ERR_ARG;
  return loo_workspace(nullptr, p, n_data, 3).bytes;
}

int l2hmc_logistic_loo_tails_mc(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data,
                                const int64_t* tail_len_row, int64_t tail_stride, float* cutoff, int64_t* n_tail, float* tail,
                                double* sums, void* workspace, void* stream) {
  LooPlan p;
  if (!loo_plan_mc("l2hmc_logistic_loo_tails_mc", n_draws, n_data, d, tail_stride, p)) return L2HMC_ERR_ARG;
  if (!tail_len_row) return fail(L2HMC_ERR_ARG, "l2hmc_logistic_loo_tails_mc: tail_len_row is required%s");
  return loo_run("l2hmc_logistic_loo_tails_mc", p, draws, n_draws, d, packed, n_data, tail_len_row, cutoff, n_tail, tail, sums,
                 workspace, stream);
}

}  // extern "C"
