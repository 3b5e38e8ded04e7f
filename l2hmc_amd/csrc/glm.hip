// l2hmc_glm_log_lik, l2hmc_glm_loo_tails, l2hmc_glm_predict -- model criticism of a generalised linear model (Poisson regression
// with the log link; glm_family.hpp) over every recorded draw, from a history that stays where the sampler wrote it: the
// pointwise log-likelihood matrix when it is wanted, the per-row raw material of PSIS-LOO (Vehtari, Gelman, Gabry 2017; Vehtari,
// Simpson, Gelman, Yao, Gabry 2024) and the sums behind the posterior predictive mean and WAIC without it.  For draws W (S, d),
// the data packed by l2hmc_pack_logistic (rows x_i, the responses y_i in the label slot) and the row constants (3, n) float32
// (glm_family.hpp: offset o_i, g_i = lgamma(y_i + 1), the saturated log-likelihood sat_i = sup over eta of ll), the
// log-likelihood of row i under draw s is ll = Family::ll(x_i . w_s, y_i, o_i, g_i).  l2hmc_amd/glm.py turns the outputs into
// numbers; include/l2hmc.h states the contracts.
//
// THE INVARIANT: every kernel below computes ll by ONE device function, Family::ll of glm_family.hpp, from the eta of
// tile_logits (draw_tiles.hpp) and nothing else; its bits depend on (W, X, y, row constants) alone -- not on the pass, the
// chunk, the kernel or the row grouping of the caller (the header of glm_family.hpp says why no contraction can differ).
//
//   matrix   glm_loglik_kernel: ll of a (16 draws) x (16 NB rows) tile goes to out (S, n) float32 with ordinary vector stores;
//            a draw at or past S and a row at or past n are never written.  The slow route, and the tests' hinge: it yields
//            the very values the fused kernels select among.
//   tails    a radix select and a gather on the keys radix_key(ll): the log importance ratio is -ll, so the largest ratios are
//            the smallest ll.  A workgroup is four waves on the SAME two data blocks and four consecutive chunks; tpc, the
//            16-draw tiles of a count chunk, comes from draw_plan(by_draws) of draw_tiles.hpp -- the function l2hmc_logistic_loo_tails
//            plans with -- and the draws of a gather segment from glm_plan below: both functions of n_draws ALONE.
//     count    glm_loo_kernel<F, NTM, 0>: the count pass of radix_select.hpp over one LDS histogram [32 rows][256 bins] per
//              workgroup.  Pass 0 ALSO takes the row's largest key: a running maximum per lane, the 16 draw lanes reduced by
//              shuffles, one integer atomicMax per row and wave -- the row's `top`, a NaN when the row holds one (its key is
//              the last).
//     advance  radix_advance_kernel, driven by radix_select_passes; after the last pass the prefix is the cutoff's key.
//     gather   glm_loo_kernel<F, NTM, 1>: a key strictly below the cutoff's takes slot atomicAdd(n_tail[row], 1) of the row's
//              tail; a slot at or past the row's length is not written and raises the error word (it cannot happen while the
//              invariant holds).  Every term is formed as loglik_tails.hip forms it -- in float64 from the exact float32
//              values: (double) c - (double) ll, then the double-precision exp, one call per term -- body = e^(c - ll) and
//              body_sq = e^(2 (c - ll)) over the draws not in the tail, lik = e^(ll - top) over all: that file's per-term bound
//              holds, and so does its table of non-finite cutoffs (the same comparisons and the same expressions).
//              THE ORDER OF THE SUMS IS THAT FILE'S TOO: a wave takes one of its segments of max(64, ceil(n_draws / 2048))
//              consecutive draws (cut out of the history at any draw: tile_load_at), and per data block of a tile the terms go
//              through 6 KiB of LDS to 48 lanes, one per (sum, row), which add the tile's 16 draws onto their running sum one
//              after the other, in draw order.  A row's three sums are therefore the sums l2hmc_loglik_tails returns for the
//              written matrix BIT FOR BIT, and every number finished from them equals the materialised route's.  (Lane-wise
//              sums over the 16 draw lanes, the first form of this kernel, differed from them in the last bits only -- which
//              the three-term body variance of the finish amplifies to 2e-11 of mcse_elpd_loo_i when a row's draws lie close
//              together.)  The partials go to workspace[segment][3][n].
//     reduce   chunk_reduce_kernel: sums[k][i] = the segments' partials added in segment order.
//   predict  glm_predict_kernel, planned like the matrix (draw_plan, filling kDrawUnits waves): sums (4, n) float64 = sum mu,
//            sum exp((double) ll - sat_i) (one double exp per term; in (0, 1] up to the rounding of sat), sum ll, sum ll^2
//            (formed and added in float64, one fma).  A draw at or past S and a row at or past n never count; partials are
//            added in chunk order.
// No floating-point atomics anywhere: integer counts and maxima do not depend on arrival order, the tail is a set, the sums have
// a fixed tree.  Every outward write is an ordinary vector store or an integer atomic from plain C++.  A row's bits do not
// depend on the other rows of the call.
//
// Occupancy by design: 2 waves per SIMD (two workgroups of four waves per CU) for every kernel and every geometry <NTM feature
// tiles compiled> = 1, 2, 4, 8, stated in the launch bounds: at most 256 registers and NO scratch (tests/test_glm_cpu.py holds
// both from the compiler's listing).  The count kernel's LDS is 32 KiB of histogram plus at most 33 KiB of staging, the
// gather's 24 KiB of terms plus the staging: two resident workgroups use at most 130 KiB of the 160 KiB of a CU.
// Measured (profiles/glm_bench.txt, 1000 x 4096 draws of d = 25 against 1000 rows): a count pass 6.0 to 8.9 ms, as
// l2hmc_logistic_loo_tails' (6.0 to 8.1); the gather 21.8 ms against 7.7 -- three double exp per element, as in
// loglik_tails.hip -- of which the draw-order sums cost 3.9 (the lane-wise form took 17.9).
#include <math.h>

#include "draw_tiles.hpp"
#include "glm_family.hpp"
#include "radix_select.hpp"

namespace l2hmc {

constexpr int kGlmThreads = 256;          // 4 waves
constexpr int kGlmNB = 2;                 // 16-row data blocks per wave
constexpr int kGlmRows = 16 * kGlmNB;     // rows of a workgroup's histogram
constexpr int kGlmTerms = 16 * 16 * 3;    // gather: the float64 terms of one data block of one tile

struct GlmPlan : DrawPlan {
  long long seg_rows, nseg, seg_quads;    // the gather's segments of consecutive draws (a function of n_draws alone)
};

static bool glm_family_ok(const char* who, int32_t family) {
  if (family != PoissonLog::kAbi) { fail(L2HMC_ERR_ARG, "%s: unknown family %lld (L2HMC_GLM_POISSON = 1)", who, family); return false; }
  return true;
}

// draw_plan (by_draws: the tails; else the matrix and the predictive sums) and the gather's segments
static bool glm_plan(const char* who, int32_t family, int64_t n_draws, int32_t n_data, int32_t d, bool by_draws, GlmPlan& p) {
  if (!glm_family_ok(who, family)) return false;
  if (!draw_plan(who, n_draws, n_data, d, kGlmNB, by_draws, p)) return false;
  draw_segments(n_draws, p.seg_rows, p.nseg);                // (loglik_tails.hip's: the two routes add in one order)
  p.seg_quads = (p.nseg + 3) / 4;
  return true;
}

// the constants of the rows a lane meets: rc[k][j][r] = row_consts[k][16 (b0 + j) + 4 q + r], 0 for a dead row
template <int NB, int KC>
__device__ __forceinline__ void row_constants(const float* __restrict__ RC, int n, int b0, int nblk, int q, float (&rc)[KC][NB][4],
                                              bool (&row_ok)[NB][4]) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (b0 + j) + 4 * q + r;
      row_ok[j][r] = b0 + j < nblk && row < n;
#pragma unroll
      for (int k = 0; k < KC; ++k) rc[k][j][r] = row_ok[j][r] ? RC[(long long)k * n + row] : 0.f;
    }
  }
}

// ---- the matrix ---------------------------------------------------------------------------------------------------------------
template <typename F, int NTM>
__global__ __launch_bounds__(kGlmThreads, 2) void glm_loglik_kernel(const float* __restrict__ W, long long S, int d,
                                                                    const float* __restrict__ P, const float* __restrict__ RC,
                                                                    int n, int NT, int ngroups, long long nchunks, long long tpc,
                                                                    float* __restrict__ out) {
  constexpr int NB = kGlmNB;
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
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
  float rc[2][NB][4];
  bool row_ok[NB][4];
  row_constants<NB, 2>(RC, n, b0, nblk, q, rc, row_ok);

  const long long ntiles = (S + 15) >> 4;
  const long long t0 = chunk * tpc, t1 = t0 + tpc < ntiles ? t0 + tpc : ntiles;
  const TileWalk walk = tile_walk(lane, d, S);
  float pre[4 * NTM];
  tile_load<NTM>(W, t0, walk, lane, pre);
  for (long long t = t0; t < t1; ++t) {
    tile_stage<NTM>(lds, pre, walk, lane);
    wave_lds_fence();
    f4 E[NB];
    tile_logits<NTM, NB>(lds, xa, c, q, NT, b0, nblk, E);
    wave_lds_fence();
    if (t + 1 < t1) tile_load<NTM>(W, t + 1, walk, lane, pre);
    const long long draw = 16 * t + c;
    const bool valid = draw < S;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (b0 + j < nblk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ll = F::ll(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r]);
          if (valid && row_ok[j][r]) out[draw * n + (16 * (b0 + j) + 4 * q + r)] = ll;
        }
      }
    }
  }
}

// ---- the tails ----------------------------------------------------------------------------------------------------------------
// workspace: error word (8 B) | hist (n, 256) int64 | remaining (n) int64 | ranks (n) int64 | prefix (n) uint32 | topkey (n)
//            uint32, the two padded to 8 B together | partials (segments, 3, n) float64
struct GlmWorkspace {
  unsigned long long* err;
  unsigned long long* hist;
  long long* remaining;
  long long* ranks;
  uint32_t* prefix;
  uint32_t* topkey;
  double* part;
  int64_t bytes;
};

static GlmWorkspace glm_workspace(void* base, const GlmPlan& p, int32_t n) {
  GlmWorkspace w;
  Carve c{(char*)base};
  w.err = c.take<unsigned long long>(1);
  w.hist = c.take<unsigned long long>((int64_t)n * kRadixBins);
  w.remaining = c.take<long long>(n);
  w.ranks = c.take<long long>(n);
  w.prefix = c.take<uint32_t>(n);
  w.topkey = c.take<uint32_t>(n);
  w.part = c.take<double>(p.nseg * 3 * (int64_t)n);
  w.bytes = c.off;
  return w;
}

__global__ void glm_loo_init_kernel(long long* __restrict__ remaining, long long* __restrict__ ranks, uint32_t* __restrict__ prefix,
                                    uint32_t* __restrict__ topkey, unsigned long long* __restrict__ n_tail,
                                    float* __restrict__ tail, int n, long long stride, long long M,
                                    const long long* __restrict__ len_row, unsigned long long* __restrict__ err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *err = 0ull;
  if (i < n) {
    long long rank = len_row ? len_row[i] : M;               // (a length outside 0 .. tail_stride is clamped: the tail has that many slots)
    rank = rank < 0 ? 0 : rank > stride ? stride : rank;
    remaining[i] = rank; ranks[i] = rank; prefix[i] = 0u; topkey[i] = 0u; n_tail[i] = 0ull;
  }
  if (i < (long long)n * stride) tail[i] = __builtin_inff();
}

// MODE 0: count the digit at `shift` of the keys on their row's prefix (first: no prefix, every key, and the row's largest key).
// MODE 1: gather.
template <typename F, int NTM, int MODE>
__global__ __launch_bounds__(kGlmThreads, 2) void glm_loo_kernel(const float* __restrict__ W, long long S, int d,
                                                                 const float* __restrict__ P, const float* __restrict__ RC, int n,
                                                                 int NT, int ngroups, long long nchunks, long long tpc,
                                                                 const uint32_t* __restrict__ prefix, int shift, int first,
                                                                 unsigned long long* __restrict__ hist,
                                                                 uint32_t* __restrict__ topkey, const long long* __restrict__ ranks,
                                                                 float* __restrict__ top, unsigned long long* __restrict__ n_tail,
                                                                 float* __restrict__ tail, long long stride,
                                                                 unsigned long long* __restrict__ err, double* __restrict__ part) {
  constexpr int NB = kGlmNB;
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
  __shared__ uint32_t hl[MODE == 0 ? kGlmRows * kRadixBins : 1];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int group = (int)(blockIdx.x % (unsigned)ngroups);
  const long long chunk = (long long)(blockIdx.x / (unsigned)ngroups) * 4 + w;
  const bool live_wave = chunk < nchunks;                    // (wave-uniform; a dead wave still meets the barriers below)
  float* lds = lds_all + w * REGION;
  tile_region_clear<NTM>(lds, lane);
  const int nblk = (n + 15) >> 4, b0 = group * NB;
  // gather: the four numbers of every row of the workgroup -- offset, g, the cutoff's key, the row's maximum -- wait in LDS and
  // are read per tile: held in registers across the float64 exponentials (whose constants the compiler keeps in registers
  // too) they pushed the widest geometry into scratch
  __shared__ __attribute__((aligned(16))) float rowc[MODE == 1 ? 4 * kGlmRows : 4];
  // gather: the terms of one data block of one tile, [16 draws][16 rows][3 sums] float64 per wave, added serially in draw order
  __shared__ double red_all[MODE == 1 ? 4 * kGlmTerms : 1];
  if (MODE == 0) {
    radix_hist_clear<kGlmRows, kGlmThreads>(hl);
  } else if (threadIdx.x < kGlmRows) {
    const int i = threadIdx.x, row = 16 * b0 + i;
    const bool live = row < n;
    const float tv = live ? radix_unkey(topkey[row]) : 0.f;
    rowc[i] = live ? RC[row] : 0.f;
    rowc[kGlmRows + i] = live ? RC[(long long)n + row] : 0.f;
    rowc[2 * kGlmRows + i] = __uint_as_float(live ? prefix[row] : 0u);
    rowc[3 * kGlmRows + i] = tv;
    if (live && blockIdx.x < (unsigned)ngroups) top[row] = tv;          // (the first quad of chunks writes the row's maximum out)
  }
  __syncthreads();

  if (live_wave) {
    f4 xa[NB][NTM], yv[NB];
    block_fragments<NTM, NB>(P, NT, b0, nblk, lane, xa, yv);
    float rc[2][NB][4];               // count: the row's offset and g
    bool row_ok[NB][4];
    uint32_t pre_key[NB][4];          // count: the row's prefix above the digit (pass 0: the running largest key)
    if (MODE == 0) row_constants<NB, 2>(RC, n, b0, nblk, q, rc, row_ok);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * (b0 + j) + 4 * q + r;
        if (MODE == 0) {
          const uint32_t key = (row_ok[j][r] && !first) ? prefix[row] : 0u;
          pre_key[j][r] = first ? 0u : key >> (shift + kRadixBits);
        } else {
          row_ok[j][r] = b0 + j < nblk && row < n;
          rc[0][j][r] = rc[1][j][r] = 0.f;
          pre_key[j][r] = 0u;
        }
      }
    }
    // gather: lane L < 48 owns the sum k = L / 16 of row L % 16 of either data block, added in DRAW ORDER over the segment
    double sacc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) sacc[j] = 0.0;
    double* red = red_all + (MODE == 1 ? w * kGlmTerms : 0);

    // count: the chunk is tpc 16-draw tiles.  gather: the chunk is ONE SEGMENT of `tpc` consecutive draws [r0, r1), the
    // segments of loglik_gather_kernel (loglik_tails.hip) -- not a multiple of 16 when n_draws > 131072, so its tiles are cut
    // out at any draw (tile_load_at; the logits of a draw do not depend on its place in a tile) and the last one is ragged
    const long long ntiles = (S + 15) >> 4;
    const long long r0 = chunk * tpc, r1 = r0 + tpc < S ? r0 + tpc : S;
    const long long t0 = MODE == 1 ? 0 : chunk * tpc;
    const long long t1 = MODE == 1 ? (r1 - r0 + 15) >> 4 : (t0 + tpc < ntiles ? t0 + tpc : ntiles);
    const TileWalk walk = tile_walk(lane, d, S);
    float pre[4 * NTM];
    auto load = [&](long long t) {
      if (MODE == 1) {
        const long long draw0 = r0 + 16 * t;
        tile_load_at<NTM>(W, draw0, (int)(r1 - draw0 < 16 ? r1 - draw0 : 16), walk, lane, pre);
      } else {
        tile_load<NTM>(W, t, walk, lane, pre);
      }
    };
    load(t0);

    constexpr bool kLate = MODE == 1 && NTM >= 4;
    for (long long t = t0; t < t1; ++t) {
      tile_stage<NTM>(lds, pre, walk, lane);
      wave_lds_fence();
      f4 E[NB];
      if (kLate) {
        // ... and the X fragments (4 NTM NB registers) are read again for every tile, L2-hot, instead of being held across
        // the exponentials; the pointer is made opaque so that the loads are not hoisted back out of the loop
        const float* Pt = P;
        asm volatile("" : "+s"(Pt));
        block_fragments<NTM, NB>(Pt, NT, b0, nblk, lane, xa, yv);
      }
      tile_logits<NTM, NB>(lds, xa, c, q, NT, b0, nblk, E);
      wave_lds_fence();
      // the next tile's loads are in flight during this tile's arithmetic -- except where their 4 NTM registers would push
      // the gather's float64 arithmetic into scratch (kLate): there they are issued after it and only the other resident
      // wave's arithmetic can cover their latency (not measured apart; the whole NTM = 8 gather takes 9.8 ms where the
      // logistic one, three float32 transcendentals per element, takes 6.9: profiles/glm_bench.txt)
      if (!kLate && t + 1 < t1) load(t + 1);
      const bool valid = MODE == 1 ? r0 + 16 * t + c < r1 : 16 * t + c < S;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (b0 + j < nblk) {                                 // wave-uniform
          f4 o4 = splat(0.f), g4 = o4, ck4 = o4, tp4 = o4;
          if (MODE == 1) {
            const float* rp = rowc + 16 * j + 4 * q;         // (opaque: the reads stay inside the loop)
            asm volatile("" : "+v"(rp));
            o4 = lds4(rp); g4 = lds4(rp + kGlmRows); ck4 = lds4(rp + 2 * kGlmRows); tp4 = lds4(rp + 3 * kGlmRows);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = MODE == 1 ? F::ll(E[j][r], yv[j][r], o4[r], g4[r]) : F::ll(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r]);
            const uint32_t key = radix_key(v);
            const bool ok = valid && row_ok[j][r];
            if (MODE == 0) {
              uint32_t* hrow = hl + (16 * j + 4 * q + r) * kRadixBins;
              if (first) {
                radix_count_first(hrow, key, ok, lane, c);
                const uint32_t mine = ok ? key : 0u;         // ... and the running largest key of the row
                pre_key[j][r] = mine > pre_key[j][r] ? mine : pre_key[j][r];
              } else {
                radix_count_next(hrow, key, ok, shift, pre_key[j][r]);
              }
            } else {
              const uint32_t ckey = __float_as_uint(ck4[r]);
              const bool in_tail = ok && key < ckey;
              if (in_tail) {
                const int row = 16 * (b0 + j) + 4 * q + r;
                const unsigned long long slot = atomicAdd(&n_tail[row], 1ull);
                if (slot < (unsigned long long)ranks[row]) tail[(long long)row * stride + (long long)slot] = v;
                else atomicOr(err, 1ull);
              }
              const double vd = (double)v, a = (double)radix_unkey(ckey) - vd;
              const bool in_body = ok && !in_tail;
              double* slot3 = red + (c * 16 + 4 * q + r) * 3;
              slot3[0] = in_body ? exp(a) : 0.0;
              slot3[1] = in_body ? exp(2.0 * a) : 0.0;
              slot3[2] = ok ? exp(vd - (double)tp4[r]) : 0.0;
            }
          }
          if (MODE == 1) {
            // the 16 draws of the tile onto the running sum, one after the other: ((s + t_0) + t_1) + ... -- the order of a
            // thread of loglik_gather_kernel over its segment (a draw past the segment adds 0.0, which changes nothing)
            wave_lds_fence();
            if (lane < 48) {
              double a = sacc[j];
#pragma unroll
              for (int cc = 0; cc < 16; ++cc) a += red[(cc * 16 + (lane & 15)) * 3 + (lane >> 4)];
              sacc[j] = a;
            }
            wave_lds_fence();
          }
        }
      }
      if (kLate) __builtin_amdgcn_sched_barrier(0);        // (the scheduler must not lift the loads back over the arithmetic)
      if (kLate && t + 1 < t1) load(t + 1);
    }

    if (MODE == 0 && first) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (b0 + j < nblk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            uint32_t m = pre_key[j][r];
#pragma unroll
            for (int o = 1; o < 16; o *= 2) {
              const uint32_t other = (uint32_t)__shfl_xor((int)m, o, 64);
              m = other > m ? other : m;
            }
            if (c == 0 && row_ok[j][r]) atomicMax(&topkey[16 * (b0 + j) + 4 * q + r], m);
          }
        }
      }
    }
    if (MODE == 1 && lane < 48) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int row = 16 * (b0 + j) + (lane & 15);
        if (b0 + j < nblk && row < n) part[(chunk * 3 + (lane >> 4)) * (long long)n + row] = sacc[j];
      }
    }
  }

  if (MODE == 0) radix_hist_flush<kGlmRows, kGlmThreads>(hl, b0, n, hist);
}

// ---- the predictive sums ------------------------------------------------------------------------------------------------------
// (NTM = 8 sits at exactly 256 registers, by late loads and per-tile re-reads of the X fragments (kLate).  The plain form --
// fragments held, loads ahead, one wave per SIMD, 298 registers -- was measured beside it: `waic` of 800 000 x 128 draws against
// 1000 rows 10.17 ms against 7.93 ms, profiles/glm_bench.txt.  Should a compiler tip this form into scratch, the test of the
// listing fails and `NTM == 8 ? 1 : 2` here with kLate = false below is the fallback.)
template <typename F, int NTM>
__global__ __launch_bounds__(kGlmThreads, 2) void glm_predict_kernel(const float* __restrict__ W, long long S, int d,
                                                                     const float* __restrict__ P, const float* __restrict__ RC,
                                                                     int n, int NT, int ngroups, long long nchunks, long long tpc,
                                                                     double* __restrict__ part) {
  constexpr int NB = kGlmNB;
  constexpr int REGION = tile_region(NTM);
  __shared__ __attribute__((aligned(16))) float lds_all[4 * REGION];
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
  float rc[3][NB][4];
  bool row_ok[NB][4];
  row_constants<NB, 3>(RC, n, b0, nblk, q, rc, row_ok);
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
  constexpr bool kLate = NTM >= 8;                            // (as in the gather above: late loads, streamed X fragments)
  for (long long t = t0; t < t1; ++t) {
    tile_stage<NTM>(lds, pre, walk, lane);
    wave_lds_fence();
    f4 E[NB];
    if (kLate) {
      const float* Pt = P;
      asm volatile("" : "+s"(Pt));
      block_fragments<NTM, NB>(Pt, NT, b0, nblk, lane, xa, yv);
    }
    tile_logits<NTM, NB>(lds, xa, c, q, NT, b0, nblk, E);
    wave_lds_fence();
    if (!kLate && t + 1 < t1) tile_load<NTM>(W, t + 1, walk, lane, pre);  // in flight during this tile's arithmetic
    const bool valid = 16 * t + c < S;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (b0 + j < nblk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = valid && row_ok[j][r];
          const float mu = F::mean(E[j][r], rc[0][j][r]);
          const float ll = F::ll(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r]);
          const double dll = ok ? (double)ll : 0.0;
          acc[j][0][r] += ok ? (double)mu : 0.0;
          acc[j][1][r] += ok ? exp((double)ll - (double)rc[2][j][r]) : 0.0;
          acc[j][2][r] += dll;
          acc[j][3][r] = fma(dll, dll, acc[j][3][r]);
          __builtin_amdgcn_sched_barrier(0);                // one element's exp at a time: interleaved they spill
        }
      }
    }
    if (kLate) __builtin_amdgcn_sched_barrier(0);
    if (kLate && t + 1 < t1) tile_load<NTM>(W, t + 1, walk, lane, pre);
  }
  tile_sums_out<NB, 4>(lds, acc, lane, b0, nblk, n, chunk, part);
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int l2hmc_glm_log_lik(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts, int32_t n_data,
                      int32_t family, float* out, void* stream) {
  const char* who = "l2hmc_glm_log_lik";
  GlmPlan p;
  if (!glm_plan(who, family, n_draws, n_data, d, false, p)) return L2HMC_ERR_ARG;
  if (n_draws > (1LL << 40) / n_data) return fail(L2HMC_ERR_ARG, "%s: matrix too large (n_draws n_data > 2^40)", who);
  if (!draws || !packed || !row_consts || !out) return fail(L2HMC_ERR_ARG, "%s: draws, packed, row_consts and out are required", who);
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)row_consts & 3) || ((uintptr_t)out & 3))
    return fail(L2HMC_ERR_ARG, "%s: draws, row_consts and out must be 4-byte, packed 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const long long units = (long long)p.ngroups * p.nchunks;
  const dim3 grid((unsigned)((units + 3) / 4)), block(kGlmThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    hipLaunchKernelGGL((glm_loglik_kernel<PoissonLog, decltype(ntm)::value>), grid, block, 0, s, draws, (long long)n_draws, (int)d,
                       packed, row_consts, (int)n_data, p.NT, p.ngroups, p.nchunks, p.tpc, out);
  });
  return launched();
}

int64_t l2hmc_glm_predict_workspace_doubles(int64_t n_draws, int32_t n_data, int32_t d) {
  GlmPlan p;
  if (!glm_plan("l2hmc_glm_predict_workspace_doubles", PoissonLog::kAbi, n_draws, n_data, d, false, p)) return L2HMC_ERR_ARG;
  return p.nchunks * 4 * (int64_t)n_data;
}

int l2hmc_glm_predict(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts, int32_t n_data,
                      int32_t family, double* sums, double* workspace, void* stream) {
  const char* who = "l2hmc_glm_predict";
  GlmPlan p;
  if (!glm_plan(who, family, n_draws, n_data, d, false, p)) return L2HMC_ERR_ARG;
  if (!draws || !packed || !row_consts || !sums || !workspace)
    return fail(L2HMC_ERR_ARG, "%s: draws, packed, row_consts, sums and workspace are required", who);
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)row_consts & 3) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)workspace & 7))
    return fail(L2HMC_ERR_ARG, "%s: draws and row_consts must be 4-byte, packed 16-byte, sums and workspace 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const long long units = (long long)p.ngroups * p.nchunks;
  const dim3 grid((unsigned)((units + 3) / 4)), block(kGlmThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    hipLaunchKernelGGL((glm_predict_kernel<PoissonLog, decltype(ntm)::value>), grid, block, 0, s, draws, (long long)n_draws, (int)d,
                       packed, row_consts, (int)n_data, p.NT, p.ngroups, p.nchunks, p.tpc, workspace);
  });
  chunk_reduce_launch(workspace, p.nchunks, 4LL * n_data, sums, s);
  return launched();
}

int64_t l2hmc_glm_loo_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d) {
  GlmPlan p;
  if (!glm_plan("l2hmc_glm_loo_workspace_bytes", PoissonLog::kAbi, n_draws, n_data, d, true, p)) return L2HMC_ERR_ARG;
  return glm_workspace(nullptr, p, n_data).bytes;
}

int l2hmc_glm_loo_tails(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts,
                        int32_t n_data, int32_t family, const int64_t* tail_len_row, int64_t tail_stride, float* cutoff, float* top,
                        int64_t* n_tail, float* tail, double* sums, void* workspace, void* stream) {
  const char* who = "l2hmc_glm_loo_tails";
  GlmPlan p;
  if (!glm_plan(who, family, n_draws, n_data, d, true, p)) return L2HMC_ERR_ARG;
  if (tail_stride < 0 || tail_stride >= n_draws)
    return fail(L2HMC_ERR_ARG, "%s: 0 <= tail_stride < n_draws (got %lld)", who, (long long)tail_stride);
  if (tail_stride * n_data > (1LL << 31))
    return fail(L2HMC_ERR_ARG, "%s: tail too large (tail_stride n_data > 2^31): fewer rows per call", who);
  if (!draws || !packed || !row_consts || !cutoff || !top || !n_tail || (!tail && tail_stride > 0) || !sums || !workspace)
    return fail(L2HMC_ERR_ARG, "%s: draws, packed, row_consts, cutoff, top, n_tail, tail, sums and workspace are required", who);
  if (((uintptr_t)draws & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)row_consts & 3) || ((uintptr_t)cutoff & 3) ||
      ((uintptr_t)top & 3) || ((uintptr_t)n_tail & 7) || ((uintptr_t)tail & 3) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)workspace & 7) || ((uintptr_t)tail_len_row & 7))
    return fail(L2HMC_ERR_ARG, "%s: draws, row_consts, cutoff, top and tail must be 4-byte, packed 16-byte, n_tail, tail_len_row, "
                               "sums and workspace 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const GlmWorkspace ws = glm_workspace(workspace, p, n_data);
  const long long n = n_data, cells = n * tail_stride > n ? n * tail_stride : n;
  hipLaunchKernelGGL(glm_loo_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, ws.remaining, ws.ranks, ws.prefix,
                     ws.topkey, (unsigned long long*)n_tail, tail, (int)n_data, (long long)tail_stride,
                     (long long)l2hmc_logistic_loo_tail_len(n_draws), (const long long*)tail_len_row, ws.err);
  const dim3 grid((unsigned)(p.quads * p.ngroups)), gather_grid((unsigned)(p.seg_quads * p.ngroups)), block(kGlmThreads);
  auto pass = [&](auto mode, int shift, bool first) {
    constexpr int MODE = decltype(mode)::value;
    on_feature_tiles(p.NTM, [&](auto ntm) {
      hipLaunchKernelGGL((glm_loo_kernel<PoissonLog, decltype(ntm)::value, MODE>), MODE == 1 ? gather_grid : grid, block, 0, s, draws,
                         (long long)n_draws, (int)d, packed, row_consts, (int)n_data, p.NT, p.ngroups,
                         MODE == 1 ? p.nseg : p.nchunks, MODE == 1 ? p.seg_rows : p.tpc, (const uint32_t*)ws.prefix, shift,
                         (int)first, ws.hist, ws.topkey, (const long long*)ws.ranks, top, (unsigned long long*)n_tail, tail,
                         (long long)tail_stride, ws.err, ws.part);
    });
  };
  const int rc = radix_select_passes(ws.hist, ws.remaining, ws.prefix, (int)n_data, cutoff, s,
                                     [&](int shift, bool first) { pass(ic<0>{}, shift, first); });
  if (rc) return rc;
  pass(ic<1>{}, 0, false);
  chunk_reduce_launch(ws.part, p.nseg, 3LL * n_data, sums, s);
  return launched();
}

}  // extern "C"
