// The kernels of csrc/glm.hip -- the matrix writer, the count / gather kernel of the tails and the predictive sums -- as
// templates over the family (glm_family.hpp), and the launch of each.  glm.hip holds the entries, the plans, the workspace and the
// Poisson instantiations; glm_binomial.hip instantiates the launches of BinomialLogit and NegBinomialLog (a unit of their own:
// one compile per family set, and glm.hip's listing stays the Poisson kernels').  glm.hip's header describes the kernels.
#pragma once
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

// the constants of the rows a lane meets: rc[k][j][r] = row_consts[k][16 (b0 + j) + 4 q + r], 0 for a dead row
// (SKIP_SAT: rc[2] is row_consts[3] -- the three constants of a family whose ll takes three, without sat)
template <int NB, int KC, bool SKIP_SAT = false>
__device__ __forceinline__ void row_constants(const float* __restrict__ RC, int n, int b0, int nblk, int q, float (&rc)[KC][NB][4],
                                              bool (&row_ok)[NB][4]) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (b0 + j) + 4 * q + r;
      row_ok[j][r] = b0 + j < nblk && row < n;
#pragma unroll
      for (int k = 0; k < KC; ++k) rc[k][j][r] = row_ok[j][r] ? RC[(long long)((SKIP_SAT && k >= 2) ? k + 1 : k) * n + row] : 0.f;
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
  constexpr int KC = F::kConsts;
  float rc[KC][NB][4];
  bool row_ok[NB][4];
  row_constants<NB, KC, true>(RC, n, b0, nblk, q, rc, row_ok);

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
          const float ll = family_ll<F>(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r], rc[KC - 1][j][r]);
          if (valid && row_ok[j][r]) out[draw * n + (16 * (b0 + j) + 4 * q + r)] = ll;
        }
      }
    }
  }
}

// ---- the tails ----------------------------------------------------------------------------------------------------------------
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
  // (a family whose ll takes three constants: the third is a fifth number)
  constexpr int KC = F::kConsts;
  __shared__ __attribute__((aligned(16))) float rowc[MODE == 1 ? (2 + KC) * kGlmRows : 4];
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
    if constexpr (KC == 3) rowc[4 * kGlmRows + i] = live ? RC[3LL * n + row] : 0.f;
    if (live && blockIdx.x < (unsigned)ngroups) top[row] = tv;          // (the first quad of chunks writes the row's maximum out)
  }
  __syncthreads();

  if (live_wave) {
    f4 xa[NB][NTM], yv[NB];
    block_fragments<NTM, NB>(P, NT, b0, nblk, lane, xa, yv);
    float rc[KC][NB][4];              // count: the row's offset and g (the constants of the family's ll)
    bool row_ok[NB][4];
    uint32_t pre_key[NB][4];          // count: the row's prefix above the digit (pass 0: the running largest key)
    if (MODE == 0) row_constants<NB, KC, true>(RC, n, b0, nblk, q, rc, row_ok);
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
          if constexpr (KC == 3) rc[2][j][r] = 0.f;
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
          [[maybe_unused]] f4 c4 = o4;
          if (MODE == 1) {
            const float* rp = rowc + 16 * j + 4 * q;         // (opaque: the reads stay inside the loop)
            asm volatile("" : "+v"(rp));
            o4 = lds4(rp); g4 = lds4(rp + kGlmRows); ck4 = lds4(rp + 2 * kGlmRows); tp4 = lds4(rp + 3 * kGlmRows);
            if constexpr (KC == 3) c4 = lds4(rp + 4 * kGlmRows);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = MODE == 1 ? family_ll<F>(E[j][r], yv[j][r], o4[r], g4[r], c4[r])
                                      : family_ll<F>(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r], rc[KC - 1][j][r]);
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
  constexpr int KC = F::kConsts;      // rc: the constants of ll and sat (rc[2]) -- all of row_consts
  // ... except at NTM = 8 for a family of three constants: sat and the third are read again for every element (L2-hot, as the
  // X fragments are under kLate below) -- held across the tile loop, their 16 registers put this geometry into scratch
  constexpr bool kStreamConsts = KC == 3 && NTM >= 8;
  constexpr int KR = kStreamConsts ? 2 : KC + 1;
  float rc[KR][NB][4];
  bool row_ok[NB][4];
  row_constants<NB, KR>(RC, n, b0, nblk, q, rc, row_ok);
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
          float sat, k2;
          if constexpr (kStreamConsts) {
            const float* rp = RC;                            // (opaque: the reads stay inside the loop)
            asm volatile("" : "+s"(rp));
            const long long row = 16 * (b0 + j) + 4 * q + r;
            sat = row_ok[j][r] ? rp[2LL * n + row] : 0.f;
            k2 = row_ok[j][r] ? rp[3LL * n + row] : 0.f;
          } else {
            sat = rc[2][j][r];
            k2 = rc[KR - 1][j][r];
          }
          const float mu = family_mean<F>(E[j][r], rc[0][j][r], rc[1][j][r]);
          const float ll = family_ll<F>(E[j][r], yv[j][r], rc[0][j][r], rc[1][j][r], k2);
          const double dll = ok ? (double)ll : 0.0;
          acc[j][0][r] += ok ? (double)mu : 0.0;
          acc[j][1][r] += ok ? exp((double)ll - (double)sat) : 0.0;
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


// ---- the launches ---------------------------------------------------------------------------------------------------------------
template <typename F>
void glm_launch_matrix(const GlmPlan& p, hipStream_t s, const float* draws, long long n_draws, int d, const float* packed,
                       const float* row_consts, int n_data, float* out) {
  const long long units = (long long)p.ngroups * p.nchunks;
  const dim3 grid((unsigned)((units + 3) / 4)), block(kGlmThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    hipLaunchKernelGGL((glm_loglik_kernel<F, decltype(ntm)::value>), grid, block, 0, s, draws, n_draws, d, packed, row_consts, n_data,
                       p.NT, p.ngroups, p.nchunks, p.tpc, out);
  });
}

template <typename F>
void glm_launch_predict(const GlmPlan& p, hipStream_t s, const float* draws, long long n_draws, int d, const float* packed,
                        const float* row_consts, int n_data, double* workspace) {
  const long long units = (long long)p.ngroups * p.nchunks;
  const dim3 grid((unsigned)((units + 3) / 4)), block(kGlmThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    hipLaunchKernelGGL((glm_predict_kernel<F, decltype(ntm)::value>), grid, block, 0, s, draws, n_draws, d, packed, row_consts, n_data,
                       p.NT, p.ngroups, p.nchunks, p.tpc, workspace);
  });
}

// one pass of the tails: MODE 0 a count pass at `shift`, MODE 1 the gather
struct GlmTailArgs {
  const uint32_t* prefix;
  unsigned long long* hist;
  uint32_t* topkey;
  const long long* ranks;
  float* top;
  unsigned long long* n_tail;
  float* tail;
  long long stride;
  unsigned long long* err;
  double* part;
};
template <typename F, int MODE>
void glm_launch_tails(const GlmPlan& p, hipStream_t s, const float* draws, long long n_draws, int d, const float* packed,
                      const float* row_consts, int n_data, int shift, bool first, const GlmTailArgs& t) {
  const dim3 grid((unsigned)(p.quads * p.ngroups)), gather_grid((unsigned)(p.seg_quads * p.ngroups)), block(kGlmThreads);
  on_feature_tiles(p.NTM, [&](auto ntm) {
    hipLaunchKernelGGL((glm_loo_kernel<F, decltype(ntm)::value, MODE>), MODE == 1 ? gather_grid : grid, block, 0, s, draws, n_draws, d,
                       packed, row_consts, n_data, p.NT, p.ngroups, MODE == 1 ? p.nseg : p.nchunks, MODE == 1 ? p.seg_rows : p.tpc,
                       t.prefix, shift, (int)first, t.hist, t.topkey, t.ranks, t.top, t.n_tail, t.tail, t.stride, t.err, t.part);
  });
}

// the launches of the binomial and the negative-binomial family live in glm_binomial.hip (the two share ll: the matrix and the
// tails of either are BinomialLogit's), those of the probit family in glm_probit.hip
#define L2HMC_GLM_LAUNCHES(KEYWORD, F)                                                                                            \
  KEYWORD template void glm_launch_matrix<F>(const GlmPlan&, hipStream_t, const float*, long long, int, const float*, const float*, \
                                             int, float*);                                                                         \
  KEYWORD template void glm_launch_tails<F, 0>(const GlmPlan&, hipStream_t, const float*, long long, int, const float*,           \
                                               const float*, int, int, bool, const GlmTailArgs&);                                  \
  KEYWORD template void glm_launch_tails<F, 1>(const GlmPlan&, hipStream_t, const float*, long long, int, const float*,           \
                                               const float*, int, int, bool, const GlmTailArgs&);
#define L2HMC_GLM_PREDICT(KEYWORD, F)                                                                                             \
  KEYWORD template void glm_launch_predict<F>(const GlmPlan&, hipStream_t, const float*, long long, int, const float*,            \
                                              const float*, int, double*);

}  // namespace l2hmc
