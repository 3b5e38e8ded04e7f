// The draw-tile statistics kernels' common ground, stated once.  predict_kernel (predictive.hip), loo_kernel (loo.hip), the
// lik_*_kernels (lik_stats.hip) and the three kernels of glm.hip stream 16-draw tiles of a history W (S, d) past the data blocks
// a wave keeps in registers; this file holds what they share, on the device and on the host.
//   load     a tile is 16 d contiguous floats of W whatever d is.  The lanes load it with coalesced SCALAR loads (the base of a
//            history slice is only 4-byte aligned), element e = lane + 64 i, one tile ahead of its use; 0 past the end of W;
//   stage    element e is (draw e / d, feature e % d), walked without a division, written to the wave's own LDS region as
//            [16 draws][16 NTM + 4]; feature columns d .. 16 NTM - 1 are zeroed once and never written: they add nothing;
//   logits   lane (c, q) reads the B operand {w[16 t + c][16 tg + 4 q + r]} with one 16-byte LDS read per feature tile and gets
//            L^T[i, c] in C/D layout (f32-input MFMA, the operand layouts of regression_grad in l2hmc_kernels.hpp): the logits of
//            draw c, rows 4 q + r of each data block, feature tiles added in the order tg = 0 .. NT - 1 onto zero;
//   end      once per wave the 16 draw lanes of every float64 sum are added through LDS in the order c = 0 .. 15 and go to
//            part[chunk][K][n]; chunk_reduce_kernel then adds the chunks' partials in chunk order.  No floating-point atomics.
// The LDS region is private to the wave (LDS operations of a wave execute in order; wave_lds_fence keeps the compiler from moving
// them), so the tile loop has no workgroup barrier.
//   plan     draw_plan: the argument checks, the compiled feature-tile count (draw_ntm) and the split of the draws into chunks
//            of tpc tiles -- from n_draws ALONE for the tails (the order in which float64 terms are added must not depend on how
//            many rows a call holds), or filling kDrawUnits waves for the sums and the matrix; on_feature_tiles names the
//            kernel of a plan.  Every unit's plan is a DrawPlan and nothing else decides these numbers.
#pragma once
#include "l2hmc_kernels.hpp"

namespace l2hmc {

// the argument checks every entry on a history shares; false with the message set
static bool logistic_history_args_ok(const char* who, int64_t n_draws, int32_t n_data, int32_t d) {
  if (n_draws < 2) { fail(L2HMC_ERR_ARG, "%s: n_draws >= 2 (got %lld)", who, n_draws); return false; }
  if (n_data < 1 || n_data > kLogisticMaxRows) {
    fail(L2HMC_ERR_ARG, "%s: 1 <= n_data <= 1048576 (got %lld)", who, n_data);
    return false;
  }
  if (d < 1 || d > kLogisticMaxDim) { fail(L2HMC_ERR_ARG, "%s: 1 <= d <= 128 (got %lld)", who, d); return false; }
  if (n_draws > (1LL << 40) / d) { fail(L2HMC_ERR_ARG, "%s: draws too large (n_draws d > 2^40)", who); return false; }
  return true;
}

constexpr int kDrawChunks = 1024;         // by_draws: draw chunks aimed for, whatever n is
constexpr int kDrawUnits = 4096;          // else: waves aimed for (two resident sets of 256 CUs x 8)
constexpr int kDrawMinTiles = 4;          // draw tiles per chunk at least: the end-of-wave reduction costs about one tile

// the feature tiles a kernel is compiled for: 1, 2, 4, 8 (d <= 128)
inline int draw_ntm(int NT) { return NT <= 2 ? NT : NT <= 4 ? 4 : 8; }

// f(ic<NTM>) for the compiled feature-tile count of a plan
template <class F>
void on_feature_tiles(int NTM, F&& f) {
  switch (NTM) {
    case 1: f(ic<1>{}); break;
    case 2: f(ic<2>{}); break;
    case 4: f(ic<4>{}); break;
    default: f(ic<8>{}); break;
  }
}

// NB 16-row data blocks per wave make a row group; a chunk is tpc consecutive 16-draw tiles; a quad is four chunks
struct DrawPlan {
  int NT, NTM, nblk, ngroups;
  long long ntiles, tpc, nchunks, quads;
};

// by_draws: tpc from n_draws alone, aiming for kDrawChunks chunks; else the chunks fill kDrawUnits waves with the row groups
static bool draw_plan(const char* who, int64_t n_draws, int32_t n_data, int32_t d, int NB, bool by_draws, DrawPlan& p) {
  if (!logistic_history_args_ok(who, n_draws, n_data, d)) return false;
  p.NT = tiles_of(d);
  p.NTM = draw_ntm(p.NT);
  p.nblk = (n_data + 15) / 16;
  p.ngroups = (p.nblk + NB - 1) / NB;
  p.ntiles = (n_draws + 15) / 16;
  long long want = by_draws ? kDrawChunks : (kDrawUnits + p.ngroups - 1) / p.ngroups;
  if (want > p.ntiles) want = p.ntiles;
  p.tpc = (p.ntiles + want - 1) / want;
  if (p.tpc < kDrawMinTiles) p.tpc = kDrawMinTiles;
  p.nchunks = (p.ntiles + p.tpc - 1) / p.tpc;                // no empty chunk
  p.quads = (p.nchunks + 3) / 4;
  return true;
}

// the segments of consecutive draws whose float64 terms loglik_gather_kernel (loglik_tails.hip) and glm_loo_kernel<*, *, 1>
// (glm.hip) add in draw order: a function of n_draws ALONE, and one function, because the two routes promise the same bits
constexpr int kDrawSegments = 2048;       // segments aimed for
constexpr int kDrawMinSegment = 64;       // draws per segment at least
inline void draw_segments(int64_t n_draws, long long& rows, long long& nseg) {
  rows = (n_draws + kDrawSegments - 1) / kDrawSegments;
  if (rows < kDrawMinSegment) rows = kDrawMinSegment;
  nseg = (n_draws + rows - 1) / rows;                        // no empty segment
}

constexpr int tile_stride(int NTM) { return 16 * NTM + 4; }       // floats per staged draw (a multiple of 4: 16-byte reads)
// floats of a wave's LDS region (a multiple of 64); the end reduction needs 256 doubles
constexpr int tile_region(int NTM) { return 16 * tile_stride(NTM) > 512 ? 16 * tile_stride(NTM) : 512; }

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NTM>
__device__ __forceinline__ void tile_region_clear(float* lds, int lane) {
#pragma unroll
  for (int i = 0; i < tile_region(NTM) / 64; ++i) lds[lane + 64 * i] = 0.f;
}

// a lane's walk over the elements e = lane + 64 i of a tile: (row0, col0) is element `lane`, a step of 64 adds (dq, dr)
struct TileWalk {
  int d, tile_elems, row0, col0, dq, dr;
  long long total;
};

__device__ __forceinline__ TileWalk tile_walk(int lane, int d, long long S) {
  const int row0 = lane / d, dq = 64 / d;
  return TileWalk{d, 16 * d, row0, lane - row0 * d, dq, 64 - dq * d, S * d};
}

// the loads of draw tile t: 4 NTM per lane, 64 x 4 NTM >= 16 d
template <int NTM>
__device__ __forceinline__ void tile_load(const float* __restrict__ W, long long t, const TileWalk& k, int lane,
                                          float (&pre)[4 * NTM]) {
#pragma unroll
  for (int i = 0; i < 4 * NTM; ++i) {
    const int e = lane + 64 * i;
    const long long g = t * k.tile_elems + e;
    pre[i] = (e < k.tile_elems && g < k.total) ? W[g] : 0.f;
  }
}

// the same tile cut out of ONE step of a history (steps, N, d): the 1 <= `live` <= 16 chains from draw `draw0` on
// (lik_stats.hip walks the steps of 16 chains); a chain at or past `live` enters as 0, like a draw past the end above.  Every
// lane loads -- an element past the live ones reads the last live one and drops it -- so the loads need no branch.
template <int NTM>
__device__ __forceinline__ void tile_load_at(const float* __restrict__ W, long long draw0, int live, const TileWalk& k, int lane,
                                             float (&pre)[4 * NTM]) {
  const float* base = W + draw0 * k.d;
  const int lim = live * k.d;
#pragma unroll
  for (int i = 0; i < 4 * NTM; ++i) {
    const int e = lane + 64 * i;
    // (a 32-bit byte offset from the wave-uniform base: one address register per load, not two; lim <= 16 x 128)
    const unsigned off = 4u * (unsigned)(e < lim ? e : lim - 1);
    const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + off);
    pre[i] = e < lim ? v : 0.f;
  }
}

template <int NTM>
__device__ __forceinline__ void tile_stage(float* lds, const float (&pre)[4 * NTM], const TileWalk& k, int lane) {
  // the walk's LDS addresses depend on the lane alone; seen as loop invariants they are hoisted out of the tile loop and
  // held in 4 NTM vector registers across it.  They cost three integer operations each: recompute them per tile.
  int row = k.row0, col = k.col0;
  asm volatile("" : "+v"(row), "+v"(col));
#pragma unroll
  for (int i = 0; i < 4 * NTM; ++i) {
    if (lane + 64 * i < k.tile_elems) lds[row * tile_stride(NTM) + col] = pre[i];
    row += k.dq;
    col += k.dr;
    if (col >= k.d) { col -= k.d; row += 1; }
  }
}

// the XA fragments and labels of data blocks b0 .. b0 + NB - 1 of the packed data P: a dead block reads block nblk - 1 (its
// results are never used), a dead feature tile is zero
template <int NTM, int NB>
__device__ __forceinline__ void block_fragments(const float* __restrict__ P, int NT, int b0, int nblk, int lane,
                                                f4 (&xa)[NB][NTM], f4 (&yv)[NB]) {
  const int BS = logistic_block_floats(NT);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const bool live = b0 + j < nblk;
    const float* blk = P + (size_t)(live ? b0 + j : nblk - 1) * BS;
#pragma unroll
    for (int tg = 0; tg < NTM; ++tg) xa[j][tg] = (live && tg < NT) ? lds4(blk + (tg * 64 + lane) * 4) : splat(0.f);
    yv[j] = lds4(blk + 512 * NT + 4 * (lane >> 4));
  }
}

// THE logits of the staged tile, unsigned: L[j][r] = x_i . w_s of draw c, row 16 (b0 + j) + 4 q + r.  Feature tiles in the order
// tg = 0 .. NT - 1, four MFMAs each, onto zero -- the bits depend on (W, X) alone.
template <int NTM, int NB>
__device__ __forceinline__ void tile_logits(const float* lds, const f4 (&xa)[NB][NTM], int c, int q, int NT, int b0, int nblk,
                                            f4 (&L)[NB]) {
#pragma unroll
  for (int j = 0; j < NB; ++j) L[j] = splat(0.f);
#pragma unroll
  for (int tg = 0; tg < NTM; ++tg) {
    if (tg < NT) {                                           // wave-uniform, like the block test: the MFMAs run with every lane
      const f4 B = lds4(lds + c * tile_stride(NTM) + 16 * tg + 4 * q);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (b0 + j < nblk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) L[j] = MFMA16(xa[j][tg][r], B[r], L[j]);
        }
      }
    }
  }
}

// the 16 draw lanes of every (data block, sum, row), added in the order c = 0 .. 15; rows at or past n are never written
template <int NB, int K>
__device__ __forceinline__ void tile_sums_out(float* lds, const double (&acc)[NB][K][4], int lane, int b0, int nblk, int n,
                                              long long chunk, double* __restrict__ part) {
  const int c = lane & 15, q = lane >> 4;
  double* red = reinterpret_cast<double*>(lds);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (b0 + j < nblk) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 4; ++r) red[c * 16 + 4 * q + r] = acc[j][k][r];
        wave_lds_fence();
        if (lane < 16) {
          double a = red[lane];
#pragma unroll
          for (int cc = 1; cc < 16; ++cc) a += red[cc * 16 + lane];
          const int row = 16 * (b0 + j) + lane;
          if (row < n) part[(chunk * K + k) * (long long)n + row] = a;
        }
      }
    }
  }
}

// sums[i] = the chunks' partials of entry i = k n + row, added in chunk order.  (static: one copy per including unit)
static __global__ void chunk_reduce_kernel(const double* __restrict__ part, long long nchunks, long long m,
                                           double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double a = 0.0;
  for (long long ch = 0; ch < nchunks; ++ch) a += part[ch * m + i];
  sums[i] = a;
}

static void chunk_reduce_launch(const double* part, long long nchunks, long long m, double* sums, hipStream_t s) {
  hipLaunchKernelGGL(chunk_reduce_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, part, nchunks, m, sums);
}

}  // namespace l2hmc
