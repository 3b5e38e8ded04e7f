// l2hmc_moment_sums -- the raw first and second moments of a recorded history X (steps, N, d) that stays where the sampler
// wrote it: sum x and sum x x^T over every draw, and the same over the batch means of `batch` consecutive steps of one chain.
// l2hmc_amd/multivariate.py turns them into the posterior covariance and the multivariate effective sample size of Vats,
// Flegal & Jones (2019); include/l2hmc.h states the contract, DESIGN.md section 3o the plan and the error argument.
//
// Every product and every sum is float64 on the matrix pipe, v_mfma_f64_16x16x4_f64 (the product of two float32 values is exact
// in float64, so the raw moments lose nothing to the products).  In that form the A operand (row = lane & 15, k = lane >> 4) and
// the B operand (k = lane >> 4, col = lane & 15) of a Gram product are the SAME register: a lane holds coordinate
// 16 tile + (lane & 15) of draw lane >> 4, and the product of tile i with tile j is the 16 x 16 block (i, j) of sum x x^T over the
// wave's 4 draws.  No transposition, no LDS in the loop.
//
//   moment_panel_kernel<TA, TB, DIAG>: a wave owns 4 adjacent chains (its 4 k-slots) and walks the steps of its segment; per
//       step a lane loads one float per tile (the wave reads 4 d contiguous floats of the row, the 4 waves of a block a
//       contiguous run of 16 d), widens it, adds it to its float64 running sum of (chain, coordinate) and feeds the tile pairs
//       of its panel to the MFMAs.  Every `batch` steps the running sums, divided once, are the batch means: they go through
//       the same MFMAs into a second accumulator set and the running sum restarts.  One read of the history per panel serves
//       all four outputs.  8 to 16 steps of loads are in flight per lane (4 to 8 in the off-diagonal panel, which loads 5 to 8 tiles), in two buffers.
//       Panels.  d <= 64 (T = ceil(d / 16) <= 4 tiles): one DIAG panel of all T (T + 1) / 2 pairs.  64 < d <= 128: tiles [0, 4)
//       and [4, T) each get a DIAG panel, and their 4 x (T - 4) cross pairs an off-diagonal one (blockIdx.z); only DIAG panels
//       write the sums.  Accumulators: 8 registers per pair and set, at most 16 pairs x 2 sets = 256 of the 512 a lane has at
//       one wave per SIMD.
//       Blocks: x walks the chunks of 16 chains (chunk b, b + gridDim.x, ...: the accumulators stay in registers across
//       chunks), y cuts the steps into segments at batch boundaries (few chains: more segments).  After the loop the 4 waves
//       are added through LDS in wave order and the block writes ONE partial, in fragment layout, to the workspace.
//   moment_reduce_kernel: every entry of the outputs = the blocks' partials added in block order; entry (a, b) and (b, a) read
//       the same partials (those of (min, max)), so both triangles carry identical bits.  No floating-point atomics anywhere.
//
// A lane outside the history (coordinate >= d, chain >= N) loads a clamped, valid address and SELECTS 0.0 -- it never multiplies
// what it loaded -- so padding contributes exact zeros, and a non-finite entry reaches the rows and columns of its own
// coordinate only (block (i, j) entry (r, c) is made of coordinates 16 i + r and 16 j + c and nothing else).
#include "l2hmc_kernels.hpp"

namespace l2hmc {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMsWaves = 4;                    // waves per block = chain groups per chunk
constexpr int kMsThreads = 64 * kMsWaves;
constexpr int kMsBlocks = 256;                 // blocks per panel the planner aims for: one wave per SIMD on 256 CUs
constexpr int kMsLoads = 8;                    // steps per load buffer (two buffers; half as many in the off-diagonal panel)
constexpr int kMsHalf = 4;                     // tiles of a DIAG panel at most (<= kMsWaves: the block-end sum of the sums)
constexpr int kMsMaxD = 128;

struct MomentPlan {
  int T, npanel, P, nsets;          // tiles, panels, pairs of the largest panel, accumulator sets (1: no batches)
  long long J, nchunks, nbx, nseg;  // row length, chunks of 16 chains, blocks along x, step segments
  long long units, unit, rem;       // segments are cut in units of `unit` rows after the first `rem` rows
  long long set_stride, stride;     // doubles per set and per block in the workspace
};

__host__ __device__ inline int ms_diag_pairs(int t) { return t * (t + 1) / 2; }

static bool moment_plan(const char* who, int64_t steps, int64_t n_chains, int32_t d, int64_t batch, MomentPlan& p) {
  if (d < 1 || d > kMsMaxD) { fail(L2HMC_ERR_ARG, "%s: 1 <= d <= 128 (got %lld)", who, d); return false; }
  if (steps < 1 || n_chains < 1) { fail(L2HMC_ERR_ARG, "%s: steps and n_chains must be >= 1 (got %lld, %lld)", who, steps, n_chains); return false; }
  if (batch < 0 || batch > steps) { fail(L2HMC_ERR_ARG, "%s: 0 <= batch <= steps = %lld (got %lld)", who, steps, batch); return false; }
  if (n_chains > (1LL << 40) / d || steps > (1LL << 31)) { fail(L2HMC_ERR_ARG, "%s: history too large", who); return false; }
  p.T = (d + 15) / 16;
  p.npanel = p.T <= kMsHalf ? 1 : 3;
  p.P = p.T <= kMsHalf ? ms_diag_pairs(p.T) : (ms_diag_pairs(kMsHalf) > kMsHalf * (p.T - kMsHalf) ? ms_diag_pairs(kMsHalf)
                                                                                                 : kMsHalf * (p.T - kMsHalf));
  p.nsets = batch > 0 ? 2 : 1;
  p.J = n_chains * d;
  p.nchunks = (n_chains + 4 * kMsWaves - 1) / (4 * kMsWaves);
  p.nbx = p.nchunks < kMsBlocks ? p.nchunks : kMsBlocks;
  p.unit = batch > 0 ? batch : 1;
  p.units = steps / p.unit;
  p.rem = steps - p.units * p.unit;
  p.nseg = (kMsBlocks + p.nbx - 1) / p.nbx;
  if (p.nseg > p.units) p.nseg = p.units;
  p.set_stride = (long long)p.P * 256 + kMsHalf * 64;
  p.stride = p.set_stride * p.nsets;
  return true;
}

// the tile pairs of a panel, both as compile-time lists: pair p of a DIAG panel is (i, j), i <= j, in row order; of an
// off-diagonal one (i, TA + j) with p = i TB + j
template <int TA, int TB, bool DIAG>
struct MsPanel {
  static constexpr int NT = DIAG ? TA : TA + TB;
  static constexpr int NP = DIAG ? TA * (TA + 1) / 2 : TA * TB;
};

template <int TA, int TB, bool DIAG>
__device__ __forceinline__ void ms_gram(const double (&v)[MsPanel<TA, TB, DIAG>::NT], d4 (&acc)[MsPanel<TA, TB, DIAG>::NP]) {
  int p = 0;
  if constexpr (DIAG) {
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = i; j < TA; ++j, ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[i], v[j], acc[p], 0, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TB; ++j, ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[i], v[TA + j], acc[p], 0, 0, 0);
  }
}

// tile0a / tile0b: the first tile of the A range and of the B range (DIAG: the B range is the A range)
template <int TA, int TB, bool DIAG>
__global__ __launch_bounds__(kMsThreads) void moment_panel_kernel(const float* __restrict__ X, long long J, long long N, int d,
                                                                  int tile0a, int tile0b, long long batch, long long rem,
                                                                  long long units, long long unit, long long nchunks,
                                                                  long long part_block0, long long stride, long long set_stride,
                                                                  int P, double* __restrict__ part) {
  using Pn = MsPanel<TA, TB, DIAG>;
  constexpr int NT = Pn::NT, NP = Pn::NP;
  __shared__ double sm[kMsWaves][4][64];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;

  // this block's rows: units [u0, u1) after the leading remainder, which the first segment walks too
  const long long u0 = units * blockIdx.y / gridDim.y, u1 = units * (blockIdx.y + 1) / gridDim.y;
  const long long t0 = blockIdx.y == 0 ? 0 : rem + u0 * unit, t1 = rem + u1 * unit;

  d4 acc[NP], bacc[NP];
  double s[NT], bs[NT];
#pragma unroll
  for (int p = 0; p < NP; ++p) { acc[p] = d4{0.0, 0.0, 0.0, 0.0}; bacc[p] = d4{0.0, 0.0, 0.0, 0.0}; }
#pragma unroll
  for (int n = 0; n < NT; ++n) { s[n] = 0.0; bs[n] = 0.0; }

  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long long chain0 = (chunk * kMsWaves + w) * 4;
    if (chain0 >= N) continue;                            // wave-uniform; nothing below synchronises the block
    const long long chain = chain0 + q;
    bool live[NT];
    long long off[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int k = 16 * ((n < TA ? tile0a : tile0b - TA) + n) + c;
      live[n] = k < d && chain < N;
      off[n] = (chain < N ? chain : N - 1) * d + (k < d ? k : d - 1);     // always inside the row
    }
    double sb[NT];                                        // the running sum of the batch in progress
#pragma unroll
    for (int n = 0; n < NT; ++n) sb[n] = 0.0;
    // rows until the running sums are flushed; the first flush of a block that walks the leading remainder only moves them
    // into the column sums (those rows belong to no batch).  batch = 0: one flush, at the end, of that kind.
    bool whole = batch > 0 && !(blockIdx.y == 0 && rem > 0);
    long long left = batch > 0 ? (whole ? batch : rem) : (t1 - t0);

    // two buffers of U steps: the loads of the next U steps are issued before the arithmetic of the current U, so a wave
    // that is alone on its SIMD always has U .. 2 U rows in flight.  Rows are clamped to the segment (a load past its end is
    // of a valid address and is not used).
    constexpr int U = NT > 4 ? kMsLoads / 2 : kMsLoads;
    float xa[U][NT], xb[U][NT];
    auto load = [&](float (&x)[U][NT], long long t) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = t + u < t1 ? t + u : t1 - 1;
#pragma unroll
        for (int n = 0; n < NT; ++n) x[u][n] = X[row * J + off[n]];
      }
    };
    auto work = [&](const float (&x)[U][NT], long long t) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < t1) {
          double v[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            v[n] = live[n] ? (double)x[u][n] : 0.0;
            sb[n] += v[n];
          }
          ms_gram<TA, TB, DIAG>(v, acc);
          if (--left == 0) {
            if (whole) {
              const double den = (double)batch;
              double y[NT];
#pragma unroll
              for (int n = 0; n < NT; ++n) {
                y[n] = sb[n] / den;
                bs[n] += y[n];
              }
              ms_gram<TA, TB, DIAG>(y, bacc);
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) { s[n] += sb[n]; sb[n] = 0.0; }
            whole = batch > 0;
            left = batch > 0 ? batch : -1;
          }
        }
      }
    };
    load(xa, t0);
    for (long long t = t0; t < t1; t += 2 * U) {
      load(xb, t + U);
      work(xa, t);
      load(xa, t + 2 * U);
      work(xb, t + U);
    }
  }

  // the block's partial: the 4 waves added in wave order, register r of a pair by wave r
  double* out = part + (part_block0 + (long long)blockIdx.y * gridDim.x + blockIdx.x) * stride;
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    if (set == 1 && batch == 0) break;
    double* o = out + set * set_stride;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const d4 a = set ? bacc[p] : acc[p];
      __syncthreads();
      sm[w][0][lane] = a[0]; sm[w][1][lane] = a[1]; sm[w][2][lane] = a[2]; sm[w][3][lane] = a[3];
      __syncthreads();
      o[(p * 4 + w) * 64 + lane] = ((sm[0][w][lane] + sm[1][w][lane]) + sm[2][w][lane]) + sm[3][w][lane];
    }
    if constexpr (DIAG) {
      __syncthreads();
#pragma unroll
      for (int n = 0; n < TA; ++n) sm[w][n][lane] = set ? bs[n] : s[n];
      __syncthreads();
      if (w < TA) o[(long long)P * 256 + w * 64 + lane] = ((sm[0][w][lane] + sm[1][w][lane]) + sm[2][w][lane]) + sm[3][w][lane];
    }
  }
}

// blockIdx.y = set (0: sum / cross, 1: batch_sum / batch_cross); nb = blocks per panel
__global__ void moment_reduce_kernel(const double* __restrict__ part, long long nb, long long stride, long long set_stride, int P,
                                     int T, int d, double* __restrict__ sum0, double* __restrict__ cross0,
                                     double* __restrict__ sum1, double* __restrict__ cross1) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int set = blockIdx.y;
  const double* base = part + set * set_stride;
  if (idx < d * d) {
    const int a = idx / d, b = idx - a * d;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int i = lo >> 4, j = hi >> 4, row = lo & 15, col = hi & 15;
    int panel, p;
    if (T <= kMsHalf) {
      panel = 0; p = i * T - i * (i - 1) / 2 + (j - i);
    } else if (j < kMsHalf) {
      panel = 0; p = i * kMsHalf - i * (i - 1) / 2 + (j - i);
    } else if (i >= kMsHalf) {
      const int ii = i - kMsHalf, jj = j - kMsHalf, t2 = T - kMsHalf;
      panel = 1; p = ii * t2 - ii * (ii - 1) / 2 + (jj - ii);
    } else {
      panel = 2; p = i * (T - kMsHalf) + (j - kMsHalf);
    }
    // the f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg.  A diagonal block holds both (row, col) and (col, row);
    // row <= col there (lo <= hi), so one of the two is read for both triangles.
    const long long o = (long long)(p * 4 + (row >> 2)) * 64 + col + 16 * (row & 3);
    double acc = 0.0;
    for (long long blk = panel * nb; blk < (panel + 1) * nb; ++blk) acc += base[blk * stride + o];
    (set ? cross1 : cross0)[idx] = acc;
  } else if (idx < d * d + d) {
    const int k = idx - d * d, i = k >> 4, cc = k & 15;
    const int panel = (T > kMsHalf && i >= kMsHalf) ? 1 : 0, n = panel ? i - kMsHalf : i;
    const long long o = (long long)P * 256 + n * 64 + cc;
    double acc = 0.0;
    for (long long blk = panel * nb; blk < (panel + 1) * nb; ++blk)
      for (int q = 0; q < 4; ++q) acc += base[blk * stride + o + 16 * q];
    (set ? sum1 : sum0)[k] = acc;
  }
}

template <int TA, int TB, bool DIAG>
static void moment_launch(const MomentPlan& p, int panel, int tile0a, int tile0b, const float* X, long long N, int d, long long batch,
                          double* ws, hipStream_t s) {
  hipLaunchKernelGGL((moment_panel_kernel<TA, TB, DIAG>), dim3((unsigned)p.nbx, (unsigned)p.nseg), dim3(kMsThreads), 0, s, X, p.J, N,
                     d, tile0a, tile0b, batch, p.rem, p.units, p.unit, p.nchunks, (long long)panel * p.nbx * p.nseg, p.stride,
                     p.set_stride, p.P, ws);
}

static void moment_diag(const MomentPlan& p, int panel, int tile0, int tiles, const float* X, long long N, int d, long long batch,
                        double* ws, hipStream_t s) {
  switch (tiles) {
    case 1: moment_launch<1, 1, true>(p, panel, tile0, tile0, X, N, d, batch, ws, s); break;
    case 2: moment_launch<2, 2, true>(p, panel, tile0, tile0, X, N, d, batch, ws, s); break;
    case 3: moment_launch<3, 3, true>(p, panel, tile0, tile0, X, N, d, batch, ws, s); break;
    default: moment_launch<4, 4, true>(p, panel, tile0, tile0, X, N, d, batch, ws, s); break;
  }
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_moment_sums_workspace_doubles(int64_t steps, int64_t n_chains, int32_t d, int64_t batch) {
  MomentPlan p;
  if (!moment_plan("l2hmc_moment_sums_workspace_doubles", steps, n_chains, d, batch, p)) return L2HMC_ERR_ARG;
  return p.stride * p.nbx * p.nseg * p.npanel;
}

int l2hmc_moment_sums(const float* X, int64_t steps, int64_t n_chains, int32_t d, int64_t batch, double* sum_out,
                      double* cross_out, double* batch_sum_out, double* batch_cross_out, double* workspace, void* stream) {
  MomentPlan p;
  if (!moment_plan("l2hmc_moment_sums", steps, n_chains, d, batch, p)) return L2HMC_ERR_ARG;
  if (!X || !sum_out || !cross_out || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_moment_sums: X, sum_out, cross_out and workspace are required%s");
  if (batch == 0 && (batch_sum_out || batch_cross_out))
    return fail(L2HMC_ERR_ARG, "l2hmc_moment_sums: batch_sum_out and batch_cross_out must be NULL when batch = 0%s");
  if (batch > 0 && (!batch_sum_out || !batch_cross_out))
    return fail(L2HMC_ERR_ARG, "l2hmc_moment_sums: batch_sum_out and batch_cross_out are required when batch > 0%s");
  hipStream_t s = (hipStream_t)stream;
  if (p.npanel == 1) {
    moment_diag(p, 0, 0, p.T, X, n_chains, d, batch, workspace, s);
  } else {
    moment_diag(p, 0, 0, kMsHalf, X, n_chains, d, batch, workspace, s);
    moment_diag(p, 1, kMsHalf, p.T - kMsHalf, X, n_chains, d, batch, workspace, s);
    switch (p.T - kMsHalf) {
      case 1: moment_launch<4, 1, false>(p, 2, 0, kMsHalf, X, n_chains, d, batch, workspace, s); break;
      case 2: moment_launch<4, 2, false>(p, 2, 0, kMsHalf, X, n_chains, d, batch, workspace, s); break;
      case 3: moment_launch<4, 3, false>(p, 2, 0, kMsHalf, X, n_chains, d, batch, workspace, s); break;
      default: moment_launch<4, 4, false>(p, 2, 0, kMsHalf, X, n_chains, d, batch, workspace, s); break;
    }
  }
  hipLaunchKernelGGL(moment_reduce_kernel, dim3((unsigned)((d * d + d + 255) / 256), (unsigned)p.nsets), dim3(256), 0, s,
                     (const double*)workspace, p.nbx * p.nseg, p.stride, p.set_stride, p.P, p.T, (int)d, sum_out, cross_out,
                     batch_sum_out, batch_cross_out);
  return launched();
}

}  // extern "C"
