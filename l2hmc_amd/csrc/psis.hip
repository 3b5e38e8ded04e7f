// l2hmc_psis_smooth -- Pareto-smoothed importance sampling (PSIS; Vehtari, Simpson, Gelman, Yao, Gabry 2024) of the tails of
// any log importance ratios, float64 throughout: the generalised-Pareto fit of Zhang & Stephens (2009) with the prior of the
// `loo` package, the smoothed tail weights and the two logsumexps a caller needs to finish an importance-weighted mean.  It is
// the arithmetic of l2hmc_amd/_pareto.py `_psis_rows`, formula for formula (nothing is folded into an equivalent form: the
// host references compute these expressions, and the tests hold the kernel to them).  Per row i, with L = n_tail[i] <= M live
// slots of lam (descending), lam_c = lam_cutoff[i]:
//     lam_max = lam[0] (lam_c when L = 0),  floor_c = e^(lam_c - lam_max),  x_s = e^(lam_s - lam_max) - floor_c
//     L >= 5:  theta_j = 1 / x_0 + (1 - sqrt(m / (j - 0.5))) / (3 x_star),  j = 1 .. m = 30 + floor(sqrt L),
//              x_star = x of ascending rank floor(L / 4 + 0.5);   k_j = (sum_s log1p(-theta_j x_s)) / L;
//              ell_j = L (log(-theta_j / k_j) - k_j - 1);  w_j = e^(ell_j - logsumexp ell);  theta_hat = sum_j theta_j w_j;
//              k = (sum_s log1p(-theta_hat x_s)) / L;  sigma = -k / theta_hat;  k <- (k L + 5) / (L + 10)
//     smooth = L >= 5 and k, sigma finite:  omega_s = min(log(q_s + floor_c), 0),  q_s the GPD quantile at p = (j - 0.5) / L with
//              j = L - s the ascending rank (k == 0: -sigma log1p(-p); else sigma expm1(-k log1p(-p)) / k);  khat = k
//     otherwise omega_s = lam_s - lam_max and khat = +inf
//     out = khat | lse_w = logsumexp_s omega_s | lse_wl = logsumexp_s (omega_s - lam_s)      (-inf, -inf when L = 0)
// A NaN among the live slots reaches both logsumexps by the arithmetic itself (a maximum here propagates NaN as numpy's does),
// and khat is then NaN too; no other row sees it.
//
// Three kernels, one plan (`psis_plan`; l2hmc_psis_plan reports it) with no branch by L or M:
//   prep     psis_prep_kernel: x_s of every live slot into the workspace, one thread per slot (grid-stride).
//   profile  psis_profile_kernel: the (row, theta) profile is n_rows x m independent sums over L terms, bound by the software
//            log1p.  A workgroup of 256 threads takes one row and kPsisTB = 8 consecutive theta: a thread loads x_s once
//            (s = thread, thread + 256, ...), and adds log1p(-theta_b x_s) to 8 accumulators held in registers; x is read
//            m / 8 times from L2 and never staged through LDS.  The grid runs over (row, theta block), so eight rows of a
//            21 467-slot tail are 8 x 22 workgroups, not 8.  Rows beyond the grid's row count are taken in a loop.
//   finish   psis_finish_kernel: one workgroup per row turns the profile into theta_hat, takes the one remaining mean at
//            theta_hat, smooths, and forms the two logsumexps (omega is computed twice -- once for the maxima and the optional
//            `weights`, once for the sums -- rather than read back, so `out` does not depend on whether weights were asked for).
// Every sum is added in an order that depends on L alone: the thread's own slots s = t, t + 256, ... in that order, then the
// 64 lanes of a wave by an xor butterfly (offsets 32, 16, 8, 4, 2, 1: every lane ends with the same bits), then the four
// waves' partials in wave order.  No floating-point atomics (the only atomic is the integer OR of the error word), so two
// calls give identical bits and a row gives the same bits whichever other rows share the call.
//
// Occupancy by design: the profile kernel, where the time goes, and the prep kernel run 4 waves per SIMD (4 workgroups of 256
// threads per CU): at most 128 registers.  The finish kernel -- one workgroup per row, a few per cent of the work, the whole
// fit's state live at once -- runs 2 waves per SIMD: at most 256 registers.  No kernel uses scratch, and none more than 1 KiB
// of LDS (the four waves' partials); tests/test_psis_cpu.py holds all of that from the compiler's listing.
#include <math.h>

#include "l2hmc_kernels.hpp"

namespace l2hmc {

constexpr int kPsisThreads = 256;            // 4 waves
constexpr int kPsisTB = 8;                   // theta accumulators a thread carries
constexpr long long kPsisMaxGridRows = 65536;   // workgroups along the rows at most; further rows are taken in a loop
constexpr long long kPsisMaxBlocks = 1LL << 23;  // workgroups of one launch at most (x 256 threads stays below 2^32)
constexpr int kPsisMinFit = 5;

struct PsisPlan {
  long long n_theta, theta_blocks, grid_rows;
};

static long long psis_isqrt(long long v) {
  long long r = (long long)floor(sqrt((double)v));
  while (r > 0 && r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

static bool psis_plan(const char* who, int64_t n_rows, int64_t tail_len, PsisPlan& p) {
  if (n_rows < 1) { fail(L2HMC_ERR_ARG, "%s: n_rows >= 1 (got %lld)", who, n_rows); return false; }
  if (tail_len < 0) { fail(L2HMC_ERR_ARG, "%s: tail_len >= 0 (got %lld)", who, tail_len); return false; }
  if (n_rows > (1LL << 31) || (tail_len > 0 && n_rows > (1LL << 31) / tail_len)) {
    fail(L2HMC_ERR_ARG, "%s: tail too large (tail_len n_rows > 2^31): fewer rows per call", who);
    return false;
  }
  p.n_theta = 30 + psis_isqrt(tail_len > 1 ? tail_len : 1);
  p.theta_blocks = (p.n_theta + kPsisTB - 1) / kPsisTB;
  long long cap = kPsisMaxBlocks / p.theta_blocks;
  if (cap > kPsisMaxGridRows) cap = kPsisMaxGridRows;
  p.grid_rows = n_rows < cap ? n_rows : cap;
  return true;
}

// workspace: error word (8 B) | x (n_rows, M) | profile sums (n_rows, n_theta)
struct PsisWorkspace {
  unsigned long long* err;
  double* x;
  double* prof;
  int64_t bytes;
};

static PsisWorkspace psis_workspace(void* base, const PsisPlan& p, int64_t n_rows, int64_t M) {
  PsisWorkspace w;
  Carve c{(char*)base};
  w.err = c.take<unsigned long long>(1);
  w.x = c.take<double>(n_rows * M);
  w.prof = c.take<double>(n_rows * p.n_theta);
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ long long psis_live(const long long* __restrict__ n_tail, long long row, long long M) {
  const long long L = n_tail[row];
  return L < 0 ? 0 : L > M ? M : L;
}

__device__ __forceinline__ double psis_lam_max(const double* __restrict__ lam, const double* __restrict__ lam_c, long long row,
                                               long long M, long long L) {
  return L > 0 ? lam[row * M] : lam_c[row];
}

// the sum of one value per thread over the workgroup, in a fixed tree; every thread gets the same bits.  `red`: 4 doubles
__device__ __forceinline__ double psis_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();                                        // (the previous reduction's readers are done with `red`)
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the maximum likewise (fmax: exact, order-free; a NaN is reported by the caller's own flag)
__device__ __forceinline__ double psis_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__device__ __forceinline__ bool psis_block_any(bool v) { return __syncthreads_or(v ? 1 : 0) != 0; }

// the centre of a logsumexp whose maximum is mx: 0 for an empty (-inf) or +inf row, NaN stays
__device__ __forceinline__ double psis_centre(double mx) { return isfinite(mx) ? mx : (mx != mx ? mx : 0.0); }

__device__ __forceinline__ double psis_theta(double x_top, double x_star, double m_theta, long long j) {
  return 1.0 / x_top + (1.0 - sqrt(m_theta / ((double)j - 0.5))) / (3.0 * x_star);
}

__global__ __launch_bounds__(kPsisThreads) void psis_prep_kernel(const double* __restrict__ lam,
                                                                 const long long* __restrict__ n_tail,
                                                                 const double* __restrict__ lam_c, long long n_rows, long long M,
                                                                 double* __restrict__ x) {
  const long long cells = n_rows * M, stride = (long long)gridDim.x * kPsisThreads;
  for (long long i = (long long)blockIdx.x * kPsisThreads + threadIdx.x; i < cells; i += stride) {
    const long long row = i / M, s = i - row * M;
    const long long L = psis_live(n_tail, row, M);
    if (s >= L) continue;                                  // a dead slot is never read
    const double lmax = lam[row * M];
    x[i] = exp(lam[i] - lmax) - exp(lam_c[row] - lmax);
  }
}

// prof[row][j - 1] = sum_s log1p(-theta_j x_s); blockIdx.x = grid row * theta_blocks + theta block
__global__ __launch_bounds__(kPsisThreads) void psis_profile_kernel(const double* __restrict__ x,
                                                                    const long long* __restrict__ n_tail, long long n_rows,
                                                                    long long M, long long n_theta, long long theta_blocks,
                                                                    long long grid_rows, double* __restrict__ prof) {
  __shared__ double red[4][kPsisTB];
  const long long tb = (long long)blockIdx.x % theta_blocks;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long row = (long long)blockIdx.x / theta_blocks; row < n_rows; row += grid_rows) {   // (uniform over the workgroup)
    const long long L = psis_live(n_tail, row, M);
    if (L < kPsisMinFit) continue;
    const double m_theta = 30.0 + floor(sqrt((double)L));
    const long long j0 = tb * kPsisTB + 1;                 // this block's first theta, 1-based
    if ((double)j0 > m_theta) continue;
    const double* xr = x + row * M;
    long long at = L - (long long)floor((double)L / 4.0 + 0.5);
    at = at < 0 ? 0 : at > M - 1 ? M - 1 : at;
    const double x_top = xr[0], x_star = xr[at];
    double th[kPsisTB], acc[kPsisTB];
#pragma unroll
    for (int b = 0; b < kPsisTB; ++b) {
      th[b] = psis_theta(x_top, x_star, m_theta, j0 + b);
      acc[b] = 0.0;
    }
    for (long long s = threadIdx.x; s < L; s += kPsisThreads) {
      const double xv = xr[s];
#pragma unroll
      for (int b = 0; b < kPsisTB; ++b) acc[b] += log1p(-th[b] * xv);
    }
#pragma unroll
    for (int b = 0; b < kPsisTB; ++b) {
      double v = acc[b];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      acc[b] = v;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < kPsisTB; ++b) red[w][b] = acc[b];
    }
    __syncthreads();
    if (threadIdx.x < kPsisTB && j0 + threadIdx.x <= n_theta) {
      const int b = threadIdx.x;
      prof[row * n_theta + (j0 - 1) + b] = ((red[0][b] + red[1][b]) + red[2][b]) + red[3][b];   // (past m_theta: not read)
    }
  }
}

// omega of slot s
struct PsisRow {
  double lam_max, floor_c, k, sigma, Ld;
  bool smooth;
};

__device__ __forceinline__ double psis_omega(const PsisRow& r, double lam_s, long long L, long long s) {
  if (!r.smooth) return lam_s - r.lam_max;
  const double j = (double)(L - s);
  const double lp = log1p(-((j - 0.5) / r.Ld));
  const double q = r.k == 0.0 ? -r.sigma * lp : r.sigma * expm1(-r.k * lp) / r.k;
  return fmin(log(q + r.floor_c), 0.0);
}

__global__ __launch_bounds__(kPsisThreads) void psis_finish_kernel(const double* __restrict__ lam,
                                                                   const long long* __restrict__ n_tail,
                                                                   const double* __restrict__ lam_c, long long n_rows,
                                                                   long long M, long long n_theta,
                                                                   const double* __restrict__ x, const double* __restrict__ prof,
                                                                   double* __restrict__ out, double* __restrict__ weights,
                                                                   unsigned long long* __restrict__ err) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {     // (uniform over the workgroup)
    const long long raw = n_tail[row];
    if (t == 0 && (raw < 0 || raw > M)) atomicOr(err, 1ull);
    const long long L = psis_live(n_tail, row, M);
    const double* lr = lam + row * M;
    const double* xr = x + row * M;
    PsisRow r;
    r.lam_max = psis_lam_max(lam, lam_c, row, M, L);
    r.floor_c = exp(lam_c[row] - r.lam_max);
    r.Ld = (double)L;
    r.k = r.sigma = nan;
    r.smooth = false;
    if (L >= kPsisMinFit) {
      const double Ld = r.Ld, m_theta = 30.0 + floor(sqrt(Ld));
      const long long m = (long long)m_theta;
      long long at = L - (long long)floor(Ld / 4.0 + 0.5);
      at = at < 0 ? 0 : at > M - 1 ? M - 1 : at;
      const double x_top = xr[0], x_star = xr[at];
      // ell_j on the grid, its logsumexp, theta_hat
      double mx = -inf;
      bool bad = false;
      for (long long j = 1 + t; j <= m; j += kPsisThreads) {
        const double th = psis_theta(x_top, x_star, m_theta, j), kj = prof[row * n_theta + j - 1] / Ld;
        const double ell = Ld * (log(-th / kj) - kj - 1.0);
        bad = bad || ell != ell;
        mx = fmax(mx, ell);
      }
      mx = psis_block_max(mx, red);
      if (psis_block_any(bad)) mx = nan;
      const double centre = psis_centre(mx);
      double se = 0.0;
      for (long long j = 1 + t; j <= m; j += kPsisThreads) {
        const double th = psis_theta(x_top, x_star, m_theta, j), kj = prof[row * n_theta + j - 1] / Ld;
        se += exp(Ld * (log(-th / kj) - kj - 1.0) - centre);
      }
      const double lse_ell = centre + log(psis_block_sum(se, red));
      double st = 0.0;
      for (long long j = 1 + t; j <= m; j += kPsisThreads) {
        const double th = psis_theta(x_top, x_star, m_theta, j), kj = prof[row * n_theta + j - 1] / Ld;
        st += th * exp(Ld * (log(-th / kj) - kj - 1.0) - lse_ell);
      }
      const double theta_hat = psis_block_sum(st, red);
      double sk = 0.0;
      for (long long s = t; s < L; s += kPsisThreads) sk += log1p(-theta_hat * xr[s]);
      double k = psis_block_sum(sk, red) / Ld;
      r.sigma = -k / theta_hat;
      r.k = (k * Ld + 5.0) / (Ld + 10.0);
      r.smooth = isfinite(r.k) && isfinite(r.sigma);
    }
    // pass 1: the maxima of omega and omega - lam (and the weights, in slot order; -inf past L)
    double mw = -inf, mwl = -inf;
    bool bw = false, bwl = false;
    for (long long s = t; s < M; s += kPsisThreads) {
      double om = -inf;
      if (s < L) {
        const double ls = lr[s];
        om = psis_omega(r, ls, L, s);
        const double ol = om - ls;
        bw = bw || om != om;
        bwl = bwl || ol != ol;
        mw = fmax(mw, om);
        mwl = fmax(mwl, ol);
      }
      if (weights) weights[row * M + s] = om;
    }
    mw = psis_block_max(mw, red);
    mwl = psis_block_max(mwl, red);
    if (psis_block_any(bw)) mw = nan;
    if (psis_block_any(bwl)) mwl = nan;
    const double cw = psis_centre(mw), cwl = psis_centre(mwl);
    // pass 2: the sums
    double sw = 0.0, swl = 0.0;
    for (long long s = t; s < L; s += kPsisThreads) {
      const double ls = lr[s];
      const double om = psis_omega(r, ls, L, s);
      sw += exp(om - cw);
      swl += exp((om - ls) - cwl);
    }
    const double lse_w = cw + log(psis_block_sum(sw, red));
    const double lse_wl = cwl + log(psis_block_sum(swl, red));
    if (t == 0) {
      const bool row_nan = lse_w != lse_w || lse_wl != lse_wl;
      out[row] = row_nan ? nan : (r.smooth ? r.k : inf);
      out[n_rows + row] = lse_w;
      out[2 * n_rows + row] = lse_wl;
    }
  }
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_psis_plan(int64_t n_rows, int64_t tail_len, int32_t what) {
  PsisPlan p;
  if (!psis_plan("l2hmc_psis_plan", n_rows, tail_len, p)) return L2HMC_ERR_ARG;
  switch (what) {
    case 0: return p.theta_blocks;
    case 1: return p.grid_rows;
    case 2: return kPsisTB;
    case 3: return kPsisThreads;
    case 4: return p.n_theta;
  }
  return fail(L2HMC_ERR_ARG, "l2hmc_psis_plan: what is 0 .. 4 (got %s%lld)", "", what);
}

int64_t l2hmc_psis_workspace_bytes(int64_t n_rows, int64_t tail_len) {
  PsisPlan p;
  if (!psis_plan("l2hmc_psis_workspace_bytes", n_rows, tail_len, p)) return L2HMC_ERR_ARG;
  return psis_workspace(nullptr, p, n_rows, tail_len).bytes;
}

int l2hmc_psis_smooth(const double* lam, const int64_t* n_tail, const double* lam_cutoff, int64_t n_rows, int64_t tail_len,
                      double* out, double* weights, void* workspace, void* stream) {
  PsisPlan p;
  if (!psis_plan("l2hmc_psis_smooth", n_rows, tail_len, p)) return L2HMC_ERR_ARG;
  if ((!lam && tail_len > 0) || !n_tail || !lam_cutoff || !out || !workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_psis_smooth: lam, n_tail, lam_cutoff, out and workspace are required%s");
  if (((uintptr_t)lam & 7) || ((uintptr_t)n_tail & 7) || ((uintptr_t)lam_cutoff & 7) || ((uintptr_t)out & 7) ||
      ((uintptr_t)weights & 7) || ((uintptr_t)workspace & 7))
    return fail(L2HMC_ERR_ARG, "l2hmc_psis_smooth: lam, n_tail, lam_cutoff, out, weights and workspace must be 8-byte aligned%s");
  hipStream_t s = (hipStream_t)stream;
  const PsisWorkspace ws = psis_workspace(workspace, p, n_rows, tail_len);
  const long long M = tail_len, n = n_rows;
  hipError_t e = hipMemsetAsync(ws.err, 0, 8, s);
  if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
  if (M > 0) {
    long long blocks = (n * M + kPsisThreads - 1) / kPsisThreads;
    if (blocks > kPsisMaxBlocks) blocks = kPsisMaxBlocks;
    hipLaunchKernelGGL(psis_prep_kernel, dim3((unsigned)blocks), dim3(kPsisThreads), 0, s, lam, (const long long*)n_tail,
                       lam_cutoff, n, M, ws.x);
    if (M >= kPsisMinFit)
      hipLaunchKernelGGL(psis_profile_kernel, dim3((unsigned)(p.grid_rows * p.theta_blocks)), dim3(kPsisThreads), 0, s,
                         (const double*)ws.x, (const long long*)n_tail, n, M, p.n_theta, p.theta_blocks, p.grid_rows, ws.prof);
  }
  hipLaunchKernelGGL(psis_finish_kernel, dim3((unsigned)(n < kPsisMaxGridRows ? n : kPsisMaxGridRows)), dim3(kPsisThreads), 0, s,
                     lam, (const long long*)n_tail, lam_cutoff, n, M, p.n_theta, (const double*)ws.x, (const double*)ws.prof, out,
                     weights, ws.err);
  return launched();
}

}  // extern "C"
