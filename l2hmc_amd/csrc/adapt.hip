// l2hmc_adapt_* -- warm-up: the step size eps = exp(alpha) adapted ON THE DEVICE between launches of the sampler loop, by the
// doubling search of Hoffman & Gelman (2014) Alg. 4 and the dual averaging of their Alg. 5, both on the mean accept
// probability over the chains of a window.  Every trajectory kernel reads eps = expf(*alpha) from device memory when it starts,
// so a kernel that rewrites *alpha in place changes the step size of the next launch with no host round trip; include/l2hmc.h
// states the contract and the update rules, l2hmc_amd/warmup.py drives it.
//
//   window <= L2HMC_ADAPT_SINGLE_BLOCK_MAX values: ONE launch of one workgroup of 1024 threads.  Thread t adds, in float64 and
//           in index order, the values t, t + 1024, t + 2048, ... (eight loads in flight, a non-finite value entering as 0);
//           the 1024 sums are folded in LDS by a fixed binary tree (slot i += slot i + w for w = 512, 256, ..., 1); thread 0
//           then runs the scalar update in plain float64 C++ and writes the state, alpha and the trace row.
//   larger: adapt_partial_kernel -- block b sums, the same way, the contiguous chunk b of the window into workspace[b] -- and
//           then the kernel above over the workspace's doubles instead of the window's floats (a kernel boundary orders the two:
//           no in-launch hand-off between workgroups, no counter to clear per call).  Chunks are a multiple of 1024 values and
//           at least 4096, at most 1024 of them.
// No floating-point atomics and no order that depends on the schedule: state, alpha and trace are bitwise reproducible.
#include "l2hmc_kernels.hpp"

namespace l2hmc {

constexpr int kAdThreads = 1024;
constexpr long long kAdMaxBlocks = 1024;
constexpr long long kAdMinChunk = 4096;
constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr double kLn10 = 2.302585092994045684017991454684;

// state slots (include/l2hmc.h)
enum { kSPhase = 0, kSDir, kST, kSLogEps, kSLogEpsBar, kSHBar, kSMu, kSAccept, kSCount, kSTarget, kSGamma, kST0, kSKappa,
       kSLogMin, kSLogMax, kSZero };

// chunk length of the multi-block form (a multiple of the block size: every block's threads walk whole strides)
static long long adapt_chunk(long long n) {
  long long c = (n + kAdMaxBlocks - 1) / kAdMaxBlocks;
  if (c < kAdMinChunk) c = kAdMinChunk;
  return (c + kAdThreads - 1) / kAdThreads * kAdThreads;
}

__device__ __forceinline__ double ad_value(float v) { return __builtin_isfinite(v) ? (double)v : 0.0; }
__device__ __forceinline__ double ad_value(double v) { return v; }

// sum of src[0 .. n) over the workgroup, in the fixed order described at the top; every thread returns the total
template <typename T>
__device__ __forceinline__ double ad_block_sum(const T* __restrict__ src, long long n, double* sm) {
  const int tid = threadIdx.x;
  double s = 0.0;
  long long i = tid;
  for (; i + 7LL * kAdThreads < n; i += 8LL * kAdThreads) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + (long long)u * kAdThreads];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += ad_value(v[u]);
  }
  for (; i < n; i += kAdThreads) s += ad_value(src[i]);
  sm[tid] = s;
  __syncthreads();
  for (int w = kAdThreads / 2; w > 0; w >>= 1) {
    if (tid < w) sm[tid] += sm[tid + w];
    __syncthreads();
  }
  return sm[0];
}

__global__ __launch_bounds__(kAdThreads) void adapt_partial_kernel(const float* __restrict__ p, long long n, long long chunk,
                                                                   double* __restrict__ part) {
  __shared__ double sm[kAdThreads];
  const long long lo = (long long)blockIdx.x * chunk;
  const long long len = n - lo < chunk ? n - lo : chunk;
  const double s = ad_block_sum(p + lo, len, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__device__ __forceinline__ double ad_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void ad_start_averaging(double* st, double log_eps) {
  st[kSPhase] = 1.0;
  st[kSMu] = log_eps + kLn10;
  st[kST] = 0.0;
  st[kSHBar] = 0.0;
  st[kSLogEpsBar] = 0.0;
}

// the scalar update of include/l2hmc.h, one thread, float64
__device__ void ad_apply(double a, double* st, float* alpha, double* trace) {
  const int phase = (int)st[kSPhase];
  const double lo = st[kSLogMin], hi = st[kSLogMax];
  const double ran = st[kSLogEps];
  double log_eps = ran;
  if (phase == 0) {
    const double d = a > 0.5 ? 1.0 : -1.0;
    double dir = st[kSDir];
    if (dir == 0.0) st[kSDir] = dir = d;
    if (d == dir) {
      const double stepped = log_eps + dir * kLn2;
      log_eps = ad_clamp(stepped, lo, hi);
      if (log_eps != stepped) ad_start_averaging(st, log_eps);       // a clamp that binds ends the search
    } else {
      ad_start_averaging(st, log_eps);                               // crossed: the next window runs at the same step size
    }
  } else if (phase == 1) {
    const double t = st[kST] + 1.0;
    const double w = 1.0 / (t + st[kST0]);
    const double hbar = (1.0 - w) * st[kSHBar] + w * (st[kSTarget] - a);
    log_eps = ad_clamp(st[kSMu] - sqrt(t) / st[kSGamma] * hbar, lo, hi);
    const double e = pow(t, -st[kSKappa]);
    st[kSLogEpsBar] = e * log_eps + (1.0 - e) * st[kSLogEpsBar];
    st[kST] = t;
    st[kSHBar] = hbar;
  }
  st[kSLogEps] = log_eps;
  st[kSAccept] = a;
  st[kSCount] += 1.0;
  *alpha = (float)log_eps;
  if (trace) {
    trace[0] = a;
    trace[1] = ran;
    trace[2] = log_eps;
    trace[3] = st[kSPhase];
  }
}

// T = float: the window itself; T = double: the blocks' partial sums of it (n_src of them; n stays the window's length)
template <typename T>
__global__ __launch_bounds__(kAdThreads) void adapt_update_kernel(const T* __restrict__ src, long long n_src, long long n,
                                                                  int mode, double* sums2, double* state, float* alpha,
                                                                  double* trace) {
  __shared__ double sm[kAdThreads];
  double sum = 0.0, cnt = 0.0;
  if (mode & L2HMC_ADAPT_REDUCE) {
    sum = ad_block_sum(src, n_src, sm);
    cnt = (double)n;
  }
  if (threadIdx.x != 0) return;
  if (mode & L2HMC_ADAPT_REDUCE) {
    if (sums2) { sums2[0] = sum; sums2[1] = cnt; }
  } else {
    sum = sums2[0];
    cnt = sums2[1];
  }
  if (mode & L2HMC_ADAPT_APPLY) ad_apply(sum / cnt, state, alpha, trace);
}

__global__ void adapt_init_kernel(double* st, const float* alpha, int search, double target, double gamma, double t0,
                                  double kappa, double lo, double hi) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double log_eps = (double)*alpha;
  st[kSPhase] = search ? 0.0 : 1.0;
  st[kSDir] = 0.0;
  st[kST] = 0.0;
  st[kSLogEps] = log_eps;
  st[kSLogEpsBar] = 0.0;
  st[kSHBar] = 0.0;
  st[kSMu] = search ? 0.0 : log_eps + kLn10;
  st[kSAccept] = 0.0;
  st[kSCount] = 0.0;
  st[kSTarget] = target;
  st[kSGamma] = gamma;
  st[kST0] = t0;
  st[kSKappa] = kappa;
  st[kSLogMin] = lo;
  st[kSLogMax] = hi;
  st[kSZero] = 0.0;
}

__global__ void adapt_finish_kernel(double* st, float* alpha) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st[kST] >= 1.0) st[kSLogEps] = st[kSLogEpsBar];
  st[kSPhase] = 2.0;
  *alpha = (float)st[kSLogEps];
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_adapt_workspace_doubles(int64_t n) {
  if (n < 1) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_workspace_doubles: n must be >= 1 (got %s%lld)", "", n);
  if (n <= L2HMC_ADAPT_SINGLE_BLOCK_MAX) return 0;
  const long long chunk = adapt_chunk(n);
  return (n + chunk - 1) / chunk;
}

int l2hmc_adapt_init(double* state, const float* alpha, int32_t search, double target_accept, double gamma, double t0,
                     double kappa, double log_eps_min, double log_eps_max, void* stream) {
  if (!state || !alpha) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_init: state and alpha are required%s");
  if (search != 0 && search != 1) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_init: search must be 0 or 1 (got %s%lld)", "", search);
  if (!(target_accept > 0.0 && target_accept < 1.0))
    return fail(L2HMC_ERR_ARG, "l2hmc_adapt_init: target_accept must lie in (0, 1)%s");
  if (!(gamma > 0.0) || !(t0 > 0.0) || !(kappa > 0.0))
    return fail(L2HMC_ERR_ARG, "l2hmc_adapt_init: gamma, t0 and kappa must be positive%s");
  if (!(log_eps_min < log_eps_max)) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_init: log_eps_min must be below log_eps_max%s");
  hipLaunchKernelGGL(adapt_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, alpha, (int)search, target_accept,
                     gamma, t0, kappa, log_eps_min, log_eps_max);
  return launched();
}

int l2hmc_adapt_update(const float* p, int64_t n, int32_t mode, double* sums2, double* state, float* alpha, double* trace_row4,
                       double* workspace, void* stream) {
  if (mode < 1 || mode > 3) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: mode must be 1 (reduce), 2 (apply) or 3 (got %s%lld)", "", mode);
  const bool reduce = mode & L2HMC_ADAPT_REDUCE, apply = mode & L2HMC_ADAPT_APPLY;
  if (reduce && !p) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: p is required to reduce%s");
  if (reduce && n < 1) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: n must be >= 1 (got %s%lld)", "", n);
  if (mode != 3 && !sums2) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: sums2 is required when mode is not 3%s");
  if (apply && (!state || !alpha)) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: state and alpha are required to apply%s");
  hipStream_t s = (hipStream_t)stream;
  if (reduce && n > L2HMC_ADAPT_SINGLE_BLOCK_MAX) {
    if (!workspace)
      return fail(L2HMC_ERR_ARG, "l2hmc_adapt_update: workspace is required for n > %s%lld", "", (long long)L2HMC_ADAPT_SINGLE_BLOCK_MAX);
    const long long chunk = adapt_chunk(n), nb = (n + chunk - 1) / chunk;
    hipLaunchKernelGGL(adapt_partial_kernel, dim3((unsigned)nb), dim3(kAdThreads), 0, s, p, (long long)n, chunk, workspace);
    hipLaunchKernelGGL(adapt_update_kernel<double>, dim3(1), dim3(kAdThreads), 0, s, (const double*)workspace, nb, (long long)n,
                       (int)mode, sums2, state, alpha, trace_row4);
  } else {
    hipLaunchKernelGGL(adapt_update_kernel<float>, dim3(1), dim3(reduce ? kAdThreads : 64), 0, s, p, (long long)n, (long long)n,
                       (int)mode, sums2, state, alpha, trace_row4);
  }
  return launched();
}

int l2hmc_adapt_finish(double* state, float* alpha, void* stream) {
  if (!state || !alpha) return fail(L2HMC_ERR_ARG, "l2hmc_adapt_finish: state and alpha are required%s");
  hipLaunchKernelGGL(adapt_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, alpha);
  return launched();
}

}  // extern "C"
