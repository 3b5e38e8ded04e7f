// l2hmc_loglik_tails -- the per-column raw material of Pareto-smoothed importance sampling (PSIS-LOO of ANY likelihood) of a
// pointwise log-likelihood matrix ll (n_draws, n_cols), float32, row-major, read where it lies.  The log importance ratio of
// column i under draw s is -ll: the largest ratios are the smallest ll.  Per column, with its own tail length M_i:
//     cutoff   c = the element of ascending rank M_i   (the total order of radix_key: -0 before +0, every NaN last)
//     top      the element of rank n_draws - 1, the column's maximum (NaN when the column holds a NaN)
//     tail     the ll strictly before c in that order, L_i <= M_i of them in any order, with the draw each came from in
//              tail_pos; the slots at or past L_i hold +inf and -1
//     sums     [0] body    = the sum over the draws NOT in the tail of e^(c - ll)        (every term in (0, 1])
//              [1] body_sq = the same sum of e^(2 (c - ll))
//              [2] lik     = the sum over ALL draws of e^(ll - top)                      (every term in (0, 1])
// l2hmc_amd/psis.py (`loo_from_log_lik(select="fused")`, `psis(select="fused")`) finishes them on the float64 Pareto kernels of
// psis.hip; include/l2hmc.h states the contract.
//
//   init     loglik_init_kernel: the two ranks of every column (M_i, clamped to 0 .. tail_stride, and n_draws - 1) for the
//            select, n_tail = 0, the tail's pads, the error word.
//   select   l2hmc_order_stats (order_stats.hip) with two ranks per column: its count / advance passes as they are -- this
//            unit has no select of its own.
//   gather   loglik_gather_kernel, one more read of the matrix.  The draws are cut into SEGMENTS of `rows` consecutive draws,
//            rows = max(64, ceil(n_draws / 2048)): a function of n_draws alone.  A thread owns one (segment, column) pair --
//            thread t of the grid <-> (t / n_cols, t % n_cols), so a wave reads runs of consecutive floats of a row -- and walks
//            its segment's draws in ascending order: a key strictly below the cutoff's takes slot atomicAdd(n_tail[i], 1) (an
//            integer atomic) of the column's tail; a slot at or past M_i is not written and raises the error word of the
//            workspace (it cannot happen: the select and the gather compare the same keys).  Every term is formed in float64
//            from the exact float32 values -- (double) c - (double) ll, then `exp` in double, one call per term -- and added
//            to the thread's own three float64 sums, which go to workspace part[segment][3][n_cols].
//   reduce   chunk_reduce_kernel (draw_tiles.hpp): sums[k][i] = the segments' partials added in segment order.
// No floating-point atomics.  The order in which a column's terms are added depends on n_draws alone: a column gives the same
// bits whichever other columns share the call, and wherever it stands among them.  Every outward write is an ordinary vector
// store or an integer atomic from plain C++.
//
// A column whose cutoff is not finite (the rule: the finished numbers equal those of the `torch.topk` route of psis.py where
// that route is finite, and are NaN or +-inf where it is):
//     c = -inf  (more than M_i draws at -inf)  the tail is empty; a draw at -inf gives c - ll = NaN: body = body_sq = NaN
//     c = +inf  (rank M_i is +inf)             the tail holds every finite draw below it; body terms are e^(inf - inf) = NaN
//     c = NaN   (fewer than M_i + 1 numbers)   the tail holds every number of the column; body = body_sq = lik = NaN
// and top = +inf makes lik 0 or NaN, top = -inf (every draw -inf) makes it NaN.  The caller's finish turns each into NaN or
// +-inf; nothing is hidden.
//
// DESIGNED FOR THE FLOAT64 ISSUE BOUND, not the memory bound.  Per element the pass reads 4 bytes and evaluates up to three
// double-precision `exp` (a tail member needs lik alone), each some 40 float64 instructions at 16 float64 lanes per SIMD and
// clock: measured on one MI355X the pass takes 8 to 12 times a plain read of the same matrix (0.88 ms against 0.11 ms at
// 409 600 x 256: about 3.6e11 exp per second; profiles/loglik_bench.txt), so the loads (four draws in flight per thread, four
// or more waves per SIMD) hide behind the arithmetic and more memory-level parallelism would buy nothing.  A cheaper pass would
// form e^(2 (c - ll)) as a square and lik as a quotient; both cost a rounding the contract's per-term bound has no room for.
// THE LIMIT OF THAT: the grid is segments x n_cols threads with at most 2048 segments, so only a wide matrix fills the device.
// 256 columns give 524 288 threads (eight waves per SIMD of 256 CUs); 32 columns give 65 536, about one wave per SIMD, and the
// pass then waits on its own loads as well -- measured 11.5 x the plain read at 4 096 000 x 32 against 7.9 x at 409 600 x 256;
// one column gives 2048 threads whose loads are `rows` floats apart and do not coalesce.  Narrow matrices are served
// correctly, not fast; more segments for them (the order of the sums must stay a function of n_draws alone) is not built.
// Occupancy by design: at most 128 registers and no scratch (tests/test_loglik_cpu.py holds both from the compiler's
// listing), no LDS: four workgroups of 256 threads per CU, four waves per SIMD.
#include <math.h>

#include "draw_tiles.hpp"
#include "radix_select.hpp"

namespace l2hmc {

constexpr int kLtThreads = 256;
constexpr int kLtMaxCols = 512;            // l2hmc_order_stats: d <= 512

struct LoglikPlan {
  long long rows, nseg;                    // draws per segment (a function of n_draws alone), segments
};

static bool loglik_plan(const char* who, int64_t n_draws, int32_t n_cols, LoglikPlan& p) {
  if (n_draws < 2) { fail(L2HMC_ERR_ARG, "%s: n_draws >= 2 (got %lld)", who, (long long)n_draws); return false; }
  if (n_cols < 1 || n_cols > kLtMaxCols) { fail(L2HMC_ERR_ARG, "%s: 1 <= n_cols <= 512 (got %lld)", who, (long long)n_cols); return false; }
  if (n_draws > (1LL << 40) / n_cols) { fail(L2HMC_ERR_ARG, "%s: matrix too large (n_draws n_cols > 2^40)", who); return false; }
  draw_segments(n_draws, p.rows, p.nseg);
  return true;
}

// workspace: error word (8 B) | pad (8 B) | ranks (2, n) int64 | n_nan (n) int64 | values (2, n) float32 | pad to 16 B |
//            the workspace of l2hmc_order_stats(n, 2) (a multiple of 16 B) | partials (nseg, 3, n) float64
struct LoglikWorkspace {
  unsigned long long* err;
  long long* ranks;
  long long* n_nan;
  float* values;
  void* select;
  double* part;
  int64_t bytes;
};

static LoglikWorkspace loglik_workspace(void* base, const LoglikPlan& p, int32_t n) {
  LoglikWorkspace w;
  Carve c{(char*)base};
  w.err = c.take<unsigned long long>(2);                     // (the word and its pad)
  w.ranks = c.take<long long>(2 * (int64_t)n);
  w.n_nan = c.take<long long>(n);
  w.values = c.take<float>(((int64_t)n * 2 + 3) / 4 * 4);    // (2, n), its length padded to 16 B
  c.pad(16);
  w.select = c.take<char>(l2hmc_order_stats_workspace_bytes(n, 2));
  w.part = c.take<double>(p.nseg * 3 * (int64_t)n);
  w.bytes = c.off;
  return w;
}

__global__ void loglik_init_kernel(long long* __restrict__ ranks, unsigned long long* __restrict__ n_tail,
                                   float* __restrict__ tail, long long* __restrict__ tail_pos, int n, long long S,
                                   long long stride, long long M, const long long* __restrict__ len_col,
                                   unsigned long long* __restrict__ err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *err = 0ull;
  if (i < n) {
    long long rank = len_col ? len_col[i] : M;               // (a length outside 0 .. tail_stride is clamped: the tail has that many slots)
    rank = rank < 0 ? 0 : rank > stride ? stride : rank;
    ranks[i] = rank; ranks[n + i] = S - 1; n_tail[i] = 0ull;
  }
  if (i < (long long)n * stride) {
    tail[i] = __builtin_inff();
    if (tail_pos) tail_pos[i] = -1ll;
  }
}

__global__ __launch_bounds__(kLtThreads) void loglik_gather_kernel(const float* __restrict__ ll, long long S, int n, long long rows,
                                                                   long long nseg, const float* __restrict__ values,
                                                                   const long long* __restrict__ ranks, long long stride,
                                                                   float* __restrict__ cutoff, float* __restrict__ top,
                                                                   unsigned long long* __restrict__ n_tail,
                                                                   float* __restrict__ tail, long long* __restrict__ tail_pos,
                                                                   unsigned long long* __restrict__ err,
                                                                   double* __restrict__ part) {
  const long long t = (long long)blockIdx.x * kLtThreads + threadIdx.x;
  if (t >= nseg * n) return;
  const long long seg = t / n;
  const int k = (int)(t - seg * n);
  const float c = values[k], tp = values[n + k];
  if (seg == 0) { cutoff[k] = c; top[k] = tp; }
  const uint32_t ckey = radix_key(c);
  const double cd = (double)c, td = (double)tp;
  const unsigned long long room = (unsigned long long)ranks[k];              // clamped to 0 .. stride by the init
  const long long r0 = seg * rows, r1 = r0 + rows < S ? r0 + rows : S;
  const float* p = ll + r0 * n + k;
  double body = 0.0, body_sq = 0.0, lik = 0.0;
  auto term = [&](float v, long long r) {
    const bool in_tail = radix_key(v) < ckey;
    if (in_tail) {
      const unsigned long long slot = atomicAdd(&n_tail[k], 1ull);
      if (slot < room) {
        tail[(long long)k * stride + (long long)slot] = v;
        if (tail_pos) tail_pos[(long long)k * stride + (long long)slot] = r;
      } else {
        atomicOr(err, 1ull);
      }
    }
    const double vd = (double)v, a = cd - vd;
    body += in_tail ? 0.0 : exp(a);
    body_sq += in_tail ? 0.0 : exp(2.0 * a);
    lik += exp(vd - td);
  };
  long long r = r0;
  for (; r + 4 <= r1; r += 4, p += 4 * (long long)n) {       // four independent loads in flight, added in draw order
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = p[u * (long long)n];
#pragma unroll
    for (int u = 0; u < 4; ++u) term(v[u], r + u);
  }
  for (; r < r1; ++r, p += n) term(*p, r);
  double* o = part + seg * 3 * (long long)n + k;
  o[0] = body; o[n] = body_sq; o[2 * (long long)n] = lik;
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_loglik_tails_workspace_bytes(int64_t n_draws, int32_t n_cols) {
  LoglikPlan p;
  if (!loglik_plan("l2hmc_loglik_tails_workspace_bytes", n_draws, n_cols, p)) return L2HMC_ERR_ARG;
  return loglik_workspace(nullptr, p, n_cols).bytes;
}

int l2hmc_loglik_tails(const float* ll, int64_t n_draws, int32_t n_cols, const int64_t* tail_len_col, int64_t tail_stride,
                       float* cutoff, float* top, int64_t* n_tail, float* tail, int64_t* tail_pos, double* sums, void* workspace,
                       void* stream) {
  const char* who = "l2hmc_loglik_tails";
  LoglikPlan p;
  if (!loglik_plan(who, n_draws, n_cols, p)) return L2HMC_ERR_ARG;
  if (tail_stride < 0 || tail_stride >= n_draws) return fail(L2HMC_ERR_ARG, "%s: 0 <= tail_stride < n_draws (got %lld)", who, (long long)tail_stride);
  if (tail_stride * n_cols > (1LL << 31))
    return fail(L2HMC_ERR_ARG, "%s: tail too large (tail_stride n_cols > 2^31): fewer columns per call", who);
  if (!ll || !cutoff || !top || !n_tail || (!tail && tail_stride > 0) || !sums || !workspace)
    return fail(L2HMC_ERR_ARG, "%s: ll, cutoff, top, n_tail, tail, sums and workspace are required", who);
  if (((uintptr_t)ll & 3) || ((uintptr_t)cutoff & 3) || ((uintptr_t)top & 3) || ((uintptr_t)n_tail & 7) || ((uintptr_t)tail & 3) ||
      ((uintptr_t)tail_pos & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 15) || ((uintptr_t)tail_len_col & 7))
    return fail(L2HMC_ERR_ARG, "%s: ll, cutoff, top and tail must be 4-byte, n_tail, tail_pos, tail_len_col and sums 8-byte, "
                               "workspace 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const LoglikWorkspace ws = loglik_workspace(workspace, p, n_cols);
  const long long n = n_cols, cells = n * tail_stride > n ? n * tail_stride : n;
  hipLaunchKernelGGL(loglik_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, ws.ranks,
                     (unsigned long long*)n_tail, tail, (long long*)tail_pos, (int)n_cols, (long long)n_draws,
                     (long long)tail_stride, (long long)l2hmc_logistic_loo_tail_len(n_draws), (const long long*)tail_len_col,
                     ws.err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
  const int rc = l2hmc_order_stats(ll, n_draws, n_cols, (const int64_t*)ws.ranks, 2, ws.values, (int64_t*)ws.n_nan, ws.select,
                                   stream);
  if (rc != L2HMC_OK) return rc;
  const long long threads = p.nseg * n;
  hipLaunchKernelGGL(loglik_gather_kernel, dim3((unsigned)((threads + kLtThreads - 1) / kLtThreads)), dim3(kLtThreads), 0, s, ll,
                     (long long)n_draws, (int)n_cols, p.rows, p.nseg, (const float*)ws.values, (const long long*)ws.ranks,
                     (long long)tail_stride, cutoff, top, (unsigned long long*)n_tail, tail, (long long*)tail_pos, ws.err, ws.part);
  chunk_reduce_launch(ws.part, p.nseg, 3 * n, sums, s);
  return launched();
}

}  // extern "C"
