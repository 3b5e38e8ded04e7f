// l2hmc_glm_log_lik, l2hmc_glm_loo_tails, l2hmc_glm_predict -- model criticism of a generalised linear model (Poisson regression
// with the log link, binomial regression with trials under the logit or the probit link and NB2 negative-binomial regression; glm_family.hpp) over every recorded draw, from a history that stays where the sampler wrote it: the
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
// The kernels and their launches are templates over the family in glm_kernels.hpp; this unit holds the entries, the plans, the
// workspace and the Poisson instantiations, glm_binomial.hip those of the binomial and the negative-binomial family, glm_probit.hip
// those of the probit family.
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
#include "glm_kernels.hpp"

namespace l2hmc {

L2HMC_GLM_LAUNCHES(extern, BinomialLogit)
L2HMC_GLM_PREDICT(extern, BinomialLogit)
L2HMC_GLM_PREDICT(extern, NegBinomialLog)
L2HMC_GLM_LAUNCHES(extern, ProbitBinomial)
L2HMC_GLM_PREDICT(extern, ProbitBinomial)

static bool glm_family_ok(const char* who, int32_t family) {
  if (family != PoissonLog::kAbi && family != BinomialLogit::kAbi && family != NegBinomialLog::kAbi && family != ProbitBinomial::kAbi) {
    fail(L2HMC_ERR_ARG, "%s: unknown family %lld (L2HMC_GLM_POISSON = 1, L2HMC_GLM_BINOMIAL = 3, L2HMC_GLM_NEGBINOMIAL = 4, "
                        "L2HMC_GLM_PROBIT = 6)", who, family);
    return false;
  }
  return true;
}

// f(family struct tag) for a checked family.  LL_ONLY: the kernel uses ll alone, which the negative binomial shares with the
// binomial -- one instantiation serves both.
template <class T> struct family_tag { using type = T; };
template <bool LL_ONLY, class Fn>
static void on_family(int32_t family, Fn&& fn) {
  switch (family) {
    case PoissonLog::kAbi: fn(family_tag<PoissonLog>{}); break;
    case BinomialLogit::kAbi: fn(family_tag<BinomialLogit>{}); break;
    case NegBinomialLog::kAbi: fn(family_tag<std::conditional_t<LL_ONLY, BinomialLogit, NegBinomialLog>>{}); break;
    case ProbitBinomial::kAbi: fn(family_tag<ProbitBinomial>{}); break;
  }
}

// draw_plan (by_draws: the tails; else the matrix and the predictive sums) and the gather's segments
static bool glm_plan(const char* who, int32_t family, int64_t n_draws, int32_t n_data, int32_t d, bool by_draws, GlmPlan& p) {
  if (!glm_family_ok(who, family)) return false;
  if (!draw_plan(who, n_draws, n_data, d, kGlmNB, by_draws, p)) return false;
  draw_segments(n_draws, p.seg_rows, p.nseg);                // (loglik_tails.hip's: the two routes add in one order)
  p.seg_quads = (p.nseg + 3) / 4;
  return true;
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
  on_family<true>(family, [&](auto fam) {
    glm_launch_matrix<typename decltype(fam)::type>(p, s, draws, (long long)n_draws, (int)d, packed, row_consts, (int)n_data, out);
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
  on_family<false>(family, [&](auto fam) {
    glm_launch_predict<typename decltype(fam)::type>(p, s, draws, (long long)n_draws, (int)d, packed, row_consts, (int)n_data, workspace);
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
  const GlmTailArgs targs{ws.prefix, ws.hist, ws.topkey, ws.ranks, top, (unsigned long long*)n_tail, tail, (long long)tail_stride,
                          ws.err, ws.part};
  auto pass = [&](auto mode, int shift, bool first) {
    on_family<true>(family, [&](auto fam) {
      glm_launch_tails<typename decltype(fam)::type, decltype(mode)::value>(p, s, draws, (long long)n_draws, (int)d, packed, row_consts,
                                                                            (int)n_data, shift, first, targs);
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
