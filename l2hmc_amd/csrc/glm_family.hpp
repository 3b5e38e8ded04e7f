// The likelihoods of the draw-tile statistics kernels, each stated once: PoissonLog, BinomialLogit, NegBinomialLog and
// ProbitBinomial for every kernel of glm.hip, and BernoulliLogit (at the end) for the logistic kernels of predictive.hip, loo.hip and lik_stats.hip.  For
// glm.hip a family is a struct with
//     kConsts            the number of per-row constants ll takes: 2 (row_consts[0], row_consts[1]) or 3 (and row_consts[3];
//                        row_consts[2] is sat for every family, which only the predictive sums read)
//     ll(eta, y, a, b[, c])   the pointwise log-likelihood of a row with response y under the linear predictor eta = x_i . w_s
//     mean(eta, a[, b])  the predictive mean
// and an ABI number (include/l2hmc.h L2HMC_GLM_*).  The kernels call them through family_ll / family_mean below.  A further
// family (another link) is one more struct here, one more case in glm.hip's dispatch and a unit that instantiates its launches
// (as glm_probit.hip does for ProbitBinomial), not another copy of three kernels.
//
// THE INVARIANT THE SELECT AND THE GATHER OF glm.hip RELY ON: every kernel -- the matrix writer, the four count passes, the
// gather, the predictive sums -- computes ll by ONE device function, Family::ll, from the eta that tile_logits of draw_tiles.hpp
// returns and from nothing else.  The function is a fixed sequence of correctly rounded float32 operations spelled out one by
// one (__fadd_rn, fmaf, __fsub_rn and the hardware exp2 of fexp) under `fp contract(off)`: there is no bare `y * h - mu` that
// the compiler could contract into a fused multiply-add in one instantiation and not in another.  The bits of ll_si therefore
// depend on (W, X, y, row constants) alone -- not on the pass, the chunk, the kernel or the row grouping of the caller.  A key
// counted in one launch is the key compared in the next, and l2hmc_glm_log_lik writes the very float32 values the fused
// kernels select among (tests/test_gpu_glm.py holds the fused tails against the written matrix bit for bit).
#pragma once
#include "l2hmc_kernels.hpp"

namespace l2hmc {

// Poisson regression with the log link and an offset (log exposure) o_i:
//     h = eta + o_i    mu = exp(h)    ll = y_i h - mu - g_i,   g_i = lgamma(y_i + 1) (float64 on the host, rounded once)
// Four roundings: the sum h, the product h log2(e) inside fexp (then the hardware exp2), the fused y h - mu, the difference.
// The family's second statement is PoissonLink in l2hmc_kernels.hpp (the ENERGY of the fused sampling target, L2HMC_ENERGY_POISSON):
// it forms h and mu by these same two operations, so a trajectory moves on the mu these statistics evaluate.  Change both or neither.
struct PoissonLog {
  static constexpr int kAbi = 1;          // L2HMC_GLM_POISSON
  static constexpr int kConsts = 2;       // ll reads the offset and g
  static __device__ __forceinline__ float ll(float eta, float y, float o, float g) {
#pragma clang fp contract(off)
    const float h = __fadd_rn(eta, o);
    const float mu = fexp(h);
    return __fsub_rn(fmaf(y, h, -mu), g);
  }
  static __device__ __forceinline__ float mean(float eta, float o) {
#pragma clang fp contract(off)
    return fexp(__fadd_rn(eta, o));
  }
};

// Binomial regression with m_i trials and the logit link, and NB2 negative-binomial regression with fixed dispersion phi: ONE
// log-likelihood with a per-row offset o_i, weight m_i and constant c_i (include/l2hmc.h says what each family puts there),
//     t = eta + o_i    ll = y_i t - m_i softplus(t) + c_i
// formed by BinomialLink of l2hmc_kernels.hpp -- the struct the fused sampling target (L2HMC_ENERGY_BINOMIAL) moves on -- so
// there is one statement of the operations, not two to keep alike.  The families differ in the predictive mean only:
// m sigmoid(t) for the binomial; exp(t) = mu / phi for the negative binomial (the host multiplies the sum by phi).
struct BinomialLogit {
  static constexpr int kAbi = 3;          // L2HMC_GLM_BINOMIAL
  static constexpr int kConsts = 3;       // ll reads the offset, the weight and c
  static __device__ __forceinline__ float ll(float eta, float y, float o, float m, float c) { return BinomialLink(eta, y, o, m).ll(c); }
  static __device__ __forceinline__ float mean(float eta, float o, float m) {
#pragma clang fp contract(off)
    return __fmul_rn(m, BinomialLink(eta, 0.f, o, m).sigmoid());
  }
};
struct NegBinomialLog {
  static constexpr int kAbi = 4;          // L2HMC_GLM_NEGBINOMIAL
  static constexpr int kConsts = 3;
  static __device__ __forceinline__ float ll(float eta, float y, float o, float m, float c) { return BinomialLogit::ll(eta, y, o, m, c); }
  static __device__ __forceinline__ float mean(float eta, float o, float m) { return fexp(BinomialLink(eta, 0.f, o, m).t); }
};

// Binomial regression with m_i trials and the PROBIT link: with t = eta + o_i,
//     ll = y_i log Phi(t) + (m_i - y_i) log Phi(-t) + c_i,   c_i = log C(m_i, y_i),   mean m_i Phi(t)
// formed by ProbitLink of l2hmc_kernels.hpp -- the struct the fused sampling target (L2HMC_ENERGY_PROBIT) moves on: one statement
// of the operations (log Phi exact in both tails).  The row constants are the binomial's (4, n): [o, m, sat, c].
struct ProbitBinomial {
  static constexpr int kAbi = 6;          // L2HMC_GLM_PROBIT
  static constexpr int kConsts = 3;       // ll reads the offset, the trials and c
  static __device__ __forceinline__ float ll(float eta, float y, float o, float m, float c) { return ProbitLink(eta, y, o, m).ll(c); }
  static __device__ __forceinline__ float mean(float eta, float o, float m) {
#pragma clang fp contract(off)
    return __fmul_rn(m, ProbitLink(eta, 0.f, o, m).Phi());
  }
};

// what the kernels of glm.hip call: the family's ll and mean with as many constants as it declares (k2 is row_consts[3])
template <typename F>
__device__ __forceinline__ float family_ll(float eta, float y, float k0, float k1, [[maybe_unused]] float k2) {
  if constexpr (F::kConsts == 3) return F::ll(eta, y, k0, k1, k2);
  else return F::ll(eta, y, k0, k1);
}
template <typename F>
__device__ __forceinline__ float family_mean(float eta, float k0, [[maybe_unused]] float k1) {
  if constexpr (F::kConsts == 3) return F::mean(eta, k0, k1);
  else return F::mean(eta, k0);
}

// Logistic regression, the link of the logistic history statistics (predictive.hip, loo.hip, lik_stats.hip -- NOT a family of
// glm.hip: their keys are the signed logit t, not ll, and their sums are float32 terms, a different and faster contract):
//     t = (2 y_i - 1) eta    e = exp(-|t|)    lik = sigmoid(t) = 1 / (1 + e) for t >= 0, e / (1 + e) below
// THE SAME INVARIANT: the tail gather of loo.hip and the series of lik_stats.hip (`relative_eff` feeds `loo(r_eff="auto")`) form
// the likelihood by ONE device function, lik, and every kernel the signed logit by signed_logit (the sign is exact); `sums`
// forms what predict_kernel needs from one e and one reciprocal by the same operations.  Each value is one expression, as it
// stands: the units compile with the default contraction, so splitting one changes bits.  Change all callers or none.
struct BernoulliLogit {
  static __device__ __forceinline__ float signed_logit(float eta, float y) { return y > 0.5f ? eta : -eta; }
  static __device__ __forceinline__ float lik(float t) {
    const float e = fexp(-fabsf(t));
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    return t >= 0.f ? inv : e * inv;
  }
  // p1 = sigmoid(eta), lik = sigmoid(z) and ll = log lik = min(z, 0) - log(1 + e) of z = signed_logit(eta, y): |z| = |eta|
  static __device__ __forceinline__ void sums(float eta, float y, float& p1, float& lik, float& ll) {
    const float e = fexp(-fabsf(eta));
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float lo = e * inv;
    const float z = signed_logit(eta, y);
    p1 = eta >= 0.f ? inv : lo;
    lik = z >= 0.f ? inv : lo;
    ll = fminf(z, 0.f) - 0.6931471805599453f * __builtin_amdgcn_logf(1.f + e);
  }
};

}  // namespace l2hmc
