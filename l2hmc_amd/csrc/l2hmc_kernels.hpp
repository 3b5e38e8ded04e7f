// l2hmc_kernels.hpp -- device templates of the fused L2HMC leapfrog kernels (gfx950 / CDNA4).
//
// One fused kernel runs a whole trajectory (T generalised leapfrog steps: grad U, VNet,
// momentum half-update, XNet x2 with masked position updates, grad U, VNet, momentum
// half-update, log|det J|) followed by the Metropolis accept probability and MH select.
// Replaces utils/dynamics.py:115-309 and utils/sampler.py:28-55 of the reference.
//
// Mapping:
//   * a workgroup owns a tile of 16 chains; NW waves (1 or 4) split the d dimensions in
//     16-wide tiles, DT tiles per wave;
//   * state layout ("S-layout"): lane l = (c = l & 15, q = l >> 4) holds, for each of its
//     tiles tg, the float4 {z[c][16 tg + 4 q + r]}, r = 0..3 -- which is at the same time
//       - the B operand (k = q) of v_mfma_f32_16x16x4_f32 for k-step r, and
//       - the C/D layout (row = 4 q + r, col = c) of a product whose rows are dimensions.
//     So every layer is computed TRANSPOSED, out^T[unit, chain] = W^T[unit, k] in^T[k, chain]
//     with the weights as the A operand, and activations flow layer to layer with no
//     cross-lane traffic at all;
//   * weights are pre-ordered into A-operand fragments (l2hmc_pack_nets), staged once per
//     workgroup into LDS and read with ds_read_b128 (4 k-steps per read);
//   * biases ride on a constant-1 hidden unit, so there are no bias adds;
//   * per-chain reductions (|v|^2, U, log-det) are per-lane partial sums, reduced once at
//     the end with two wave shuffles (+ one LDS hop when NW = 4);
//   * the energy kind EK is a template parameter: each target gets its own straight-line
//     kernel (compiled in its own translation unit, traj_ek<k>.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "../../include/l2hmc.h"

namespace l2hmc {

typedef float f4 __attribute__((ext_vector_type(4)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// Geometries with DT >= 4 tiles per wave (d > 128 with NW = 4, or the one-wave-per-tile kernels
// for d > 32) read the packed weight / precision fragments straight from global memory (L2-hot,
// prefetched a phase ahead) instead of staging them in LDS: beyond d ~ 190 the two nets no longer
// fit the 160 KiB, and for the NW = 1 kernels a 45 KiB staging buffer per 64-thread workgroup
// would cap the occupancy.
__host__ __device__ constexpr bool weights_in_global(int DT) { return DT >= 4; }

int fail(int code, const char* fmt, const char* a = "", long long b = 0, long long c = 0);
// Rough Well (distributions.py:93): the divisor of the cosine argument.  The reference forms the Python-DOUBLE product
// eps * eps and TF rounds it to float32 once; a binding that holds the double passes that float in L2hmcEnergy.den.  den = 0:
// derived here from the float eta (the exact product of two floats rounded once -- the same value whenever eta is a float).
inline float roughwell_den(const L2hmcEnergy* e) {
  if (e->den > 0.f) return e->den;
  return e->easy ? e->eta : (float)((double)e->eta * (double)e->eta);
}
void note_kernel(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0);   // -> l2hmc_last_kernel
// Adam's host side (l2hmc_adam_step, l2hmc_adam_step_terms, l2hmc_train_step): the hyper-parameters it accepts, and the
// bias-corrected step size lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) (TF1 Adam: epsilon is added to sqrt(v), uncorrected)
inline bool adam_args_ok(float lr, float beta1, float beta2, float epsilon, int64_t step) {
  return step >= 1 && lr >= 0.f && (beta1 >= 0.f && beta1 < 1.f) && (beta2 >= 0.f && beta2 < 1.f) && epsilon > 0.f;
}
inline float adam_lr_t(float lr, float beta1, float beta2, int64_t step) {
  const double t = (double)step;
  return (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t)));
}

// Debug builds with -DL2HMC_LDS_POISON (tools/build_variant_full.sh poison -DL2HMC_LDS_POISON): every kernel that works out of
// dynamic LDS first fills ALL of it with NaN bit patterns.  LDS is not cleared between workgroups, so a kernel that reads a word
// it never staged normally sees whatever the previous workgroup left there -- often plausible numbers, and parity tests pass by
// luck; with the poison such a read turns into NaN and the same tests fail (profiles/r04_lds_poison.txt: the pass of round 4).
// group_segment_size is read from the dispatch packet (hsa_kernel_dispatch_packet_t, byte offset 28).
__device__ __forceinline__ void lds_poison(float* smem) {
#if defined(L2HMC_LDS_POISON) && defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(4))) const unsigned* cptr_t;
  const unsigned total = ((cptr_t)__builtin_amdgcn_dispatch_ptr())[7];
  const unsigned words = (total - __builtin_amdgcn_groupstaticsize()) / 4;
  const unsigned nthr = blockDim.x * blockDim.y * blockDim.z;
  for (unsigned i = threadIdx.x; i < words; i += nthr) reinterpret_cast<unsigned*>(smem)[i] = 0xffffffffu;
  __syncthreads();
#endif
}
int check_energy(const L2hmcEnergy* e, int d);
// what every training entry point answers for L2HMC_ENERGY_POISSON (no kernel holds its Hessian-vector product X^T [mu (X u)])
constexpr const char* kPoissonTrainRefusal =
    "no training kernel for the Poisson-regression target: train on the same likelihood as a caller-supplied energy "
    "(energy_cb / hvp_cb of l2hmc_train_split_grad), then sample with the trained nets on the fused kind%s";
// ... and for L2HMC_ENERGY_BINOMIAL (its Hessian-vector product is X^T [m s (1 - s) (X u)])
constexpr const char* kBinomialTrainRefusal =
    "no training kernel for the binomial / negative-binomial regression target: train on the same likelihood as a caller-supplied "
    "energy (energy_cb / hvp_cb of l2hmc_train_split_grad), then sample with the trained nets on the fused kind%s";
// ... and for L2HMC_ENERGY_PROBIT (its Hessian-vector product is X^T [(y lam(t) (t + lam(t)) + (m - y) lam(-t) (lam(-t) - t)) (X u)])
constexpr const char* kProbitTrainRefusal =
    "no training kernel for the probit-regression target: train on the slow path, the same likelihood as a caller-supplied "
    "energy (energy_cb / hvp_cb of l2hmc_train_split_grad), then load_state_dict the trained nets and sample on the fused kind%s";
int device_cus();      // l2hmc_abi.hip: compute units of the current device (256 when the query fails)
struct KArgs;
// traj_wide.hip: the LDS plan of the LDS-resident-state kernel for d > 256 (elementwise energies) and its waves per workgroup
long long plan_lds_wide(KArgs& k, int& NW);

// ------------------------------------------------------------------------------------------
// Packed layouts (shared by host and device)
// ------------------------------------------------------------------------------------------
// A "group" is 4 A-operand fragments interleaved per lane: element (lane, r) at
// (group * 64 + lane) * 4 + r, so one ds_read_b128 fetches the operands of 4 k-steps.
//
// Hidden units live on D rows 4 q + r with r < KH ("live" rows); unit u <-> (q = u / KH,
// r = u % KH).  Unit H is the constant-1 bias unit.  KH = ceil((H + 1) / 4) k-steps contract
// over the hidden layer.
__host__ __device__ inline int net_groups(int NT) { return 5 * NT + 2; }
__host__ __device__ inline int net_floats(int NT) { return net_groups(NT) * 256 + 32 * NT; }
__host__ __device__ inline int gauss_floats(int NT) { return NT * NT * 256; }
// the same groups as f16x2 fragments (traj_fast.hpp: [64 w_hi | w_hi] then [64 w_lo | w_lo], 16 bytes per lane each; all first
// fragments of a net, then all second ones): what traj_wide_kernel streams from L2 for the elementwise targets
__host__ __device__ inline int net_f16_floats(int NT) { return net_groups(NT) * 512; }

inline int tiles_of(int d) { return (d + 15) / 16; }

// Bayesian logistic regression (L2HMC_ENERGY_LOGISTIC), packed by l2hmc_pack_logistic: per 16-row data block ib,
// logistic_block_floats(NT) floats --
//   NT groups "XA", lane (i, q), k-step r:  X[16 ib + i][16 tg + 4 q + r]   A operand of the logits L^T = X w^T (over features)
//   NT groups "XT", lane (k, q), k-step r:  X[16 ib + 4 q + r][16 tg + k]   A operand of the gradient g^T = X^T r (over rows)
//   the block's 16 labels
// Rows beyond n_data are zero (and masked by the kernels: each would add softplus(0) = log 2 to U).
constexpr int kLogisticMaxRows = 1 << 20;
constexpr int kLogisticMaxDim = 128;      // the general kernel's register-resident geometries (NW * DT <= 8 tiles)
__host__ __device__ inline int logistic_block_floats(int NT) { return 512 * NT + 16; }
inline long long logistic_floats(int n, int d) { return (long long)((n + 15) / 16) * logistic_block_floats(tiles_of(d)); }
// Bayesian Poisson regression (L2HMC_ENERGY_POISSON): the same packed buffer with the counts in the label slot, and the per-row
// offsets beside it (L2hmcEnergy.prec): poisson_offset_floats(n) floats, 16 per data block, zero beyond n_data.
__host__ __device__ inline int poisson_offset_floats(int n) { return 16 * ((n + 15) >> 4); }
// The data-regression kinds: grad U is two contractions over the packed data (regression_grad) -- the general kernel only, four
// waves splitting the data blocks, the data staged in LDS or streamed.  Every host rule and kernel branch for them asks this.
__host__ __device__ constexpr bool is_data_regression(int ek) {
  return ek == L2HMC_ENERGY_LOGISTIC || ek == L2HMC_ENERGY_POISSON || ek == L2HMC_ENERGY_BINOMIAL || ek == L2HMC_ENERGY_PROBIT;
}
// Binomial / negative-binomial regression (L2HMC_ENERGY_BINOMIAL): the same packed buffer, and two per-row constants beside it
// (L2hmcEnergy.prec): per 16-row data block 32 floats, [16 offsets | 16 weights], zero beyond n_data.
__host__ __device__ inline int binomial_aux_floats(int n) { return 32 * ((n + 15) >> 4); }
// the floats of L2hmcEnergy.prec that travel with the packed data of a data-regression kind (staged behind the data blocks)
__host__ __device__ inline int regression_aux_floats(int ek, int n) {
  // (probit regression, L2HMC_ENERGY_PROBIT, has the binomial's [offsets | weights])
  return ek == L2HMC_ENERGY_POISSON ? poisson_offset_floats(n)
         : ek == L2HMC_ENERGY_BINOMIAL || ek == L2HMC_ENERGY_PROBIT ? binomial_aux_floats(n) : 0;
}
inline int khid_of(int H) { return (H + 1 + 3) / 4; }

// ------------------------------------------------------------------------------------------
// Device-side argument block
// ------------------------------------------------------------------------------------------
struct KArgs {
  const float* packed;
  const float* packed16;     // the f16x2 fragments of both nets (net_f16_floats each) behind the lane layout, or NULL
  const float* masks;
  const float* trig;
  const float* alpha;
  float eps_host;
  long long N;
  int d, H, T, step_begin, n_steps, NT;
  const float *x, *v;
  const unsigned char* dir;
  int dir_all;
  const float* u;
  float *x_out, *v_out, *logjac_out, *p_out, *x_next, *x_hist;
  int M;                     // proposals per launch (persistent sampler loop)
  unsigned rng_flags;        // L2HMC_RNG_*: which draws come from the in-kernel Philox
  unsigned long long rng_seed, rng_prop0;
  long long chain_off;
  // energy (logistic regression: mu = the packed data (global), ncomp = n_data, eta = sigma^2, easy = 1 when the data is
  // staged in LDS at o_mu; o_XB / o_prec: the state and gradient exchanges between the waves)
  int ekind, ncomp, easy;
  const float *mu, *prec, *logc;
  float eta, temperature;
  float den;                 // Rough Well: the divisor of the cosine argument (L2hmcEnergy.den, or derived from eta in float32)
  float beta;                // AIS bridge (utils/ais.py:46-47): U := (1 - beta) |x|^2 / 2 + beta U;  1 = off
  // p_accept-only kernel inputs
  const float *x1, *v1, *logjac_in;
  float *U_out, *grad_out;
  // LDS offsets (floats)
  int o_mask, o_trig, o_tb, o_P, o_XB, o_red, o_mu, o_prec, o_logc, xb_stride;
  int o_state;               // traj_wide_kernel: x, v, grad U of the tile (3 x NT x 256 floats)
  // AIS mode of the persistent loop (utils/ais.py:43-66): proposal m is anneal step m with beta = ais_beta[m]
  const float* ais_beta;     // (M) or NULL
  const float* ais_v0;       // (N, d) momentum before the first step (only read when refreshing), or NULL -> Philox
  float ais_dbeta, ais_refresh;   // refresh < 0: fresh momenta every step (ais.py:57)
  float *ais_w, *ais_alpha;  // (N) log-weights / summed accept probabilities, accumulated
  int o_fw, o_fc, o_rec;     // traj_fast_kernel: staged tail fragments, constant tables, schedule records
  unsigned long long* dbg;   // phase-timing buffer (profiling builds only, else NULL)
};

// Ladder mode (traj_ladder_kernel, l2hmc_trajectory_ladder): rows are ladder-major, K rungs per ladder; every M-th proposal
// ends with a deterministic even-odd swap sweep.  A second kernel argument of the ladder kernel only, so KArgs -- and with it
// the kernarg layout and code of every other kernel -- stays as it was.
struct LadArgs {
  int K, M;                  // rungs (2, 4, 8, 16), proposals per round
  int o_lad;                 // LDS: the tile's ladder tables (kLadLds floats)
  float temp[16];            // the ladder, by rung
  unsigned long long round0; // global index of this launch's first round
  signed char *rung, *trip, *rung_hist;   // (N) labels in/out, (N) trip states in/out or NULL, (R, N) or NULL
  const float* u;            // (R, n_ladders, K / 2) injected swap uniforms, or NULL: Philox stream 2
  float* cold;               // (R M, n_ladders, d) the rung-0 state of every ladder after every proposal, or NULL
  long long *acc, *att, *trips;   // (K - 1) swap counters, (n_ladders) round trips: accumulated (+=), or NULL
};

// Phase timers: compiled in only with -DL2HMC_PHASE_TIMING (tools/phase_timing.py).  Wave w of
// block 0 accumulates s_memtime deltas per phase into dbg[w * 16 + phase].
#ifdef L2HMC_PHASE_TIMING
#define PT_DECL unsigned long long pt_t0 = __builtin_amdgcn_s_memtime(), pt_acc[12] = {0}
#define PT_MARK(i)                                                     \
  do {                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                 \
    const unsigned long long pt_t1 = __builtin_amdgcn_s_memtime();     \
    pt_acc[i] += pt_t1 - pt_t0;                                        \
    pt_t0 = pt_t1;                                                     \
    __builtin_amdgcn_sched_barrier(0);                                 \
  } while (0)
#define PT_FLUSH(w, lane)                                                                \
  do {                                                                                   \
    if (A.dbg != nullptr && blockIdx.x == 0 && (lane) == 0)                              \
      for (int pt_i = 0; pt_i < 12; ++pt_i) A.dbg[(w) * 16 + pt_i] = pt_acc[pt_i];       \
  } while (0)
#else
#define PT_DECL
#define PT_MARK(i)
#define PT_FLUSH(w, lane)
#endif

__device__ __forceinline__ f4 splat(float a) { return f4{a, a, a, a}; }
// Branch-free transcendental forms for the hot loop (ocml's expf / tanhf carry range and
// denormal branches that serialise the 12 independent chains of a tile):
//   exp(x)  = v_exp_f32(x * log2 e)                  rel. error <= ~1e-7 (1 + |x|)
//   tanh(z) = 1 - 2 / (1 + exp(2 z))  (v_exp + v_rcp) abs. error <= ~2e-7, exact limits +-1
// Both are applied to net outputs that only enter as eps * S, eps * Q (|.| < ~1); the parity
// tests against the golden vectors bound the effect ("numerics").
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float ftanh(float z) {
  const float t = __builtin_amdgcn_exp2f(z * 2.8853900817779268f);
  return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + t), 1.f);
}
__device__ __forceinline__ f4 exp4(f4 a) { return f4{fexp(a.x), fexp(a.y), fexp(a.z), fexp(a.w)}; }
__device__ __forceinline__ f4 tanh4(f4 a) { return f4{ftanh(a.x), ftanh(a.y), ftanh(a.z), ftanh(a.w)}; }
__device__ __forceinline__ f4 exp2_4(f4 a) {
#ifdef L2HMC_ABL_NOTRANS
  return a + 1.f;
#endif
  return f4{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y), __builtin_amdgcn_exp2f(a.z),
            __builtin_amdgcn_exp2f(a.w)};
}
// c * tanh(z) with the constant folded in: c (1 - 2 / (1 + 2^(z * 2 log2 e)))
__device__ __forceinline__ f4 ctanh4(f4 c, f4 z) {
  const f4 t = exp2_4(z * 2.8853900817779268f);
  const f4 u = t + 1.f;
#ifdef L2HMC_ABL_NOTRANS
  return c * (u * -2.f + 1.f);
#endif
  const f4 r = f4{__builtin_amdgcn_rcpf(u.x), __builtin_amdgcn_rcpf(u.y), __builtin_amdgcn_rcpf(u.z),
                  __builtin_amdgcn_rcpf(u.w)};
  return c * (r * -2.f + 1.f);
}
// (an inline-asm single v_max_f32 was tried: it hides the MFMA->VALU read hazard from the
// compiler's hazard recogniser and produced wrong results -- keep the builtin)
__device__ __forceinline__ float relu1(float a) { return fmaxf(a, 0.f); }
__device__ __forceinline__ f4 relu4(f4 a) { return f4{relu1(a.x), relu1(a.y), relu1(a.z), relu1(a.w)}; }
__device__ __forceinline__ float hsum(f4 a) { return (a.x + a.y) + (a.z + a.w); }
// Sum over the four lanes (c, q = 0..3) = lanes c, c + 16, c + 32, c + 48 that hold one chain; every one of them gets the total.
// gfx950's row swaps do it on the VALU -- v_permlane16_swap_b32 exchanges the odd 16-lane rows of one register with the even rows of
// another, v_permlane32_swap_b32 the wave's halves -- where `v += __shfl_xor(v, 16); v += __shfl_xor(v, 32)` compiles to two
// dependent ds_bpermute_b32 (an LDS round trip each: ~100 cycles in front of a lone wave, four per leapfrog step in the mixtures'
// grad U).  Same pairs added in the same order, (r0 + r1) + (r2 + r3) in every lane: the same bits as the shuffle form (round 6).
typedef unsigned u2v_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float chain4_sum(float a) {
#ifdef L2HMC_CHAIN_SUM_BPERMUTE
  a += __shfl_xor(a, 16);
  a += __shfl_xor(a, 32);
  return a;
#else
  const u2v_ r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
  const float b = __uint_as_float(r.x) + __uint_as_float(r.y);
  const u2v_ t = __builtin_amdgcn_permlane32_swap(__float_as_uint(b), __float_as_uint(b), false, false);
  return __uint_as_float(t.x) + __uint_as_float(t.y);
#endif
}
__device__ __forceinline__ f4 sel4(bool c, f4 a, f4 b) { return c ? a : b; }
__device__ __forceinline__ f4 lds4(const float* p) { return *reinterpret_cast<const f4*>(p); }

// ---- sin / cos of the Rough Well (distributions.py:84-97): arguments are x / eta (easy) or x / eta^2 ------------------------
// ocml's sinf / cosf carry the Payne-Hanek path for arguments up to 2^127; the `easy` sweep (BASELINE config 4) only ever sees
// |x / eta| of a few hundred.  For |a| < 8192 pi/2 the quadrant count n = rint(a 2/pi) fits 13 bits, so the three-term
// Cody-Waite reduction r = ((a - n P1) - n P2) - n P3 (P1, P2 with 8 / 11 significand bits: both products exact) is exact up to
// the last fma, and the two minimax polynomials on [-pi/4, pi/4] are good to 1 ulp (Cephes sinf / cosf constants): abs. error
// <= 1.2e-7 like ocml's, at a third of the instructions.  Larger arguments take ocml's path; the switch is WAVE-uniform
// (one lane outside the range sends its whole wave through ocml), so there is no divergence.
__device__ __forceinline__ void rw_sincos_core(float a, float& s, float& c) {
  const float n = __builtin_rintf(a * 0.6366197723675814f);
  float r = fmaf(n, -1.5703125f, a);
  r = fmaf(n, -4.837512969970703125e-4f, r);
  r = fmaf(n, -7.549789948768648e-8f, r);
  const float z = r * r;
  const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
  const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f) * z, z,
                        fmaf(-0.5f, z, 1.f));
  const int k = (int)n;
  const float ss = (k & 1) ? pc : ps, cc = (k & 1) ? ps : pc;
  s = (k & 2) ? -ss : ss;
  c = ((k + 1) & 2) ? -cc : cc;
}
constexpr float RW_FAST_MAX = 12867.0f;          // 8192 * pi / 2
__device__ __forceinline__ f4 rw_sin4(f4 a) {
  const float mx = fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w)));
  if (__builtin_amdgcn_ballot_w64(!(mx < RW_FAST_MAX)) != 0) return f4{sinf(a.x), sinf(a.y), sinf(a.z), sinf(a.w)};
  float s0, s1, s2, s3, c0, c1, c2, c3;
  rw_sincos_core(a.x, s0, c0); rw_sincos_core(a.y, s1, c1); rw_sincos_core(a.z, s2, c2); rw_sincos_core(a.w, s3, c3);
  return f4{s0, s1, s2, s3};
}
__device__ __forceinline__ f4 rw_cos4(f4 a) {
  const float mx = fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w)));
  if (__builtin_amdgcn_ballot_w64(!(mx < RW_FAST_MAX)) != 0) return f4{cosf(a.x), cosf(a.y), cosf(a.z), cosf(a.w)};
  float s0, s1, s2, s3, c0, c1, c2, c3;
  rw_sincos_core(a.x, s0, c0); rw_sincos_core(a.y, s1, c1); rw_sincos_core(a.z, s2, c2); rw_sincos_core(a.w, s3, c3);
  return f4{c0, c1, c2, c3};
}
__device__ __forceinline__ float rw_sin1(float a) {
  if (__builtin_amdgcn_ballot_w64(!(fabsf(a) < RW_FAST_MAX)) != 0) return sinf(a);
  float s, c;
  rw_sincos_core(a, s, c);
  return s;
}
__device__ __forceinline__ float rw_cos1(float a) {
  if (__builtin_amdgcn_ballot_w64(!(fabsf(a) < RW_FAST_MAX)) != 0) return cosf(a);
  float s, c;
  rw_sincos_core(a, s, c);
  return c;
}

// dynamics.py:302-309: exp(min(dH + logjac, 0)) with non-finite results mapped to 0.  TF's
// `minimum` propagates NaN (fminf would not), so a NaN Hamiltonian difference gives p = 0.
__device__ __forceinline__ float accept_prob(float val) {
  const float mn = (val != val) ? val : fminf(val, 0.f);
  const float p = expf(mn);
  return (fabsf(p) <= 3.402823466e38f) ? p : 0.f;
}

// ---- counter-based RNG (K6): Philox4x32-10 (Salmon et al. 2011), same constants as
// Random123 / cuRAND.  counter = (global chain, dim / 4, proposal index, stream), key = seed.
struct U4 { unsigned x, y, z, w; };
__host__ __device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
    const U4 n = {(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// 4 standard normals from one Philox block (two Box-Muller pairs, 24-bit uniforms) on the hardware transcendentals:
// v_log_f32 (log2), v_sqrt_f32, v_sin_f32 / v_cos_f32 (which take the angle in REVOLUTIONS: the uniform itself) -- 8
// transcendentals + 6 VALU per block against ~200 instructions for libm's logf / sqrtf / sincosf with their range reductions.
// Normals within 2e-6 of the libm forms (tests/test_gpu_parity.py::test_in_kernel_philox_matches_oracle_stream, whose oracle uses
// numpy's).  Round 3 measured +2 % in the many-chain regime and left it (the draws feed the training runs of the ESS evidence);
// since round 4 the one-wave-per-tile kernel is bound by VALU issue (profiles/r04_tile_pmc.txt: the per-proposal random-number
// work was ~20 % of its VALU instructions), which changes the sum: profiles/r04_bf16x3_heads.txt.  -DL2HMC_LIBM_NORMALS restores
// the libm forms.
__device__ __forceinline__ f4 philox_normal4(unsigned long long seed, long long gchain, unsigned blk,
                                             unsigned long long prop) {
  const U4 r = philox4x32_10(U4{(unsigned)gchain, blk, (unsigned)prop, (unsigned)(prop >> 32) << 1},
                             (unsigned)seed, (unsigned)(seed >> 32));
  const float k = 5.9604644775390625e-08f;   // 2^-24
  const float u1 = ((r.x >> 8) + 1) * k, u2 = (r.y >> 8) * k, u3 = ((r.z >> 8) + 1) * k, u4 = (r.w >> 8) * k;
#ifdef L2HMC_LIBM_NORMALS
  const float ra = sqrtf(-2.f * logf(u1)), rb = sqrtf(-2.f * logf(u3));
  float sa, ca, sb, cb;
  sincosf(6.283185307179586f * u2, &sa, &ca);
  sincosf(6.283185307179586f * u4, &sb, &cb);
#else
  const float m2ln2 = -1.3862943611198906f;   // -2 ln 2:  -2 ln u = (-2 ln 2) log2 u
  const float ra = __builtin_amdgcn_sqrtf(m2ln2 * __builtin_amdgcn_logf(u1)), rb = __builtin_amdgcn_sqrtf(m2ln2 * __builtin_amdgcn_logf(u3));
  const float sa = __builtin_amdgcn_sinf(u2), ca = __builtin_amdgcn_cosf(u2), sb = __builtin_amdgcn_sinf(u4), cb = __builtin_amdgcn_cosf(u4);
#endif
  return f4{ra * ca, ra * sa, rb * cb, rb * sb};
}
// direction bit and accept uniform of (chain, proposal): stream 1
__device__ __forceinline__ void philox_dir_u(unsigned long long seed, long long gchain,
                                             unsigned long long prop, bool& fwd, float& u) {
  const U4 r = philox4x32_10(U4{(unsigned)gchain, 0u, (unsigned)prop, ((unsigned)(prop >> 32) << 1) | 1u},
                             (unsigned)seed, (unsigned)(seed >> 32));
  fwd = (r.x & 1u) != 0;
  u = (r.y >> 8) * 5.9604644775390625e-08f;
}
// swap uniform of pair (k, k + 1) of ladder `gladder` in global round `round`: stream 2 (parallel tempering),
//   counter = (global ladder, 0xFFFFFFFF, round mod 2^32, (round >> 32) << 4 | (k >> 1) << 1 | 1),  u = (r.x >> 8) 2^-24.
// Word 1 = 0xFFFFFFFF with word 3 odd is a counter neither other stream produces: stream 1 has word 1 = 0, stream 0 an even word 3.
__device__ __forceinline__ float philox_swap_u(unsigned long long seed, long long gladder, unsigned long long round, int k) {
  const U4 r = philox4x32_10(U4{(unsigned)gladder, 0xFFFFFFFFu, (unsigned)round,
                                ((unsigned)(round >> 32) << 4) | ((unsigned)(k >> 1) << 1) | 1u},
                             (unsigned)seed, (unsigned)(seed >> 32));
  return (r.x >> 8) * 5.9604644775390625e-08f;
}
template <int DT, int NW>
__device__ __forceinline__ void rng_state(const KArgs& A, long long gchain, unsigned long long prop,
                                          int w, int q, f4 (&z)[DT]) {
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int dim0 = 16 * (w * DT + t) + 4 * q;
    f4 n = philox_normal4(A.rng_seed, gchain, (unsigned)(dim0 >> 2), prop);
    z[t] = f4{dim0 + 0 < A.d ? n.x : 0.f, dim0 + 1 < A.d ? n.y : 0.f, dim0 + 2 < A.d ? n.z : 0.f,
              dim0 + 3 < A.d ? n.w : 0.f};
  }
}

// Sum over the lanes / waves that hold one chain; every lane of the chain gets the total.
template <int NW, int NV>
__device__ __forceinline__ void chain_allreduce(float (&v)[NV], float* red, int w, int lane) {
  // (NV = 1 -- the mixtures' quadratic form, once per component and leapfrog step, with nothing to run beside it -- on the row swaps;
  //  several values at once -- a proposal's epilogue -- through the LDS crossbar, whose requests pipeline: six swaps in a row measured
  //  1.5 % of the bench kernel's cycles more than the twelve ds_bpermute they replaced, profiles/r06_chain_sum.txt)
  if constexpr (NV == 1) {
    v[0] = chain4_sum(v[0]);
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[i] += __shfl_xor(v[i], 16);
      v[i] += __shfl_xor(v[i], 32);
    }
  }
  if (NW > 1) {
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < NV; ++i) red[(w * 16 + lane) * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) s += red[(ww * 16 + (lane & 15)) * NV + i];
      v[i] = s;
    }
    __syncthreads();
  }
}

// y = G dx for a dense symmetric G packed by pack_gauss_kernel (fragments in LDS at Gp).
template <int DT, int NW>
__device__ __forceinline__ void dense_matvec(const float* Gp, const KArgs& A, float* smem, int w,
                                             int lane, const f4 (&dx)[DT], f4 (&y)[DT]) {
  const int NT = A.NT, d = A.d;
  if (NW == 1) {
#pragma unroll
    for (int to = 0; to < DT; ++to) {
      f4 acc = splat(0.f);
      if (16 * to < d) {
#pragma unroll
        for (int ti = 0; ti < DT; ++ti) {
          if (16 * ti < d) {
            const f4 G = lds4(Gp + ((to * NT + ti) * 64 + lane) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = MFMA16(G[r], dx[ti][r], acc);
          }
        }
      }
      y[to] = acc;
    }
  } else {
    float* XB = smem + A.o_XB;
    const int c = lane & 15, q = lane >> 4;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int tg = w * DT + t;
      if (tg < NT) *reinterpret_cast<f4*>(XB + c * A.xb_stride + 16 * tg + 4 * q) = dx[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int to = w * DT + t;
      f4 acc = splat(0.f);
      if (16 * to < d) {
        for (int ti = 0; ti < NT; ++ti) {
          const f4 B = lds4(XB + c * A.xb_stride + 16 * ti + 4 * q);
          const f4 G = lds4(Gp + ((to * NT + ti) * 64 + lane) * 4);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc = MFMA16(G[r], B[r], acc);
        }
      }
      y[t] = acc;
    }
    __syncthreads();
  }
}

// grad U (S-layout) and this lane's share of U (summing `Upart` over the chain's lanes
// gives U).  dynamics.py:203-218 with the energies of distributions.py.
// Per-lane energy constants kept in registers across the whole launch (diagonal Gaussian: this
// lane's slice of the mean and of the precision diagonal).
template <int EK, int DT>
struct EnergyRegs {
  static constexpr int NR = (EK == L2HMC_ENERGY_GAUSS_DIAG && DT <= 2) ? DT : 1;
  f4 mu[NR], prec[NR];
  bool loaded;
};
template <int EK, int DT, int NW>
__device__ __forceinline__ void load_energy_regs(EnergyRegs<EK, DT>& er, const KArgs& A, const float* smem, int w,
                                                 int lane) {
  er.loaded = false;
  if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG && DT <= 2) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int off = 16 * (w * DT + t) + 4 * (lane >> 4);
      const bool ok = (w * DT + t) < A.NT;
      er.mu[t] = ok ? lds4(smem + A.o_mu + off) : splat(0.f);
      er.prec[t] = ok ? lds4(smem + A.o_prec + off) : splat(0.f);
    }
    er.loaded = true;
  }
}

// Bayesian logistic regression: grad U = X^T (sigmoid(X w) - y) + w / sigma^2 for the 16 chains of the tile (S-layout), and this
// lane's share of U's data term.  Two f32-input MFMA contractions per 16-row data block, no cross-lane traffic between them:
//   logits    L^T[i, c] = sum_k XA[i, k] x^T[k, c]  -- the state tiles are the B operand, as for a net layer; the result is in
//             C/D layout, lane (c, q) holding rows 16 ib + 4 q + r,
//   gradient  g^T[k, c] += sum_i XT[k, i] r^T[i, c] -- and that C/D layout of the residuals r = sigmoid(L) - y is exactly the
//             B operand (k-step r = row 4 q + r) of this contraction.
// Wave w takes the data blocks w, w + NW, ... over ALL NT state tiles: with NW > 1 the state goes to LDS first (the exchange of
// dense_matvec), and every wave's partial gradient of all tiles comes back through LDS, summed over the waves in wave order.
// STAGED: the fragments are read from LDS (staged by stage_energy), else streamed from global memory / L2.
//
// The body is regression_grad<Link, ...>: one body for every data-regression kind, the link between the two contractions a
// small struct built from a row's linear predictor L, response y and offset o -- residual() is the row's entry of the
// gradient contraction's B operand, u_term() its term of U (evaluated only when U is wanted).  kOffset: the kind has per-row
// offsets (A.prec, 16 per data block).  kWeight: it has per-row weights too, and a link built from (L, y, o, m); A.prec then
// holds kAux = 32 floats per data block, [16 offsets | 16 weights].
struct LogitLink {          // L2HMC_ENERGY_LOGISTIC
  static constexpr bool kOffset = false, kWeight = false;
  static constexpr int kAux = 0;
  float l, y, e, inv;
  // r = sigmoid(L) - y with e = exp(-|L|): sigmoid = 1 / (1 + e) (L >= 0) or e / (1 + e); softplus(L) = max(L, 0) + log(1 + e)
  __device__ __forceinline__ LogitLink(float L, float y_, float) : l(L), y(y_) {
    e = fexp(-fabsf(l));
    inv = __builtin_amdgcn_rcpf(1.f + e);
  }
  __device__ __forceinline__ float residual() const { return (l >= 0.f ? inv : e * inv) - y; }
  __device__ __forceinline__ float u_term() const { return fmaf(-y, l, fmaxf(l, 0.f) + 0.6931471805599453f * __builtin_amdgcn_logf(1.f + e)); }
};
// L2HMC_ENERGY_POISSON, the log link with an offset: h = L + o, mu = exp(h), r = mu - y, U term mu - y h.  The family is stated
// twice in this library: PoissonLog in glm_family.hpp (the log-likelihood and mean of the history statistics, glm.hip) and here
// (the energy that is sampled).  h and mu are formed by PoissonLog's own operations -- __fadd_rn, then the hardware exp2 of fexp,
// under `fp contract(off)` -- so the mu a trajectory moves on is the mu the statistics of its history evaluate; a change to one
// statement is a change to the other.  Overflow is IEEE's: mu = inf gives a non-finite U and gradient, which the accept rule rejects.
struct PoissonLink {
  static constexpr bool kOffset = true, kWeight = false;
  static constexpr int kAux = 16;
  float h, y, mu;
  __device__ __forceinline__ PoissonLink(float L, float y_, float o) : y(y_) {
#pragma clang fp contract(off)
    h = __fadd_rn(L, o);
    mu = fexp(h);
  }
  __device__ __forceinline__ float residual() const { return __fsub_rn(mu, y); }
  __device__ __forceinline__ float u_term() const { return fmaf(-y, h, mu); }      // mu - y h, one rounding
};
// L2HMC_ENERGY_BINOMIAL, the logit link with an offset o and a weight m per row: binomial regression with m trials, and NB2
// negative-binomial regression with fixed dispersion phi as m = y + phi, o = offset - log phi (include/l2hmc.h):
//     t = L + o    e = exp(-|t|)    s = sigmoid(t) = 1 / (1 + e) for t >= 0, e / (1 + e) below    sp = softplus(t) = max(t, 0) + log(1 + e)
//     r = m s - y  (one fma)        U term = m sp - y t  (the product, then one fma)        ll = y t - m sp + c = c - U term
// THE ONE STATEMENT of the family: BinomialLogit and NegBinomialLog of glm_family.hpp (the history statistics, glm.hip) build
// this struct and call ll(), sigmoid() and t, so the t and the softplus a trajectory moves on are the ones the statistics of its
// history evaluate.  A fixed sequence of individually rounded float32 operations under `fp contract(off)`: one hardware exp2
// (fexp), one reciprocal, one hardware log2.  Nothing overflows: 0 <= s <= 1, |r| <= max(m, y), and sp <= max(t, 0) + log 2.
struct BinomialLink {
  static constexpr bool kOffset = true, kWeight = true;
  static constexpr int kAux = 32;
  float t, y, m, e, inv;
  __device__ __forceinline__ BinomialLink(float L, float y_, float o, float m_) : y(y_), m(m_) {
#pragma clang fp contract(off)
    t = __fadd_rn(L, o);
    e = fexp(-fabsf(t));
    inv = __builtin_amdgcn_rcpf(__fadd_rn(1.f, e));
  }
  __device__ __forceinline__ float sigmoid() const {
#pragma clang fp contract(off)
    return t >= 0.f ? inv : __fmul_rn(e, inv);
  }
  __device__ __forceinline__ float softplus() const {
#pragma clang fp contract(off)
    return __fadd_rn(fmaxf(t, 0.f), __fmul_rn(0.6931471805599453f, __builtin_amdgcn_logf(__fadd_rn(1.f, e))));
  }
  __device__ __forceinline__ float residual() const { return fmaf(m, sigmoid(), -y); }
  __device__ __forceinline__ float u_term() const {
#pragma clang fp contract(off)
    return fmaf(-y, t, __fmul_rn(m, softplus()));
  }
  // the log-likelihood of the row with its constant c (log C(m, y), or the NB2 one): the negation is exact, the sum one rounding
  __device__ __forceinline__ float ll(float c) const {
#pragma clang fp contract(off)
    return __fadd_rn(-u_term(), c);
  }
};
// L2HMC_ENERGY_PROBIT: binomial regression with m trials and the PROBIT link, an offset o and a weight m per row (binary probit
// is m = 1).  With t = L + o, Phi the standard normal distribution function, phi its density and lam(t) = phi(t) / Phi(t):
//     ll = y log Phi(t) + (m - y) log Phi(-t) + c        U term = -(ll - c)        r = dU/dt = (m - y) lam(-t) - y lam(t)
// Both tails are exact to a few ulps: nothing forms 1 - Phi or the log of an underflowing erfc.  With a = |t| and x = a / sqrt 2:
//     E = erfcx(x)     u = rcp(x + 2); s = (x - 2) u refined by one Newton step (e = fma(s + 1, -2, x); e = fma(s, -x, e);
//                      s = fma(u, e, s)), so that s does not depend on the reciprocal's last bit; E = P(s) u, P of degree 10 by
//                      Horner (fitted and measured by tools/fit_erfcx.py, worst relative error 5.42 x 2^-24 for
//                      every x >= 0 with the reciprocal anywhere within one ulp)
//     h = E / 2        a2 = (a / 2) a        G = exp(-a2) (hardware exp2)        Q = h G = Phi(-a) <= 1/2
//     log Phi(-a) = ln 2 log2(h) - a2                        (h <= 1/2: no cancellation, no underflow: h >= 4e-20 while a2 is finite)
//     log Phi(a) = log(1 - Q) = ln 2 log2(w) - rho / w       w = fl(1 - Q), rho = Q - (1 - w) exactly: the rounding of 1 - Q is
//                                                            put back to first order, so Q < 2^-24 (w = 1) gives -Q, not 0
//     lam(-a) = sqrt(2 / pi) / E                             lam(a) = G / (sqrt(2 pi) w)
// and the sign of t selects which of each pair belongs to t and which to -t: branch-free, as the rows of a wave have both signs.
// One exp2, two log2, three reciprocals (x + 2, E, w).  THE ONE STATEMENT of the family: ProbitBinomial of glm_family.hpp (the
// history statistics) builds this struct and calls ll() and Phi(), so a trajectory moves on the values `loo` of its history
// evaluates.  A fixed sequence of individually rounded float32 operations under `fp contract(off)`.
// Range: nothing overflows for finite |t| up to about 1e19 (E >= 4e-20, |log Phi(-a)| <= 1e38, lam(-a) <= 1.3e19).  Beyond
// |t| = 2.6e19 a2 = a^2 / 2 is inf: U is non-finite (-inf, or NaN where 0 x inf meets it), which the accept rule rejects.
struct ProbitLink {
  static constexpr bool kOffset = true, kWeight = true;
  static constexpr int kAux = 32;
  float t, y, m, a2, E, G, Q, w, invw;
  __device__ __forceinline__ ProbitLink(float L, float y_, float o, float m_) : y(y_), m(m_) {
#pragma clang fp contract(off)
    t = __fadd_rn(L, o);
    const float a = fabsf(t);
    const float x = __fmul_rn(a, 0.7071067811865476f);
    const float u = __builtin_amdgcn_rcpf(__fadd_rn(x, 2.f));
    float s = __fmul_rn(__fadd_rn(x, -2.f), u);
    float e = fmaf(__fadd_rn(s, 1.f), -2.f, x);
    e = fmaf(s, -x, e);
    s = fmaf(u, e, s);
    float p = fmaf(8.27431722e-05f, s, 7.45708967e-05f);          // the coefficients tools/fit_erfcx.py prints, highest power first
    p = fmaf(p, s, -0.000595473393f);
    p = fmaf(p, s, -0.000864148315f);
    p = fmaf(p, s, 0.00305606565f);
    p = fmaf(p, s, 0.00648878235f);
    p = fmaf(p, s, -0.021502696f);
    p = fmaf(p, s, -0.0364437886f);
    p = fmaf(p, s, 0.279471427f);
    p = fmaf(p, s, -0.687160611f);
    p = fmaf(p, s, 1.02158272f);
    E = __fmul_rn(p, u);
    a2 = __fmul_rn(__fmul_rn(0.5f, a), a);
    G = __builtin_amdgcn_exp2f(__fmul_rn(a2, -1.4426950408889634f));
    Q = __fmul_rn(__fmul_rn(0.5f, E), G);
    w = __fsub_rn(1.f, Q);
    invw = __builtin_amdgcn_rcpf(w);
  }
  // log Phi(-|t|) and log Phi(|t|)
  __device__ __forceinline__ float log_small() const {
#pragma clang fp contract(off)
    return __fsub_rn(__fmul_rn(0.6931471805599453f, __builtin_amdgcn_logf(__fmul_rn(0.5f, E))), a2);
  }
  __device__ __forceinline__ float log_big() const {
#pragma clang fp contract(off)
    const float rho = __fsub_rn(Q, __fsub_rn(1.f, w));
    return fmaf(-rho, invw, __fmul_rn(0.6931471805599453f, __builtin_amdgcn_logf(w)));
  }
  // lam(-|t|) and lam(|t|)
  __device__ __forceinline__ float lam_small() const {
#pragma clang fp contract(off)
    return __fmul_rn(0.7978845608028654f, __builtin_amdgcn_rcpf(E));
  }
  __device__ __forceinline__ float lam_big() const {
#pragma clang fp contract(off)
    return __fmul_rn(__fmul_rn(G, 0.3989422804014327f), invw);
  }
  __device__ __forceinline__ float Phi() const { return t >= 0.f ? w : Q; }
  __device__ __forceinline__ float residual() const {
#pragma clang fp contract(off)
    const float ls = lam_small(), lb = lam_big();
    const float lam_t = t >= 0.f ? lb : ls, lam_nt = t >= 0.f ? ls : lb;
    return fmaf(__fsub_rn(m, y), lam_nt, __fmul_rn(-y, lam_t));
  }
  __device__ __forceinline__ float u_term() const {
#pragma clang fp contract(off)
    const float ls = log_small(), lb = log_big();
    const float lp = t >= 0.f ? lb : ls, lq = t >= 0.f ? ls : lb;
    return fmaf(-y, lp, __fmul_rn(__fsub_rn(y, m), lq));
  }
  // the log-likelihood of the row with its constant c = log C(m, y): the negation is exact, the sum one rounding
  __device__ __forceinline__ float ll(float c) const {
#pragma clang fp contract(off)
    return __fadd_rn(-u_term(), c);
  }
};
template <class Link, int DT, int NW, bool STAGED>
__device__ __forceinline__ float regression_grad(const KArgs& A, float* smem, int w, int lane, const f4 (&x)[DT], f4 (&g)[DT],
                                                 bool wantU) {
  constexpr int NTM = NW * DT;              // compiled tiles (>= A.NT)
  const int NT = A.NT, n = A.ncomp, nblk = (n + 15) >> 4, BS = logistic_block_floats(NT);
  const int c = lane & 15, q = lane >> 4;
  const float* P;
  if constexpr (STAGED) P = smem + A.o_mu;
  else P = A.mu;
  // the offsets: staged behind the data blocks (stage_energy), or the caller's buffer
  [[maybe_unused]] const float* O = nullptr;
  if constexpr (Link::kOffset) {
    if constexpr (STAGED) O = P + (size_t)nblk * BS;
    else O = A.prec;
  }
  const float* XB = smem + A.o_XB;
  if constexpr (NW > 1) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int tg = w * DT + t;
      if (tg < NT) *reinterpret_cast<f4*>(smem + A.o_XB + c * A.xb_stride + 16 * tg + 4 * q) = x[t];
    }
    __syncthreads();
  }
  f4 gp[NTM];
#pragma unroll
  for (int tg = 0; tg < NTM; ++tg) gp[tg] = splat(0.f);
  float Ud = 0.f;
  for (int ib = NW > 1 ? w : 0; ib < nblk; ib += NW) {
    const float* blk = P + (size_t)ib * BS;
    f4 xa[NTM], xt[NTM];
#pragma unroll
    for (int tg = 0; tg < NTM; ++tg) {
      xa[tg] = tg < NT ? lds4(blk + (tg * 64 + lane) * 4) : splat(0.f);
      xt[tg] = tg < NT ? lds4(blk + ((NT + tg) * 64 + lane) * 4) : splat(0.f);
    }
    const f4 y = lds4(blk + 512 * NT + 4 * q);
    [[maybe_unused]] f4 off = splat(0.f);
    if constexpr (Link::kOffset) off = lds4(O + Link::kAux * ib + 4 * q);
    [[maybe_unused]] f4 wt = splat(0.f);
    if constexpr (Link::kWeight) wt = lds4(O + Link::kAux * ib + 16 + 4 * q);
    f4 L = splat(0.f);
#pragma unroll
    for (int tg = 0; tg < NTM; ++tg) {
      if (tg < NT) {
        // the state as the B operand: this wave's own registers, or (NW > 1) the exchanged tile
        f4 B;
        if constexpr (NW > 1) B = lds4(XB + c * A.xb_stride + 16 * tg + 4 * q);
        else B = x[tg];
#pragma unroll
        for (int r = 0; r < 4; ++r) L = MFMA16(xa[tg][r], B[r], L);
      }
    }
    // the residuals and U terms of this lane's four rows; rows beyond n_data are masked (a padded row would add softplus(0) or
    // exp(0) to U)
    const int row0 = 16 * ib + 4 * q;
    f4 res;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (Link::kWeight) {
        const Link row(L[r], y[r], off[r], wt[r]);
        const bool live = row0 + r < n;
        res[r] = live ? row.residual() : 0.f;
        if (wantU) Ud += live ? row.u_term() : 0.f;
      } else {
        const Link row(L[r], y[r], off[r]);
        const bool live = row0 + r < n;
        res[r] = live ? row.residual() : 0.f;
        if (wantU) Ud += live ? row.u_term() : 0.f;
      }
    }
#pragma unroll
    for (int tg = 0; tg < NTM; ++tg) {
      if (tg < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gp[tg] = MFMA16(xt[tg][r], res[r], gp[tg]);
      }
    }
  }
  if constexpr (NW == 1) {
#pragma unroll
    for (int t = 0; t < DT; ++t) g[t] = gp[t];
  } else {
    // (the previous call's reads of this area finished before every wave passed the state exchange's barrier above)
    float* PX = smem + A.o_prec;
#pragma unroll
    for (int tg = 0; tg < NTM; ++tg)
      if (tg < NT) *reinterpret_cast<f4*>(PX + ((w * NT + tg) * 64 + lane) * 4) = gp[tg];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int tg = w * DT + t;
      f4 sum = splat(0.f);
      if (tg < NT) {
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) sum += lds4(PX + ((ww * NT + tg) * 64 + lane) * 4);
      }
      g[t] = sum;
    }
  }
  return Ud;
}

// LAD (ladder mode): the temperature is this lane's chain's rung temperature `temp`, divided in exactly as the scalar path divides
// by A.temperature (so equal rungs give the scalar path's bits), and `Uraw` receives this lane's share of the untempered U.
template <int EK, int DT, int NW, bool LAD = false>
__device__ __forceinline__ void grad_energy(const KArgs& A, float* smem, int w, int lane,
                                            const f4 (&x)[DT], f4 (&g)[DT], float& Upart,
                                            bool wantU, const EnergyRegs<EK, DT>* er = nullptr,
                                            const float* beta_p = nullptr, float temp = 1.f, float* Uraw = nullptr) {
  const int q = lane >> 4, DP = 16 * A.NT;
  const float beta_a = beta_p != nullptr ? *beta_p : A.beta;     // (AIS loop: the bridge moves every proposal)
  float U = 0.f;
  if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) {
    {
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        f4 mu, s;
        if constexpr (DT <= 2) {
          if (er != nullptr) { mu = er->mu[t]; s = er->prec[t]; }
          else {
            const bool ok = (w * DT + t) < A.NT;
            mu = ok ? lds4(smem + A.o_mu + 16 * (w * DT + t) + 4 * q) : splat(0.f);
            s = ok ? lds4(smem + A.o_prec + 16 * (w * DT + t) + 4 * q) : splat(0.f);
          }
        } else {
          const bool ok = (w * DT + t) < A.NT;
          mu = ok ? lds4(smem + A.o_mu + 16 * (w * DT + t) + 4 * q) : splat(0.f);
          s = ok ? lds4(smem + A.o_prec + 16 * (w * DT + t) + 4 * q) : splat(0.f);
        }
        const f4 dx = x[t] - mu;
        g[t] = s * dx;
        U += 0.5f * hsum(dx * g[t]);      // (always: a wave-uniform `if (wantU)` here costs more than it saves)
      }
    }
  } else if constexpr (EK == L2HMC_ENERGY_GAUSS_DENSE) {
    {
      f4 dx[DT];
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const bool ok = (w * DT + t) < A.NT;
        const f4 mu = ok ? lds4(smem + A.o_mu + 16 * (w * DT + t) + 4 * q) : splat(0.f);
        dx[t] = x[t] - mu;
      }
      dense_matvec<DT, NW>(weights_in_global(DT) ? A.prec : smem + A.o_prec, A, smem, w, lane, dx, g);
#pragma unroll
      for (int t = 0; t < DT; ++t) U += 0.5f * hsum(dx[t] * g[t]);
    }
  } else if constexpr (EK == L2HMC_ENERGY_GMM) {
    {
      // U = -logsumexp_i(-q_i/2 + log c_i); grad = sum_i softmax_i G_i (x - mu_i).
      // Online softmax over components: no per-component storage.
      float m = -INFINITY, ssum = 0.f;
      f4 gacc[DT];
#pragma unroll
      for (int t = 0; t < DT; ++t) gacc[t] = splat(0.f);
      for (int i = 0; i < A.ncomp; ++i) {
        f4 dx[DT], y[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          const bool ok = (w * DT + t) < A.NT;
          const f4 mu = ok ? lds4(smem + A.o_mu + i * DP + 16 * (w * DT + t) + 4 * q) : splat(0.f);
          dx[t] = x[t] - mu;
        }
        dense_matvec<DT, NW>((weights_in_global(DT) ? A.prec : smem + A.o_prec) + i * gauss_floats(A.NT), A, smem, w, lane, dx, y);
        float qq[1] = {0.f};
#pragma unroll
        for (int t = 0; t < DT; ++t) qq[0] += hsum(dx[t] * y[t]);
        chain_allreduce<NW, 1>(qq, smem + A.o_red, w, lane);
        const float V = -(0.5f * qq[0]) + smem[A.o_logc + i];
        // (a component with V = -inf -- zero weight, or an overflowed quadratic -- contributes nothing; without
        //  the guards m - mn = -inf - -inf = NaN would poison the running sums: reduce_logsumexp semantics)
        const float mn = fmaxf(m, V);
        const float sc = (m == mn) ? 1.f : expf(m - mn), wi = (V == -INFINITY) ? 0.f : expf(V - mn);
        ssum = ssum * sc + wi;
#pragma unroll
        for (int t = 0; t < DT; ++t) gacc[t] = gacc[t] * sc + wi * y[t];
        m = mn;
      }
      const float inv = 1.f / ssum;
#pragma unroll
      for (int t = 0; t < DT; ++t) g[t] = gacc[t] * inv;
      if (w == 0 && lane < 16) U = -(m + logf(ssum));
    }
  } else if constexpr (EK == L2HMC_ENERGY_ROUGHWELL) {
    {
      const float eta = A.eta;
      const float den = A.den;
      const float scale = eta / den;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        f4 arg = x[t] / den;
        g[t] = x[t] - scale * rw_sin4(arg);
        if (wantU) {
          // padded dims hold x = 0 and would add eta * cos(0): mask them out
          const int dim0 = 16 * (w * DT + t) + 4 * q;
          f4 cs = rw_cos4(arg);
          f4 live = f4{dim0 < A.d ? 1.f : 0.f, dim0 + 1 < A.d ? 1.f : 0.f,
                       dim0 + 2 < A.d ? 1.f : 0.f, dim0 + 3 < A.d ? 1.f : 0.f};
          U += 0.5f * hsum(x[t] * x[t]) + eta * hsum(live * cs);
        }
      }
    }
  } else if constexpr (EK == L2HMC_ENERGY_FUNNEL) {
    {
      const bool has0 = (w == 0 && lane < 16);  // lane holding dim 0 (tile 0, q 0, r 0)
      float rv[2] = {has0 ? x[0].x : 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < DT; ++t) rv[1] += hsum(x[t] * x[t]);
      if (has0) rv[1] -= x[0].x * x[0].x;
      chain_allreduce<NW, 2>(rv, smem + A.o_red, w, lane);
      const float vv = rv[0], sum_sq = rv[1], sigma = A.eta, clip = 4.f * sigma;
      const float n = (float)(A.d - 1);
      const bool hi = vv > clip, lo = -clip > vv;
      const float s = expf(vv);
      const float s_eff = hi ? expf(clip) : (lo ? expf(-clip) : s);
      const float inv_s = 1.f / s_eff;
#pragma unroll
      for (int t = 0; t < DT; ++t) g[t] = x[t] * inv_s;
      if (has0) {
        const float gv = vv / (sigma * sigma) + ((hi || lo) ? 0.f : 0.5f * (-sum_sq / s + n));
        g[0].x = gv;
        const float lp = (vv / sigma) * (vv / sigma);
        U = 0.5f * (lp + sum_sq / s_eff + n * logf(6.283185307179586f * s_eff));
      }
    }
  } else if constexpr (is_data_regression(EK)) {
    {
      // data term (the NLL of the labels / counts), then the N(0, sigma^2 I) prior; padded dimensions hold x = 0 and add nothing
      using Link = std::conditional_t<EK == L2HMC_ENERGY_PROBIT, ProbitLink,
                                      std::conditional_t<EK == L2HMC_ENERGY_BINOMIAL, BinomialLink,
                                                         std::conditional_t<EK == L2HMC_ENERGY_POISSON, PoissonLink, LogitLink>>>;
      U = A.easy ? regression_grad<Link, DT, NW, true>(A, smem, w, lane, x, g, wantU)
                 : regression_grad<Link, DT, NW, false>(A, smem, w, lane, x, g, wantU);
      const float iv = 1.f / A.eta;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        U += 0.5f * iv * hsum(x[t] * x[t]);
        g[t] = g[t] + x[t] * iv;
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < DT; ++t) g[t] = splat(0.f);
  }
  if (beta_a != 1.f) {       // annealed energy between N(0, I) and the target (wave-uniform branch)
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      q += hsum(x[t] * x[t]);
      g[t] = x[t] * (1.f - beta_a) + g[t] * beta_a;
    }
    U = (1.f - beta_a) * 0.5f * q + beta_a * U;
  }
  if constexpr (LAD) {
    *Uraw = U;
    U = U / temp;
#pragma unroll
    for (int t = 0; t < DT; ++t) g[t] = g[t] / temp;
  } else if (A.temperature != 1.f) {
    U = U / A.temperature;
#pragma unroll
    for (int t = 0; t < DT; ++t) g[t] = g[t] / A.temperature;
  }
  Upart = U;
}

// ---- S/T/Q network, split so that layer-1 partial products can be shared -------------------
// h1_pre = W1^T a + W2^T b + (W3^T tau + biases).  The (a, b) contractions are K-split over the
// NW waves (`l1_part` + `xchg`); the tau/bias k-step, layer 2 and the heads are `net_tail`.
// Sharing (DESIGN.md "layer-1 reuse"): VNet is evaluated at the same (x, grad U) at the end of
// step t and the start of step t+1, and both XNet calls of a step see the same v_h -- those
// partial products are computed and exchanged once.

// Layer-1 partial pre-activation from one input, summed over this wave's dimension tiles.
// grp0 = 0 selects the weights of input `a` (W1), grp0 = NT those of input `b` (W2).
// For DT <= 2 the wave's layer-1 A fragments (one float4 per tile per input per net) are loaded
// ONCE per launch and stay in registers (`L1W`): no LDS round trip in front of the MFMAs.
template <int DT>
struct L1W {
  static constexpr bool RES = DT <= 2;          // register-resident?
  f4 xa[RES ? DT : 1], xb[RES ? DT : 1], va[RES ? DT : 1], vb[RES ? DT : 1];
};
template <int DT, int NW>
__device__ __forceinline__ void load_l1w(L1W<DT>& l, const float* wx, const float* wv, const KArgs& A, int w,
                                         int lane) {
  if constexpr (L1W<DT>::RES) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int tg = w * DT + t;
      const bool ok = 16 * tg < A.d;
      l.xa[t] = ok ? lds4(wx + (tg * 64 + lane) * 4) : splat(0.f);
      l.xb[t] = ok ? lds4(wx + ((A.NT + tg) * 64 + lane) * 4) : splat(0.f);
      l.va[t] = ok ? lds4(wv + (tg * 64 + lane) * 4) : splat(0.f);
      l.vb[t] = ok ? lds4(wv + ((A.NT + tg) * 64 + lane) * 4) : splat(0.f);
    }
  }
}
template <int DT, int NW>
__device__ __forceinline__ f4 l1_part(const float* wn, int grp0, const KArgs& A, int w, int lane,
                                      const f4 (&z)[DT], f4 acc, const f4* Wres = nullptr) {
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int tg = w * DT + t;
    if constexpr (L1W<DT>::RES) {
      const f4 W = Wres[t];           // zero for dead tiles: no guard branch at all
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = MFMA16(W[r], z[t][r], acc);
    } else {
      if (16 * tg < A.d) {
        const f4 W = lds4(wn + ((grp0 + tg) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r)   // dead k-steps (dims >= d) multiply zeros: no guard branch
          acc = MFMA16(W[r], z[t][r], acc);
      }
    }
  }
  return acc;
}

// Sum NP partial vectors over the NW waves of the workgroup: one LDS hop, one barrier
// (double-buffered so the next exchange never overwrites a buffer still being read).
template <int NW, int NP>
__device__ __forceinline__ void xchg(f4 (&p)[NP], const KArgs& A, float* smem, int w, int lane,
                                     int& pb) {
#ifdef L2HMC_ABL_NOXCHG
  return;
#endif
  if (NW > 1) {
    float* P = smem + A.o_P + pb * (NW * NP * 256);
#pragma unroll
    for (int i = 0; i < NP; ++i) *reinterpret_cast<f4*>(P + ((w * NP + i) * 64 + lane) * 4) = p[i];
    __syncthreads();
    // all NW * NP reads are issued back to back into distinct registers and summed afterwards
    // (a running sum makes the compiler wait for each read before issuing the next)
    f4 part[NP][NW];
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) part[i][ww] = lds4(P + ((ww * NP + i) * 64 + lane) * 4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      f4 sum = part[i][0];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) sum += part[i][ww];
      p[i] = sum;
    }
    pb ^= 1;
  }
}

// Weight fragments of the tail (tau/bias k-step, layer 2, heads, ScaleTanh scales).  Loaded
// BEFORE the exchange barrier so their LDS latency hides under it.
// (Head fragments are register-prefetched only for DT <= 2; wider waves read them from LDS
// tile by tile inside net_tail to stay within the register budget.)
template <int DT>
struct TailW {
  static constexpr int NH = DT <= 2 ? DT : 1;
  f4 w2;
  f4 hs[NH], ht[NH], hq[NH], es[NH], eq[NH];
  const float* wn;
  int NT, w, lane;
};

template <int DT, int NW>
__device__ __forceinline__ void load_tail(TailW<DT>& tw, const float* wn, const KArgs& A, int w,
                                          int lane) {
  const int NT = A.NT, q = lane >> 4;
  tw.wn = wn; tw.NT = NT; tw.w = w; tw.lane = lane;
  tw.w2 = lds4(wn + ((2 * NT + 1) * 64 + lane) * 4);
  const float* sc = wn + net_groups(NT) * 256;
  if constexpr (DT > 2) return;
#pragma unroll
  for (int t = 0; t < TailW<DT>::NH; ++t) {
    const int tg = w * DT + t;
    if (tg < NT) {
      tw.hs[t] = lds4(wn + ((2 * NT + 2 + 3 * tg + 0) * 64 + lane) * 4);
      tw.ht[t] = lds4(wn + ((2 * NT + 2 + 3 * tg + 1) * 64 + lane) * 4);
      tw.hq[t] = lds4(wn + ((2 * NT + 2 + 3 * tg + 2) * 64 + lane) * 4);
      tw.es[t] = lds4(sc + 16 * tg + 4 * q);
      tw.eq[t] = lds4(sc + 16 * NT + 16 * tg + 4 * q);
    } else {
      tw.hs[t] = tw.ht[t] = tw.hq[t] = tw.es[t] = tw.eq[t] = splat(0.f);
    }
  }
}

// h1 = relu(hpre + tau/bias term); h2 = relu(W4^T h1); heads.  The heads' nonlinearities are
// emitted in "folded" form: with kS = (+-)eps log2(e) (eps/2 for VNet) and kQ = eps log2(e),
//   aS = kS e^{lam_s} tanh(z_s)   (= log2 of the scale factor; sums to the log-det / ln 2)
//   ES = 2^{aS} = exp(+-eps S),   EQ = 2^{kQ e^{lam_q} tanh(z_q)} = exp(eps Q),   T = z_t
// `apply(t, ES, aS, T, EQ)` consumes one 16-dimension tile at a time.
template <int DT, int KH, class F>
__device__ __forceinline__ void net_tail(const TailW<DT>& tw, f4 hpre, f4 tb, float kS,
                                         float kQ, F&& apply) {
  // tb = W3^T tau + (b1 + b2 + b3) for this chain's schedule row: a per-(net, row) table built
  // once per launch (it is the same for every chain), so no tau k-step MFMA on the critical path
  f4 h = relu4(hpre + tb);
  {
    f4 acc = splat(0.f);
#pragma unroll
    for (int r = 0; r < KH; ++r) acc = MFMA16(tw.w2[r], h[r], acc);
    h = relu4(acc);
  }
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    f4 Ws, Wt, Wq, es, eq;
    if constexpr (DT <= 2) {
      Ws = tw.hs[t]; Wt = tw.ht[t]; Wq = tw.hq[t]; es = tw.es[t]; eq = tw.eq[t];
    } else {
      const int tg = tw.w * DT + t, NT = tw.NT, lane = tw.lane;
      const float* sc = tw.wn + net_groups(NT) * 256;
      const bool ok = tg < NT;
      Ws = ok ? lds4(tw.wn + ((2 * NT + 2 + 3 * tg + 0) * 64 + lane) * 4) : splat(0.f);
      Wt = ok ? lds4(tw.wn + ((2 * NT + 2 + 3 * tg + 1) * 64 + lane) * 4) : splat(0.f);
      Wq = ok ? lds4(tw.wn + ((2 * NT + 2 + 3 * tg + 2) * 64 + lane) * 4) : splat(0.f);
      es = ok ? lds4(sc + 16 * tg + 4 * (lane >> 4)) : splat(0.f);
      eq = ok ? lds4(sc + 16 * NT + 16 * tg + 4 * (lane >> 4)) : splat(0.f);
    }
    f4 zs = splat(0.f), zt = splat(0.f), zq = splat(0.f);
#ifdef L2HMC_ABL_NOHEADS
    zs = h * Ws; zq = h * Wq; zt = h * Wt;
#else
#pragma unroll
    for (int r = 0; r < KH; ++r) {
      zs = MFMA16(Ws[r], h[r], zs);
      zq = MFMA16(Wq[r], h[r], zq);
      zt = MFMA16(Wt[r], h[r], zt);
    }
#endif
#ifdef L2HMC_IGLP
    __builtin_amdgcn_iglp_opt(L2HMC_IGLP);
#endif
    const f4 aS = ctanh4(es * kS, zs);
    apply(t, exp2_4(aS), aS, zt, exp2_4(ctanh4(eq * kQ, zq)));
  }
}

// One momentum half-update.  forward (dynamics.py:121-125,149-153):
//   v' = v e^{eps S / 2} + (eps/2)(T - e^{eps Q} grad);   backward (:164-170,194-199):
//   v' = (v - (eps/2)(T - e^{eps Q} grad)) e^{-eps S / 2}.
// ES = e^{+-eps S / 2}, EQ = e^{eps Q}, aS = log2(ES); `ld2` accumulates log2|det| as a 4-wide partial
// sum (one packed add per update; summed across its components once per trajectory).
__device__ __forceinline__ f4 v_half(f4 vin, f4 g, f4 ES, f4 aS, f4 T, f4 EQ, float heps, bool fwd,
                                     f4& ld2) {
  const f4 cc = heps * (T - EQ * g);
  ld2 += aS;
  return sel4(fwd, vin * ES + cc, (vin - cc) * ES);
}

// One masked position update; `kp` = kept coordinates (0/1).  forward (dynamics.py:131-145):
//   z' = kp z + (1-kp)(z e^{eps S} + eps (e^{eps Q} v_h + T));   backward (:176-190):
//   z' = kp z + (1-kp) e^{-eps S} (z - eps (e^{eps Q} v_h + T)).
__device__ __forceinline__ f4 x_half(f4 zin, f4 kp, f4 vh, f4 ES, f4 aS, f4 T, f4 EQ, float eps,
                                     bool fwd, f4& ld2) {
  const f4 up = splat(1.f) - kp;
  const f4 tr = eps * (EQ * vh + T);
  const f4 nw = sel4(fwd, zin * ES + tr, ES * (zin - tr));
  ld2 += up * aS;
  return kp * zin + up * nw;
}

template <int DT, int NW>
__device__ __forceinline__ void load_state(const float* p, const KArgs& A, long long chain,
                                           bool live, int w, int q, f4 (&z)[DT]) {
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int dim0 = 16 * (w * DT + t) + 4 * q;
    f4 r = splat(0.f);
    if (live && p != nullptr) {
      // rows are 16-byte aligned when d % 4 == 0 (one dwordx4 per lane and tile), 8-byte aligned when d is
      // even (two dwordx2); dim0 is a multiple of 4, so "dim0 < d" then covers the whole vector
      const float* row = p + chain * A.d + dim0;
      if ((A.d & 3) == 0) {
        if (dim0 < A.d) r = *reinterpret_cast<const f4*>(row);
      } else if ((A.d & 1) == 0) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        if (dim0 < A.d) { const f2 a = *reinterpret_cast<const f2*>(row); r.x = a.x; r.y = a.y; }
        if (dim0 + 2 < A.d) { const f2 b = *reinterpret_cast<const f2*>(row + 2); r.z = b.x; r.w = b.y; }
      } else {
        if (dim0 + 0 < A.d) r.x = row[0];
        if (dim0 + 1 < A.d) r.y = row[1];
        if (dim0 + 2 < A.d) r.z = row[2];
        if (dim0 + 3 < A.d) r.w = row[3];
      }
    }
    z[t] = r;
  }
}

template <int DT, int NW>
__device__ __forceinline__ void store_state(float* p, const KArgs& A, long long chain, bool live,
                                            int w, int q, const f4 (&z)[DT]) {
  if (p == nullptr || !live) return;
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int dim0 = 16 * (w * DT + t) + 4 * q;
    float* row = p + chain * A.d + dim0;
    if ((A.d & 3) == 0) {
      if (dim0 < A.d) *reinterpret_cast<f4*>(row) = z[t];
    } else if ((A.d & 1) == 0) {
      typedef float f2 __attribute__((ext_vector_type(2)));
      if (dim0 < A.d) *reinterpret_cast<f2*>(row) = f2{z[t].x, z[t].y};
      if (dim0 + 2 < A.d) *reinterpret_cast<f2*>(row + 2) = f2{z[t].z, z[t].w};
    } else {
      if (dim0 + 0 < A.d) row[0] = z[t].x;
      if (dim0 + 1 < A.d) row[1] = z[t].y;
      if (dim0 + 2 < A.d) row[2] = z[t].z;
      if (dim0 + 3 < A.d) row[3] = z[t].w;
    }
  }
}

// Stage energy parameters into LDS (padded with zeros to 16*NT dims).
template <int EK, bool WG = false>
__device__ __forceinline__ void stage_energy(const KArgs& A, float* smem, int tid, int nthr) {
  const int DP = 16 * A.NT;
  const int nc = EK == L2HMC_ENERGY_GMM ? A.ncomp : 1;
  if (EK == L2HMC_ENERGY_GAUSS_DIAG || EK == L2HMC_ENERGY_GAUSS_DENSE ||
      EK == L2HMC_ENERGY_GMM) {
    for (int i = tid; i < nc * DP; i += nthr) {
      const int comp = i / DP, dim = i % DP;
      smem[A.o_mu + i] = dim < A.d ? A.mu[comp * A.d + dim] : 0.f;
    }
  }
  if (EK == L2HMC_ENERGY_GAUSS_DIAG) {
    for (int i = tid; i < DP; i += nthr) smem[A.o_prec + i] = i < A.d ? A.prec[i] : 0.f;
  } else if (EK == L2HMC_ENERGY_GAUSS_DENSE || EK == L2HMC_ENERGY_GMM) {
    if (!WG) {
      const int n4 = nc * gauss_floats(A.NT) / 4;
      const f4* src = reinterpret_cast<const f4*>(A.prec);
      f4* dst = reinterpret_cast<f4*>(smem + A.o_prec);
      for (int i = tid; i < n4; i += nthr) dst[i] = src[i];
    }
    if (EK == L2HMC_ENERGY_GMM)
      for (int i = tid; i < nc; i += nthr) smem[A.o_logc + i] = A.logc[i];
  } else if (is_data_regression(EK)) {
    if (A.easy) {
      const int n4 = ((A.ncomp + 15) >> 4) * logistic_block_floats(A.NT) / 4;
      const f4* src = reinterpret_cast<const f4*>(A.mu);
      f4* dst = reinterpret_cast<f4*>(smem + A.o_mu);
      for (int i = tid; i < n4; i += nthr) dst[i] = src[i];
      if (EK == L2HMC_ENERGY_POISSON) {      // the offsets behind the data blocks (regression_grad reads them there)
        const f4* so = reinterpret_cast<const f4*>(A.prec);
        for (int i = tid; i < poisson_offset_floats(A.ncomp) / 4; i += nthr) dst[n4 + i] = so[i];
      }
      if (EK == L2HMC_ENERGY_BINOMIAL || EK == L2HMC_ENERGY_PROBIT) {     // ... and the [offsets | weights] of every block
        const f4* so = reinterpret_cast<const f4*>(A.prec);
        for (int i = tid; i < binomial_aux_floats(A.ncomp) / 4; i += nthr) dst[n4 + i] = so[i];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The fused trajectory kernel
// ------------------------------------------------------------------------------------------
// LDS of the ladder tables (floats at A.o_lad): temperature by rung, raw U by row, then ints: label by row, row by rung, trip state
// by row, accepted / attempted swaps by pair, the "some row changed temperature" flag
constexpr int kLadLds = 128;
enum { LAD_TEMP = 0, LAD_U = 16, LAD_LAB = 32, LAD_INV = 48, LAD_TRIP = 64, LAD_ACC = 80, LAD_ATT = 96, LAD_FLAG = 112 };


// (waves-per-SIMD hint 2 for DT <= 2 caps the kernel at 256 VGPRs, which makes the compiler keep
// MFMA accumulators in VGPRs -- no v_accvgpr_read traffic; wide-DT kernels keep all 512.)
#ifndef L2HMC_WAVES_PER_SIMD
#define L2HMC_WAVES_PER_SIMD 2
#endif
// (logistic regression keeps all 512 at every DT: its data contractions hold the state of every tile of the workgroup, the
//  prefetched fragments and the partial gradients on top of the trajectory's registers -- under the 256 cap they spilled)
template <int EK, int DT>
constexpr int traj_waves_per_simd() { return (DT <= 2 && !is_data_regression(EK)) ? L2HMC_WAVES_PER_SIMD : 1; }
template <int EK, int DT, int NW, int KH>
__global__ __launch_bounds__(64 * NW, (traj_waves_per_simd<EK, DT>())) void traj_kernel(const KArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  lds_poison(smem);
  constexpr bool LAD = false;
  const LadArgs* const L = nullptr;
#include "traj_body.inc"
}

// Parallel tempering (l2hmc_trajectory_ladder): rows are ladder-major, K | 16 rungs per ladder, so every ladder lies inside
// one 16-chain tile.  Proposal m runs at the temperature of the row's current rung; after every M-th proposal the tile's
// raw energies go to LDS and one lane per ladder runs the even-odd swap sweep, which relabels rows -- no state moves.
template <int EK, int DT, int NW, int KH>
__global__ __launch_bounds__(64 * NW, (traj_waves_per_simd<EK, DT>())) void traj_ladder_kernel(const KArgs A, const LadArgs Lk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  lds_poison(smem);
  constexpr bool LAD = true;
  const LadArgs* const L = &Lk;
#include "traj_body.inc"
}

// energy / grad only  (Dynamics.energy, Dynamics.grad_energy)
template <int EK, int DT, int NW>
__global__ __launch_bounds__(64 * NW) void energy_kernel(const KArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  lds_poison(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int c = lane & 15, q = lane >> 4;
  const long long chain = (long long)blockIdx.x * 16 + c;
  const bool live = chain < A.N;
  stage_energy<EK, weights_in_global(DT)>(A, smem, tid, 64 * NW);
  f4 x[DT], g[DT];
  load_state<DT, NW>(A.x, A, chain, live, w, q, x);
  __syncthreads();
  float U[1];
  grad_energy<EK, DT, NW>(A, smem, w, lane, x, g, U[0], true);
  store_state<DT, NW>(A.grad_out, A, chain, live, w, q, g);
  chain_allreduce<NW, 1>(U, smem + A.o_red, w, lane);
  if (A.U_out != nullptr && live && w == 0 && lane < 16) A.U_out[chain] = U[0];
}

// p_accept on arbitrary end points  (Dynamics.p_accept)
template <int EK, int DT, int NW>
__global__ __launch_bounds__(64 * NW) void paccept_kernel(const KArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  lds_poison(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int c = lane & 15, q = lane >> 4;
  const long long chain = (long long)blockIdx.x * 16 + c;
  const bool live = chain < A.N;
  stage_energy<EK, weights_in_global(DT)>(A, smem, tid, 64 * NW);
  f4 x[DT], v[DT], g[DT];
  float red[4];
  __syncthreads();
  load_state<DT, NW>(A.x, A, chain, live, w, q, x);
  load_state<DT, NW>(A.v, A, chain, live, w, q, v);
  grad_energy<EK, DT, NW>(A, smem, w, lane, x, g, red[0], true);
  red[1] = 0.f;
#pragma unroll
  for (int t = 0; t < DT; ++t) red[1] += 0.5f * hsum(v[t] * v[t]);
  load_state<DT, NW>(A.x1, A, chain, live, w, q, x);
  load_state<DT, NW>(A.v1, A, chain, live, w, q, v);
  grad_energy<EK, DT, NW>(A, smem, w, lane, x, g, red[2], true);
  red[3] = 0.f;
#pragma unroll
  for (int t = 0; t < DT; ++t) red[3] += 0.5f * hsum(v[t] * v[t]);
  chain_allreduce<NW, 4>(red, smem + A.o_red, w, lane);
  if (live && w == 0 && lane < 16) {
    const float val = (red[0] + red[1]) - (red[2] + red[3]) + A.logjac_in[chain];
    A.p_out[chain] = accept_prob(val);
  }
}


// ------------------------------------------------------------------------------------------
// Launch plans and launchers.  l2hmc_abi.hip plans a call (plan_trajectory: every selection rule) and hands the plan to the
// translation unit that holds its kernel; the launcher templates are defined in traj_launch.hpp / traj_lane_inst.hpp /
// traj_wide.hip and explicitly instantiated by those units only.
// ------------------------------------------------------------------------------------------
const int kMaxLdsBytes = 160 * 1024;

// the kernel a plan launches (ENERGY, PACCEPT: l2hmc_energy, l2hmc_p_accept)
enum Family { FAM_GENERAL, FAM_FAST, FAM_SMALL, FAM_TILE, FAM_WIDE, FAM_LANE, FAM_LADDER, FAM_ENERGY, FAM_PACCEPT };

// Everything the launch of one call needs beyond KArgs: the family and its template arguments.
struct TrajPlan {
  int family = FAM_GENERAL;
  int ek = 0;               // energy kind (EK)
  int DT = 1, NW = 1;       // tiles per wave and waves per workgroup; tile: DT = dim-tiles; wide: NW only
  int KH = 3;               // hidden k-steps of the nets, 3 or 4
  int tpw = 4;              // tile: tiles (waves) per workgroup
  bool half = false;        // tile: the last dimension slice holds <= 2 dimensions
  int DP = 0, HPR = 0, RES = 0;   // lane: compiled dimensions, hidden units per register pair, weight residency
  int f16 = 0;              // f16x2 contractions (PK / F16 of the fast, small and wide kernels)
  bool one_wave = false;    // fast: the common-launch body under the one-workgroup-per-CU bound (traj_fast_cc_kernel)
  long long lds = 0;        // dynamic LDS bytes
};

// The end of every entry that launched something: the launches' error, or L2HMC_OK.
inline int launched() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
  return L2HMC_OK;
}

// A workspace handed out front to back: take<T>(count) is the next `count` elements of T, pad(a) rounds the offset up to a
// multiple of `a` bytes.  Only the offsets count under a null base: `off` after the last take is the workspace's size.
struct Carve {
  char* base;
  int64_t off = 0;
  template <class T> T* take(int64_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += count * (int64_t)sizeof(T);
    return p;
  }
  void pad(int64_t a) { off = (off + a - 1) / a * a; }
};

// One kernel launch: the LDS limit, the dynamic-LDS attribute above 48 KiB, the grid size, the launch and its error.
template <class K, class... X>
int launch_kernel(K kern, long long blocks, int threads, long long lds_bytes, hipStream_t s, const X&... args) {
  if (lds_bytes > kMaxLdsBytes)
    return fail(L2HMC_ERR_UNSUPPORTED, "needs %s%lld bytes of LDS (> 160 KiB): d too large for the LDS-resident weight path", "", lds_bytes);
  if (lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return fail(L2HMC_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  if (blocks > 0x7fffffffLL) return fail(L2HMC_ERR_UNSUPPORTED, "too many chains%s");
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), (size_t)lds_bytes, s, args...);
  return launched();
}

// Template arguments from run-time values: f is a generic lambda called with std::integral_constant arguments, so every branch
// names (and instantiates) one kernel.
template <auto V> using ic = std::integral_constant<decltype(V), V>;

// f(ic<A>) if first, else f(ic<B>)
template <auto A, auto B, class F>
int on_either(bool first, F&& f) { return first ? f(ic<A>{}) : f(ic<B>{}); }

// f(ic<EK>) for a built-in energy kind (L2HMC_ENERGY_GAUSS_DIAG = 1 ... L2HMC_ENERGY_FUNNEL = 5, L2HMC_ENERGY_LOGISTIC = 7,
// L2HMC_ENERGY_POISSON = 8, L2HMC_ENERGY_BINOMIAL = 9, L2HMC_ENERGY_PROBIT = 10)
template <class F>
int on_energy_kind(int ek, F&& f) {
  switch (ek) {
    case 1: return f(ic<1>{});
    case 2: return f(ic<2>{});
    case 3: return f(ic<3>{});
    case 4: return f(ic<4>{});
    case 5: return f(ic<5>{});
    case 7: return f(ic<7>{});
    case 8: return f(ic<8>{});
    case 9: return f(ic<9>{});
    case 10: return f(ic<10>{});
  }
  return fail(L2HMC_ERR_ARG, "unknown energy kind%s");
}

// The compiled (DT, NW) geometries: general, energy, p_accept and ladder kernels; the instruction-lean kernel (traj_fast.hpp).
template <int DT_, int NW_> struct Geom { static constexpr int DT = DT_, NW = NW_; };
template <class... G> struct Geoms {};
using GeneralGeoms = Geoms<Geom<1, 1>, Geom<2, 1>, Geom<4, 1>, Geom<1, 4>, Geom<2, 4>, Geom<4, 4>, Geom<8, 4>>;
// the data-regression kinds (d <= 128): four waves with one or two state tiles each, and one wave for d <= 16 (variant 101)
using LogisticGeoms = Geoms<Geom<1, 1>, Geom<1, 4>, Geom<2, 4>>;
using FastGeoms = Geoms<Geom<1, 1>, Geom<2, 1>, Geom<1, 4>, Geom<2, 4>, Geom<2, 2>>;

// f(ic<DT>, ic<NW>) for the geometry of the set; `what` names the kernel in the refusal ("" or "fast ")
template <class... G, class F>
int on_geometry(Geoms<G...>, int DT, int NW, const char* what, F&& f) {
  int rc = L2HMC_OK;
  const bool found = ((DT == G::DT && NW == G::NW && ((rc = f(ic<G::DT>{}, ic<G::NW>{})), true)) || ...);
  return found ? rc : fail(L2HMC_ERR_UNSUPPORTED, "no %skernel for this geometry", what);
}

// The launchers, one per kind of translation unit; each launches the kernel plan p names, with k.
template <int EK>   // traj_kernel, traj_fast_kernel (f32-input MFMA), traj_small_kernel, energy_kernel, paccept_kernel: traj_ek<EK>.hip
int launch_ek(const TrajPlan& p, const KArgs& k, hipStream_t s);
template <int EK>   // traj_fast_kernel<EK, ., ., ., 1>: traj_f16_ek<EK>.hip (diagonal Gaussian, Rough Well)
int launch_fast16_ek(const TrajPlan& p, const KArgs& k, hipStream_t s);
// traj_fast_cc_kernel<1, 1, 4, ., 1, 1>: traj_f16_one_wave.hip (diagonal Gaussian, one tile per wave, common launches)
int launch_fast16_one_wave(const TrajPlan& p, const KArgs& k, hipStream_t s);
template <int EK>   // traj_tile_kernel: traj_tile_inst.hip (diagonal Gaussian, Rough Well)
int launch_tile_ek(const TrajPlan& p, const KArgs& k, hipStream_t s);
template <int EK>   // traj_ladder_kernel: traj_ladder_ek<EK>.hip, apart from the plain kernels' units so that their code objects stay as they were
int launch_ladder_ek(const TrajPlan& p, const KArgs& k, const LadArgs& l, hipStream_t s);
template <int EK>   // traj_wide_kernel: traj_wide.hip (Gaussians incl. dense, mixtures, Rough Well)
int launch_wide_ek(const TrajPlan& p, const KArgs& k, hipStream_t s);
template <int EK>   // traj_lane_kernel: traj_lane_a.hip (diagonal Gaussian), traj_lane_b.hip (Rough Well), traj_lane_c.hip (dense, mixtures)
int launch_lane_ek(const TrajPlan& p, const KArgs& k, hipStream_t s);

}  // namespace l2hmc
