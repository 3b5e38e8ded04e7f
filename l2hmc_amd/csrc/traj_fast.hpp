// traj_fast.hpp -- the instruction-lean form of the fused trajectory kernel (gfx950 / CDNA4).
//
// Same algorithm, tiling, S-layout, K-split exchange and sampler loop as traj_kernel
// (l2hmc_kernels.hpp; reference: utils/dynamics.py:115-309, utils/sampler.py:28-55) for the
// geometries whose weights are LDS/register resident (DT <= 2 dim-tiles per wave) with S/T/Q
// nets.  On gfx950 the f32 MFMA and the f32 VALU share the SIMD's issue time (measured:
// profiles/README.md, "many-chains regime"), so the lever is the instruction count per leapfrog
// step.  What this form removes (profiles/r02_traj_isa_hist.txt has the before / after counts):
//
//   * constants folded at staging time instead of multiplied in the loop: the S and Q head
//     fragments (weights and bias row) are scaled by 2 log2(e) when they are copied into LDS,
//     so 2^z is the first op on the MFMA result; the T head is scaled by the step size (eps for
//     XNet, eps/2 for VNet) and log2(step) is added to the Q exponent, so
//     tr = eps (e^{eps Q} v_h + T) resp. (eps/2)(T - e^{eps Q} grad U) is ONE packed fma;
//   * c tanh(z) = c + c * rcp(-(2^z + 1)/2): one per-lane constant, the sign of the direction
//     folded into it (two tables in LDS, each lane reads the one of its direction);
//   * no per-lane selects between the forward and the inverse update: with f = 1 (forward) / 0
//     and nf = f - 1,   z' = ES (z + nf tr) + f tr   is the forward update for f = 1 and the
//     inverse one for f = 0 (ES = e^{-eps S} there);
//   * masks enter as 0/1 factors of the exponent and of tr (z' = z exactly where kept), read
//     from per-direction tables ("forward keeps m first, backward keeps 1 - m first");
//   * relu on the integer view (one v_max_i32; fmaxf needs a canonicalising second v_max);
//   * the diagonal-Gaussian energy value is taken once at the end points, not every step.
#pragma once
#include "l2hmc_kernels.hpp"
#include "bf3k.hpp"

// (Round 4 measured the head contractions as K-packed bf16x3 -- bf3k.hpp, the form traj_tile.hpp uses -- in this kernel too: no
//  gain with one wave per SIMD, profiles/r04_bf16x3_heads.txt; the switch and its code were removed in round 5, commit history
//  has them.)

namespace l2hmc {

__device__ __forceinline__ float relu_i(float a) { return __int_as_float(max(__float_as_int(a), 0)); }
__device__ __forceinline__ f4 rcp4(f4 a) {
  return f4{__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y), __builtin_amdgcn_rcpf(a.z),
            __builtin_amdgcn_rcpf(a.w)};
}
__device__ __forceinline__ f4 ex2_4(f4 a) {
  return f4{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y), __builtin_amdgcn_exp2f(a.z),
            __builtin_amdgcn_exp2f(a.w)};
}

// ---- f16x2: every 16-wide contraction of the step loop as TWO f16 MFMAs at fp32-level accuracy (round 6) --------------------------
// v_mfma_f32_16x16x4_f32 runs at the f32 VECTOR rate and blocks the SIMD's VALU while it does (32 cycles per instruction,
// profiles/r03_ubench_issue.txt); v_mfma_f32_16x16x32_f16 takes 16 cycles for K = 32 and leaves the plain VALU free.
//   * w a = (64 w) (a / 64).  An activation a is split as  hd = f16(a / 64),  lo = f16(a - 64 hd)  (both round-to-nearest; the
//     fma in front of the second rounding is exact):  |a - 64 hd - lo| <= 2^-22 |a| (two 11-bit terms: within a factor four of
//     f32's own rounding of an operand) while lo is a normal f16, |a| >= 0.25; below that lo's error is
//     2^-25 ABSOLUTE.  Eight VALU instructions per float4: 2 v_pk_mul_f32,
//     2 v_cvt_pk_f16_f32, 4 v_fma_mixlo/hi_f16 (or ten: split16<true>).  hd overflows at |a| = 64 x 65504 = 4.2e6 (see L2HMC_F16_STATE_MAX
//     below: proposals whose end points exceed 2.5e5 are poisoned; variant 200 + v keeps the f32-input MFMA for such states).
//   * A weight w is split as  w_hi = f16(w),  w_lo = f16(64 (w - w_hi)) / 64  -- exact to 2^-22 |w| down to |w| ~ 4e-3, whatever
//     the size of the activation it multiplies -- and staged as two fragments  [64 w_hi | w_hi]  and  [64 w_lo | w_lo]
//     (|w| < 1023).
//   * The k-slots of one MFMA carry [hd(k) | lo(k)] of the lane's own four k (slot 8q + j: hd of k = 4q + j for j < 4, lo of k =
//     4q + j - 4 above): the first MFMA adds w_hi (64 hd + lo), the second one w_lo (64 hd + lo), ONE accumulate chain, no
//     rescaling anywhere.  Products of two f16 are exact in the f32 accumulator.
//   * Error of a K-term contraction: <= 2.5 x 2^-22 sum |w_k a_k| + 2^-25 sum over {k: |a_k| < 1/4} of |w_k| in the worst case
//     (oracle/f16x2_oracle.py, tests/test_f16x2_oracle.py); in the median within a factor two of an fp32 dot product's own error,
//     and end to end indistinguishable from the f32-input MFMA against float64 (profiles/r06_f16x2_accuracy.txt).
//   * The two MFMAs of a chain MUST be the same instruction: a v_mfma_f32_16x16x16_f16 issued right behind the
//     v_mfma_f32_16x16x32_f16 whose result it accumulates onto loses that result (roc-7.2.0 places no wait states between the
//     two pass counts; tools/ubench_f16x2.hip).
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float f2v __attribute__((ext_vector_type(2)));
#define L2HMC_F16_SCALE 64.0f
struct WF16 {      // one weight fragment: [64 w_hi | w_hi] and [64 w_lo | w_lo], one K = 32 instruction each
  h8v a1;
  h8v a2;
};
__device__ __forceinline__ h2v cvt_pk16(float a, float b) { return __builtin_convertvector(f2v{a, b}, h2v); }   // v_cvt_pk_f16_f32
// { f16(a0 - 64 h.x), f16(a1 - 64 h.y) }: the fma is exact, one rounding each (no builtin; VALU -> VALU only: nothing to pad)
__device__ __forceinline__ h2v lo_pair16(h2v h, float a0, float a1) {
  h2v r;
  const float ns = -L2HMC_F16_SCALE;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "s"(ns), "v"(a0));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(h), "s"(ns), "v"(a1));
  return r;
}
// LAT = true: the two residuals of a pair through independent v_fma_mix_f32 and one v_cvt_pk_f16_f32 -- ten instructions per
// float4 instead of eight, but no instruction waits for its neighbour's half of a register: measured faster where one wave owns
// its SIMD (traj_fast_kernel: 20.4 against 20.7 us per proposal at 4096 chains, 31.5 against 32.3 at 8192;
// profiles/r06_f16x2.txt).  LAT = false: v_fma_mixlo_f16 + v_fma_mixhi_f16 write the two halves of the pair in place.
// W0 = true: the caller's a.w is a literal +0 (the dead fourth hidden unit of a KH = 3 tail).  Its residual f16(0 - 64 * 0) is
// +0 as well, but the compiler cannot see through the asm: it is written as the constant, one instruction less per split.
template <bool LAT, bool W0 = false>
__device__ __forceinline__ h8v split16(f4 a) {
  const f4 ad = a * (1.f / L2HMC_F16_SCALE);
  const h2v h01 = cvt_pk16(ad.x, ad.y), h23 = cvt_pk16(ad.z, ad.w);
  h2v l01, l23;
  if constexpr (LAT) {
    float r0, r1, r2, r3 = 0.f;
    const float ns = -L2HMC_F16_SCALE;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h01), "s"(ns), "v"(a.x));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h01), "s"(ns), "v"(a.y));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r2) : "v"(h23), "s"(ns), "v"(a.z));
    if constexpr (!W0) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r3) : "v"(h23), "s"(ns), "v"(a.w));
    l01 = cvt_pk16(r0, r1);
    l23 = cvt_pk16(r2, r3);
  } else {
    l01 = lo_pair16(h01, a.x, a.y);
    l23 = lo_pair16(h23, a.z, a.w);
  }
  return h8v{h01.x, h01.y, h23.x, h23.y, l01.x, l01.y, l23.x, l23.y};
}
__device__ __forceinline__ WF16 wsplit16(f4 w) {
  const float sc = L2HMC_F16_SCALE;
  const h2v h01 = cvt_pk16(w.x, w.y), h23 = cvt_pk16(w.z, w.w);                       // w_hi
  const f4 r = f4{w.x - (float)h01.x, w.y - (float)h01.y, w.z - (float)h23.x, w.w - (float)h23.y} * sc;
  const h2v L01 = cvt_pk16(r.x, r.y), L23 = cvt_pk16(r.z, r.w);                       // 64 w_lo
  const h2v H01 = cvt_pk16((float)h01.x * sc, (float)h01.y * sc), H23 = cvt_pk16((float)h23.x * sc, (float)h23.y * sc);   // 64 w_hi
  const h2v l01 = cvt_pk16((float)L01.x / sc, (float)L01.y / sc), l23 = cvt_pk16((float)L23.x / sc, (float)L23.y / sc);   // w_lo
  WF16 f;
  f.a1 = h8v{H01.x, H01.y, H23.x, H23.y, h01.x, h01.y, h23.x, h23.y};
  f.a2 = h8v{L01.x, L01.y, L23.x, L23.y, l01.x, l01.y, l23.x, l23.y};
  return f;
}
// The states a proposal starts from and arrives at are checked against this bound (|x|, |v|, |grad U|; one chain-wide flag beside
// the energy sums): hd overflows at 4.2e6, the hidden layer's relu (an integer max on the bit pattern) can turn the NaN that
// follows into a plausible zero, and the proposal is therefore POISONED instead -- Lx, Lv, log-det NaN, accept probability 0.
// The bound sits a factor 16 under the operand's range because the HIDDEN activations share that range and are not watched:
// |h1| <= (row sum of |W1|) max |input| + |bias|, so nets whose rows sum to less than 16 in absolute value (the reference's
// initialisation: ~6 at d = 50) cannot overflow a hidden activation from a state inside the bound; others: variant 200 + v.
#define L2HMC_F16_STATE_MAX 2.5e5f
__device__ __forceinline__ float amax4(f4 a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))); }
// acc += W^T a for the 16 logical k of one fragment
__device__ __forceinline__ f4 mfma16x2(const WF16& W, h8v b, f4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.a1, b, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(W.a2, b, acc, 0, 0, 0);
}

// (Measured and not kept, profiles/r03_exchange_variants.txt: moving the K-split partial as 96 bits -- only r < KH of the
//  float4 are live hidden units -- and keeping a wave's own partial in registers, 3 x ds_read_b96 instead of
//  4 x ds_read_b128 per wave.  The exchange is latency-, not LDS-bandwidth-bound: b96 is neutral, and the wave-uniform
//  switch that keeps the canonical summation order costs 2.5-6 % at 4096 chains.)
// LDS geometry of the fast kernel (floats).  Host and device agree through these helpers.
// NTp = NW * DT >= NT: every wave's tiles exist in the tables (zero-filled beyond NT), so the loop has no
// "is this tile live" branches.
__host__ __device__ constexpr int fast_fw_net_f32(int NTp) { return (3 * NTp + 1) * 256; }                   // f32 tail fragments per net
__host__ __device__ constexpr int fast_fw_net(int NTp, bool f16 = false) { return (3 * NTp + 1) * (f16 ? 512 : 256); }   // staged tail fragments per net (f16x2: 2 x 16 bytes per lane)
__host__ __device__ inline int fast_dpp(int NTp) { return 16 * NTp + 16; }            // padded row of a constant table
__host__ __device__ inline int fast_fc_net(int NTp) { return 4 * fast_dpp(NTp); }     // cS(fwd) cS(bwd) cQ bQ
// What the one-workgroup-per-CU kernel (traj_fast_cc_kernel below) builds into its body, a bit per item (the OW argument of
// traj_fast_body; the host's LDS plan reads the same bits).  Bit 0: tails once per launch.  Bit 1: a static exchange buffer per
// site of the step (a third buffer).  Bit 2: the schedule record in per-wave rows, every field at a constant offset from one
// per-lane pointer.  Bit 3: the next step's XNet input split one step ahead, under the VNet exchange's reads.  (Bit 4: not
// built.)  Bit 5: every tail's log-det term added under the reads of the exchange that follows it.
// profiles/sampler_one_wave.txt, profiles/sampler_step_pipeline.txt.
#ifndef L2HMC_ONE_WAVE_ITEMS
#define L2HMC_ONE_WAVE_ITEMS 47
#endif
// ow = false: tbx(16) tbv(16) k1 mask(16 NTp).  ow = true (OW bit 2): one block of 64 floats per wave tile,
// [tbx 16 | tbv 16 | k1 of the tile 16 | 1 - k1 of the tile 16] -- tbx and tbv repeated in every block
__host__ __device__ inline int fast_rec(int NTp, bool ow = false) { return ow ? 64 * NTp : 32 + 16 * NTp; }
// T rows plus one never-used row on either side (the next-row prefetch of the last step lands there)
__host__ __device__ inline int fast_rec_dir(int NTp, int T, bool ow = false) { return (T + 2) * fast_rec(NTp, ow) + 16; }
__host__ __device__ constexpr int fast_xchg_bufs(int ow_items) { return (ow_items & 2) != 0 ? 3 : 2; }

// ow_items: the items of the one-workgroup-per-CU body when the plan picks it, 0 for every other kernel
long long plan_lds_fast(KArgs& k, int NW, int DT, bool f16 = false, int ow_items = 0);

// which activation split the four-wave kernel's contractions take (split16 above): measured per place, profiles/r06_f16x2.txt section 3
// and profiles/r06_paired_tails.txt section 4
#ifndef L2HMC_FAST_SPLIT_LAT_TAIL
#define L2HMC_FAST_SPLIT_LAT_TAIL true
#endif
#ifndef L2HMC_FAST_SPLIT_LAT_PAIR
#define L2HMC_FAST_SPLIT_LAT_PAIR true
#endif
#ifndef L2HMC_FAST_SPLIT_LAT_L1
#define L2HMC_FAST_SPLIT_LAT_L1 false        // (layer 1's splits in the 8-instruction form since the paired tails: 18.98 -> 18.70 us at 4096 chains, 8192 level)
#endif
template <int DT, bool F16 = false>
struct TailK {
  f4 w2;
  f4 hs[DT], ht[DT], hq[DT];
  f4 cS[DT], cQ[DT], bQ[DT];
};
template <int DT>
struct TailK<DT, true> {
  WF16 w2;
  WF16 hs[DT], ht[DT], hq[DT];
  f4 cS[DT], cQ[DT], bQ[DT];
};

// fw: this net's staged fragments; fc: this net's constant tables; dofs: 0 (forward) / DPp (backward)
template <int DT>
__device__ __forceinline__ void load_tailk(TailK<DT, false>& tk, const float* fw, const float* fc, int dofs, int NTp,
                                           int w, int lane) {
  const int q = lane >> 4, DPp = fast_dpp(NTp);
  tk.w2 = lds4(fw + lane * 4);
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int tg = w * DT + t;
    tk.hs[t] = lds4(fw + ((1 + 3 * tg + 0) * 64 + lane) * 4);
    tk.ht[t] = lds4(fw + ((1 + 3 * tg + 1) * 64 + lane) * 4);
    tk.hq[t] = lds4(fw + ((1 + 3 * tg + 2) * 64 + lane) * 4);
    tk.cS[t] = lds4(fc + dofs + 16 * tg + 4 * q);
    tk.cQ[t] = lds4(fc + 2 * DPp + 16 * tg + 4 * q);
    tk.bQ[t] = lds4(fc + 3 * DPp + 16 * tg + 4 * q);
  }
}
// f16x2: group g's [w_hi | w_hi] fragment at 16-byte slot g * 64 + lane, its [w_lo | w_lo] fragment at the same slot behind
// all the first ones
__device__ __forceinline__ WF16 lds_wf16(const float* fw, int NTp, int g, int lane) {
  WF16 f;
  f.a1 = *reinterpret_cast<const h8v*>(fw + (g * 64 + lane) * 4);
  f.a2 = *reinterpret_cast<const h8v*>(fw + (3 * NTp + 1) * 256 + (g * 64 + lane) * 4);
  return f;
}
template <int DT>
__device__ __forceinline__ void load_tailk(TailK<DT, true>& tk, const float* fw, const float* fc, int dofs, int NTp,
                                           int w, int lane) {
  const int q = lane >> 4, DPp = fast_dpp(NTp);
  tk.w2 = lds_wf16(fw, NTp, 0, lane);
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const int tg = w * DT + t;
    tk.hs[t] = lds_wf16(fw, NTp, 1 + 3 * tg + 0, lane);
    tk.ht[t] = lds_wf16(fw, NTp, 1 + 3 * tg + 1, lane);
    tk.hq[t] = lds_wf16(fw, NTp, 1 + 3 * tg + 2, lane);
    tk.cS[t] = lds4(fc + dofs + 16 * tg + 4 * q);
    tk.cQ[t] = lds4(fc + 2 * DPp + 16 * tg + 4 * q);
    tk.bQ[t] = lds4(fc + 3 * DPp + 16 * tg + 4 * q);
  }
}

// hsum = exchanged layer-1 sum + time/bias term.  apply(t, aS, T', EQ') with
//   aS = log2 of the (unmasked) scale factor,  T' = step * T,  EQ' = step * e^{eps Q}.
template <int DT, int KH, class F>
__device__ __forceinline__ void tail_fast(const TailK<DT, false>& tk, f4 hs_, F&& apply) {
  f4 h = splat(0.f);
#pragma unroll
  for (int r = 0; r < KH; ++r) h[r] = relu_i(hs_[r]);
  {
    f4 acc = splat(0.f);
#pragma unroll
    for (int r = 0; r < KH; ++r) acc = MFMA16(tk.w2[r], h[r], acc);
#pragma unroll
    for (int r = 0; r < KH; ++r) h[r] = relu_i(acc[r]);
  }
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    f4 zs = splat(0.f), zt = splat(0.f), zq = splat(0.f);
#pragma unroll
    for (int r = 0; r < KH; ++r) {
      zs = MFMA16(tk.hs[t][r], h[r], zs);
      zq = MFMA16(tk.hq[t][r], h[r], zq);
      zt = MFMA16(tk.ht[t][r], h[r], zt);
    }
#if !defined(L2HMC_NO_HEAD_FENCE)
    // all nine head MFMAs first: by the time they have issued, zs (whose chain ended two MFMAs ago) is readable
    // without hazard nops, then zq; zt is used last (the compiler otherwise starts the exps after two chains and pays
    // the MFMA -> VALU wait states in front of them)
    __builtin_amdgcn_sched_barrier(0);
#endif
    // c tanh(z) = c + c * rcp(-(2^{2 z log2 e} + 1) / 2); the head outputs arrive pre-scaled
    const f4 rS = rcp4(-(ex2_4(zs) * 0.5f + 0.5f));
    const f4 aS = rS * tk.cS[t] + tk.cS[t];
    const f4 rQ = rcp4(-(ex2_4(zq) * 0.5f + 0.5f));
    const f4 EQ = ex2_4(rQ * tk.cQ[t] + tk.bQ[t]);
    apply(t, aS, zt, EQ);
  }
}
// f16x2 form: two splits (the two hidden layers' activations: rows r >= KH are dead hidden units, zero), 2 + 6 MFMAs of
// 16 cycles that leave the VALU free -- no fence: the S chain's transcendentals run beside the Q and T products
template <int DT, int KH, class F>
__device__ __forceinline__ void tail_fast(const TailK<DT, true>& tk, f4 hs_, F&& apply) {
  f4 h = splat(0.f);
#pragma unroll
  for (int r = 0; r < KH; ++r) h[r] = relu_i(hs_[r]);
  {
    const f4 acc = mfma16x2(tk.w2, split16<L2HMC_FAST_SPLIT_LAT_TAIL, KH == 3>(h), splat(0.f));
#pragma unroll
    for (int r = 0; r < KH; ++r) h[r] = relu_i(acc[r]);
  }
  const h8v b = split16<L2HMC_FAST_SPLIT_LAT_TAIL, KH == 3>(h);
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    f4 zs = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a1, b, splat(0.f), 0, 0, 0);
    f4 zq = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a1, b, splat(0.f), 0, 0, 0);
    f4 zt = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a1, b, splat(0.f), 0, 0, 0);
    zs = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a2, b, zs, 0, 0, 0);
    zq = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a2, b, zq, 0, 0, 0);
    zt = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a2, b, zt, 0, 0, 0);
    const f4 rS = rcp4(-(ex2_4(zs) * 0.5f + 0.5f));
    const f4 aS = rS * tk.cS[t] + tk.cS[t];
    const f4 rQ = rcp4(-(ex2_4(zq) * 0.5f + 0.5f));
    const f4 EQ = ex2_4(rQ * tk.cQ[t] + tk.bQ[t]);
    apply(t, aS, zt, EQ);
  }
}

// TWO tails of one net on two inputs, stage by stage (round 6): VNet sees the same (x, grad U(x)) at the end of step t and at the start
// of step t + 1 -- only the time row differs, and S, T, Q do not depend on the momentum -- so the two evaluations are independent
// given the shared layer-1 sum.  The compiler keeps independent chains in source order (written one after the other, each MFMA pair
// is followed by its own wait states): here every stage is written for both.  A lone wave per SIMD is bound by the length of its
// dependent chain; four tails per step become three.  applyA consumes the first evaluation, keepB stores the second.
template <int DT, int KH, class FA, class FB>
__device__ __forceinline__ void tail_fast2(const TailK<DT, true>& tk, f4 hsa, f4 hsb, FA&& applyA, FB&& keepB) {
  f4 ha = splat(0.f), hb = splat(0.f);
#pragma unroll
  for (int r = 0; r < KH; ++r) { ha[r] = relu_i(hsa[r]); hb[r] = relu_i(hsb[r]); }
  {
    const h8v sa = split16<L2HMC_FAST_SPLIT_LAT_PAIR, KH == 3>(ha), sb = split16<L2HMC_FAST_SPLIT_LAT_PAIR, KH == 3>(hb);
    f4 acca = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.w2.a1, sa, splat(0.f), 0, 0, 0);
    f4 accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.w2.a1, sb, splat(0.f), 0, 0, 0);
    acca = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.w2.a2, sa, acca, 0, 0, 0);
    accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.w2.a2, sb, accb, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < KH; ++r) { ha[r] = relu_i(acca[r]); hb[r] = relu_i(accb[r]); }
  }
  const h8v ba = split16<L2HMC_FAST_SPLIT_LAT_PAIR, KH == 3>(ha), bb = split16<L2HMC_FAST_SPLIT_LAT_PAIR, KH == 3>(hb);
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    f4 zsa = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a1, ba, splat(0.f), 0, 0, 0);
    f4 zqa = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a1, ba, splat(0.f), 0, 0, 0);
    f4 zta = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a1, ba, splat(0.f), 0, 0, 0);
    f4 zsb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a1, bb, splat(0.f), 0, 0, 0);
    f4 zqb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a1, bb, splat(0.f), 0, 0, 0);
    f4 ztb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a1, bb, splat(0.f), 0, 0, 0);
    zsa = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a2, ba, zsa, 0, 0, 0);
    zqa = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a2, ba, zqa, 0, 0, 0);
    zta = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a2, ba, zta, 0, 0, 0);
    zsb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hs[t].a2, bb, zsb, 0, 0, 0);
    zqb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.hq[t].a2, bb, zqb, 0, 0, 0);
    ztb = __builtin_amdgcn_mfma_f32_16x16x32_f16(tk.ht[t].a2, bb, ztb, 0, 0, 0);
    const f4 rSa = rcp4(-(ex2_4(zsa) * 0.5f + 0.5f));
    const f4 aSa = rSa * tk.cS[t] + tk.cS[t];
    const f4 rQa = rcp4(-(ex2_4(zqa) * 0.5f + 0.5f));
    const f4 EQa = ex2_4(rQa * tk.cQ[t] + tk.bQ[t]);
    applyA(t, aSa, zta, EQa);
    const f4 rSb = rcp4(-(ex2_4(zsb) * 0.5f + 0.5f));
    const f4 aSb = rSb * tk.cS[t] + tk.cS[t];
    const f4 rQb = rcp4(-(ex2_4(zqb) * 0.5f + 0.5f));
    const f4 EQb = ex2_4(rQb * tk.cQ[t] + tk.bQ[t]);
    keepB(t, aSb, ztb, EQb);
  }
}

// xchg (l2hmc_kernels.hpp) for ONE partial vector with the buffer as a template argument: the address of every ds_write / ds_read
// is the lane's base plus an immediate, and no parity is carried.  Safe whenever two exchanges in a row take different buffers:
// a wave writes buffer B of exchange n + 2 (or later) only behind the barrier of exchange n + 1, and every wave reaches that
// barrier behind the s_waitcnt lgkmcnt(0) that completes its own reads of exchange n.
// In parts, so that work which does not depend on the sum can be issued while the reads are in flight: put = the write,
// get_issue = wait, barrier and the NW reads, get_sum = the sum in xchg's order.
template <int NW>
__device__ __forceinline__ void xchg_put(float* P, f4 p, int w, int lane) {
  *reinterpret_cast<f4*>(P + (w * 64 + lane) * 4) = p;
}
template <int NW>
__device__ __forceinline__ void xchg_get_issue(const float* P, int lane, f4 (&part)[NW]) {
  __syncthreads();
#pragma unroll
  for (int ww = 0; ww < NW; ++ww) part[ww] = lds4(P + (ww * 64 + lane) * 4);
  __builtin_amdgcn_sched_barrier(0);
}
template <int NW>
__device__ __forceinline__ f4 xchg_get_sum(const f4 (&part)[NW]) {
  f4 sum = part[0];
#pragma unroll
  for (int ww = 1; ww < NW; ++ww) sum += part[ww];
  return sum;
}
template <int NW>
__device__ __forceinline__ f4 xchg_get(const float* P, int lane) {
  f4 part[NW];
  xchg_get_issue<NW>(P, lane, part);
  return xchg_get_sum<NW>(part);
}
template <int NW, int B>
__device__ __forceinline__ void xchg_at(f4 (&p)[1], const KArgs& A, float* smem, int w, int lane) {
  float* P = smem + A.o_P + B * (NW * 256);
  xchg_put<NW>(P, p[0], w, lane);
  p[0] = xchg_get<NW>(P, lane);
}

// layer-1 fragments of the f16x2 form (register-resident, split once per launch)
template <int DT>
struct L1W16 {
  WF16 xa[DT], xb[DT], va[DT], vb[DT];
};
template <int DT>
__device__ __forceinline__ f4 l1_part16(const f4 (&z)[DT], f4 acc, const WF16* W) {
#pragma unroll
  for (int t = 0; t < DT; ++t) acc = mfma16x2(W[t], split16<L2HMC_FAST_SPLIT_LAT_L1>(z[t]), acc);
  return acc;
}

// PK: 0 = f32-input MFMA (v_mfma_f32_16x16x4_f32), 1 = f16x2 (above)
// CC: the body compiled for the sampler's common launch -- all three draws in-kernel, p_out + x_next and no other output.  What
// a launch draws and writes is launch-uniform, but the general body tests it lane by lane at every proposal boundary; with CC
// those tests are constants (traj_fast_kernel below picks the body by one uniform branch at entry).  The same statements either
// way: the same bits.
// OW: what the one-workgroup-per-CU kernel (traj_fast_cc_kernel below) spends its register headroom on, a bit per item; 0 in every
// other kernel.  Bit 0: both nets' tail fragments and constant rows are loaded once per launch, in front of the proposal loop.
// Bit 1: the three exchanges of a step take the static buffers 0, 1, 2 (xchg_at).  Bit 2: per-wave schedule records (fast_rec).
// Bit 3: the next step's XNet input k1 * x and its split are formed one step ahead, under the reads of the VNet exchange (the
// same expression on the same values; the first step's at the proposal's start, the peeled last step forms none).
// Bit 5: the log-det accumulation ldv += aS of a tail waits for the exchange that follows the tail and is issued while that
// exchange's reads are in flight (the same additions in the same order).
template <int EK, int DT, int NW, int KH, int PK, bool CC, int OW = 0>
__device__ __forceinline__ void traj_fast_body(const KArgs& A);

template <int EK, int DT, int NW, int KH, int PK = 0>
#ifndef L2HMC_FAST_WAVES
#define L2HMC_FAST_WAVES 2
#endif
// Register budget (round 6, profiles/r06_fast_dt2_spills.txt): with two dimension tiles per wave the f16x2 form holds 120 VGPRs of
// weight fragments (8 layer-1 + 7 tail WF16) beside the state -- under the two-waves-per-SIMD bound (256 VGPRs) the allocator spilled
// 450-630 bytes per lane to SCRATCH inside the step loop (`.amdhsa_private_segment_fixed_size`).  One wave per SIMD for DT = 2: the
// overflow goes to AGPRs (v_accvgpr_*), no scratch -- Rough Well d = 32 / 16 384 chains 62.1 -> 39.4 us per proposal, d = 96 ... 128
// 207 -> 160 (it had been SLOWER than the f32-input form it replaced: 44.9 / 181).  DT = 1 keeps the two-wave bound (8192 chains =
// two workgroups per CU), and so does the f32-input form of DT = 2 (44-184 bytes of scratch; one wave per SIMD measured 5-9 % slower:
// dense Gaussian d = 32 41.9 -> 45.6 us).  The 5-7 % that 512 registers cost DT = 1 in round 6 were not the scheduler's choices: with
// AGPRs in the budget the compiler takes the AGPR form of every MFMA result and copies each out with four v_accvgpr_read_b32 --
// 60 VALU instructions more per step (524 against 464).  -mllvm -amdgpu-mfma-vgpr-form keeps the results in VGPRs; the launches
// whose grid leaves one workgroup per CU take traj_fast_cc_kernel (below), compiled with it (profiles/sampler_one_wave.txt).
#ifndef L2HMC_FAST_WAVES_DT2
#define L2HMC_FAST_WAVES_DT2 1
#endif
__global__ __launch_bounds__(64 * NW, (DT >= 2 && PK == 1) ? L2HMC_FAST_WAVES_DT2 : L2HMC_FAST_WAVES) void traj_fast_kernel(const KArgs A) {
  // (the diagonal Gaussian's one-tile f16x2 kernels: the bench workload and its relatives.  Not Rough Well's: its body spills
  //  under the two-wave bound as it is, and a second copy raised that)
  if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG && DT == 1 && PK == 1) {
    const bool common = (A.rng_flags & (L2HMC_RNG_V | L2HMC_RNG_DIR | L2HMC_RNG_U)) == (L2HMC_RNG_V | L2HMC_RNG_DIR | L2HMC_RNG_U) &&
                        A.p_out != nullptr && A.x_next != nullptr && A.x_hist == nullptr && A.logjac_out == nullptr &&
                        A.x_out == nullptr && A.v_out == nullptr;
    if (common) traj_fast_body<EK, DT, NW, KH, PK, true>(A);
    else traj_fast_body<EK, DT, NW, KH, PK, false>(A);
  } else {
    traj_fast_body<EK, DT, NW, KH, PK, false>(A);
  }
}

// The common-launch body under a bound of its own (WB workgroups per CU; PK stays the last argument: l2hmc_last_kernel's readers tell
// the arithmetic by it).  WB = 1 for the launches whose grid has no more workgroups than the device has CUs -- the second workgroup the
// two-wave bound of traj_fast_kernel keeps half of every SIMD's register file for never arrives there.  Its translation unit
// (traj_f16_one_wave.hip) is compiled with -mllvm -amdgpu-mfma-vgpr-form: see the note at L2HMC_FAST_WAVES above.  The planner
// (plan_trajectory) sends it common launches only, so the body is picked without the entry test.
template <int EK, int DT, int NW, int KH, int WB, int PK>
__global__ __launch_bounds__(64 * NW, WB) void traj_fast_cc_kernel(const KArgs A) {
  traj_fast_body<EK, DT, NW, KH, PK, true, L2HMC_ONE_WAVE_ITEMS>(A);
}

template <int EK, int DT, int NW, int KH, int PK, bool CC, int OW>
__device__ __forceinline__ void traj_fast_body(const KArgs& A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  lds_poison(smem);
  static_assert(DT <= 2, "the fast kernel keeps layer-1 and tail fragments in registers");
  const int tid = threadIdx.x, lane = tid & 63, nthr = 64 * NW;
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int c = lane & 15, q = lane >> 4;
  const long long chain = (long long)blockIdx.x * 16 + c;
  const bool live = chain < A.N;
  const int NT = A.NT, DP = 16 * NT, NF = net_floats(NT);
  const float LOG2E = 1.4426950408889634f;
  const float eps = A.alpha != nullptr ? expf(*A.alpha) : A.eps_host;
  const float heps = 0.5f * eps;
  constexpr int NTp = NW * DT;
  constexpr bool F16 = PK == 1;
  constexpr bool XS = (OW & 2) != 0, REC1 = (OW & 4) != 0, PIPE = (OW & 8) != 0, LDW = (OW & 32) != 0;
  static_assert(!(XS || REC1 || PIPE || LDW) || (DT == 1 && PK == 1 && NW > 1), "the step-loop items: the one-tile f16x2 body only");
  // XS and the exchanges outside the step loop: they keep xchg and its parity, which alternates between buffers 0 and 1.  The
  // precision fold takes 0 (and ends in a barrier of its own), the first VNet layer-1 sum takes 1, the steps take 0, 1, 2,
  // 0, 1, 2, ...; a proposal's last exchange (2) is followed by chain_allreduce (its own area, two barriers) and the next
  // proposal's first (0).  No two exchanges in a row share a buffer, which is all xchg_at needs.
  static_assert(!LDW || PIPE, "the log-det terms under the reads: with the exchange in its parts");
  const int FWN = fast_fw_net(NTp, F16), DPp = fast_dpp(NTp), FCN = fast_fc_net(NTp), R = fast_rec(NTp, REC1),
            RECD = fast_rec_dir(NTp, A.T, REC1);

  // ---- prologue: stage the tail fragments (scaled), the constant tables and the schedule records ----
  // (the state and the register-resident layer-1 fragments are asked for first: global loads that nothing below depends on, in flight
  //  beside the staging instead of a round trip of their own behind the barrier)
  f4 x[DT], v[DT], g[DT];
  load_state<DT, NW>(A.x, A, chain, live, w, q, x);
  L1W<DT> l1w;
  load_l1w<DT, NW>(l1w, A.packed, A.packed + NF, A, w, lane);
  {
    // (eight loads in flight per thread: one element per trip, each waited for before the next, made the prologue ~7 us)
    constexpr int GN = 3 * NTp + 1;                 // groups per net: W4, then (S, T, Q) per dimension tile
    constexpr int NCP = 2 * GN * 64, NTRIP = (NCP + 64 * NW - 1) / (64 * NW);
    for (int t0 = 0; t0 < NTRIP; t0 += 8) {
      f4 buf[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = tid + (t0 + u) * nthr;
        const int net = i >= GN * 64, j = i - net * (GN * 64), g = j >> 6;
        buf[u] = splat(0.f);
        if (i < NCP && g < 3 * NT + 1) buf[u] = reinterpret_cast<const f4*>(A.packed + (size_t)net * NF + (2 * NT + 1) * 256)[j];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = tid + (t0 + u) * nthr;
        const int net = i >= GN * 64, j = i - net * (GN * 64), g = j >> 6;
        float sc = 1.f;
        if (g > 0) sc = ((g - 1) % 3 == 1) ? (net == 0 ? eps : heps) : 2.f * LOG2E;
        if constexpr (F16) {
          if (i < NCP) {
            const WF16 f = wsplit16(buf[u] * sc);
            float* base = smem + A.o_fw + net * FWN;
            reinterpret_cast<h8v*>(base)[j] = f.a1;
            reinterpret_cast<h8v*>(base + GN * 256)[j] = f.a2;
          }
        } else {
          if (i < NCP) reinterpret_cast<f4*>(smem + A.o_fw + net * FWN)[j] = buf[u] * sc;
        }
      }
    }
  }
  for (int i = tid; i < 2 * 16 * NTp; i += nthr) {
    const int net = i / (16 * NTp), dim = i % (16 * NTp);
    const float* scl = A.packed + (size_t)net * NF + net_groups(NT) * 256;
    const float epn = net == 0 ? eps : heps;
    const float es = dim < DP ? scl[dim] : 0.f, eq = dim < DP ? scl[DP + dim] : 0.f;
    const float cs = es * epn * LOG2E, cq = eq * eps * LOG2E;
    float* fc = smem + A.o_fc + net * FCN;
    fc[dim] = cs;
    fc[DPp + dim] = -cs;
    fc[2 * DPp + dim] = cq;
    fc[3 * DPp + dim] = cq + log2f(epn);
  }
  // The schedule records, both directions' tables from one evaluation, four elements' loads in flight per thread before the first
  // is waited for.  (One loop over all 2 T R elements with a select between the two kinds became a divergent branch with a
  // load-and-wait on either side in every trip: some sixteen dependent global round trips, most of the prologue's time.)
  constexpr int SU = 4;
  {      // time / bias rows: the same for both directions
    const int nA = A.T * 32;
    for (int i0 = tid; i0 < nA; i0 += SU * nthr) {
      float a0[SU], a1[SU], a2[SU], c0[SU], c1[SU];
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = min(i0 + s * nthr, nA - 1), r = i >> 5, net = (i >> 4) & 1, u = i & 15;
        const float* tf = A.packed + (size_t)net * NF + (2 * NT * 64) * 4;
        a0[s] = tf[u * 4], a1[s] = tf[(16 + u) * 4], a2[s] = tf[(32 + u) * 4], c0[s] = A.trig[2 * r], c1[s] = A.trig[2 * r + 1];
      }
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = i0 + s * nthr, r = i >> 5, j = i & 31;
        if (i < nA) {
          const float tbr = fmaf(a0[s], c0[s], fmaf(a1[s], c1[s], a2[s]));
          if constexpr (REC1) {
#pragma unroll
            for (int tg = 0; tg < NTp; ++tg) {
              smem[A.o_rec + (A.T - r) * R + 64 * tg + j] = tbr;      // (the backward table in the order it is walked)
              smem[A.o_rec + RECD + (r + 1) * R + 64 * tg + j] = tbr;
            }
          } else {
            smem[A.o_rec + (r + 1) * R + j] = tbr;
            smem[A.o_rec + RECD + (r + 1) * R + j] = tbr;
          }
        }
      }
    }
  }
  {      // mask rows: forward keeps m first, backward keeps 1 - m first
    constexpr int W16 = 16 * NTp;
    const int nB = A.T * W16;
    for (int i0 = tid; i0 < nB; i0 += SU * nthr) {
      float mk[SU];
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = min(i0 + s * nthr, nB - 1), r = i / W16, dim = i % W16;
        mk[s] = A.masks[r * A.d + (dim < A.d ? dim : 0)];
      }
#pragma unroll
      for (int s = 0; s < SU; ++s) {
        const int i = i0 + s * nthr, r = i / W16, dim = i % W16;
        if (i < nB) {
          const float m = dim < A.d ? mk[s] : 0.f;
          if constexpr (REC1) {
            // (k1 and up = 1 - k1 side by side: the expression the step would evaluate, evaluated here)
            const int o = 64 * (dim >> 4) + 32 + (dim & 15);
            const float mb = 1.f - m;
            smem[A.o_rec + (A.T - r) * R + o] = mb;
            smem[A.o_rec + (A.T - r) * R + o + 16] = 1.f - mb;
            smem[A.o_rec + RECD + (r + 1) * R + o] = m;
            smem[A.o_rec + RECD + (r + 1) * R + o + 16] = mb;
          } else {
            smem[A.o_rec + (r + 1) * R + 32 + dim] = 1.f - m;
            smem[A.o_rec + RECD + (r + 1) * R + 32 + dim] = m;
          }
        }
      }
    }
  }
  stage_energy<EK, false>(A, smem, tid, nthr);

  const bool need_p = CC || A.p_out != nullptr || A.x_next != nullptr || A.u != nullptr ||
                      (A.rng_flags & L2HMC_RNG_U) != 0;
  __syncthreads();

  const float* fwx = smem + A.o_fw;
  const float* fwv = fwx + FWN;
  const float* fcx = smem + A.o_fc;
  const float* fcv = fcx + FCN;
  int pb = 0;
  const f4 Z = splat(0.f);
  EnergyRegs<EK, DT> er;
  load_energy_regs<EK, DT, NW>(er, A, smem, w, lane);
  // grad U (and, at the end points only, this lane's share of U)
  auto grad = [&](const f4 (&xx)[DT], f4 (&gg)[DT], float& Up, bool wantU) {
    if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) {
#pragma unroll
      for (int t = 0; t < DT; ++t) gg[t] = er.prec[t] * (xx[t] - er.mu[t]);
    } else {
      grad_energy<EK, DT, NW>(A, smem, w, lane, xx, gg, Up, wantU, &er);
    }
  };
  auto diag_U = [&](const f4 (&xx)[DT], const f4 (&gg)[DT]) {
    float U = 0.f;
    if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) {
#pragma unroll
      for (int t = 0; t < DT; ++t) U += 0.5f * hsum((xx[t] - er.mu[t]) * gg[t]);
    }
    return U;
  };
  float U_start = 0.f;
  grad(x, g, U_start, need_p);
  if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) U_start = diag_U(x, g);

  TailK<DT, F16> tk;
  f4 pv[1];
  // VNet layer 1 at (x, grad U(x)).  Diagonal Gaussian: grad U = P (x - mu) is linear in x, so
  //   W1^T x + W2^T grad U = (W1 + P W2)^T x - W2^T P mu:
  // the precision is folded into the register-resident W1 fragments once per launch (fragment element
  // (lane, r) belongs to dimension 16 tg + 4 q + r -- this lane's own slice of P) and the constant goes
  // into the VNet time/bias table: one contraction per step instead of two.
  L1W16<F16 ? DT : 1> l1h;       // (filled below, after the precision has been folded into va)
  auto vnet_l1 = [&](const f4 (&xx)[DT], const f4 (&gg)[DT]) {
    if constexpr (F16) {
      if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) return l1_part16<DT>(xx, Z, l1h.va);
      else return l1_part16<DT>(gg, l1_part16<DT>(xx, Z, l1h.va), l1h.vb);
    } else if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) {
      return l1_part<DT, NW>(nullptr, 0, A, w, lane, xx, Z, l1w.va);
    } else {
      return l1_part<DT, NW>(nullptr, 0, A, w, lane, xx, Z, l1w.va) + l1_part<DT, NW>(nullptr, NT, A, w, lane, gg, Z, l1w.vb);
    }
  };
  if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) {
    f4 pm[DT], cv[1];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      l1w.va[t] = l1w.va[t] + er.prec[t] * l1w.vb[t];
      pm[t] = -(er.prec[t] * er.mu[t]);
    }
    cv[0] = l1_part<DT, NW>(nullptr, NT, A, w, lane, pm, Z, l1w.vb);
    xchg<NW, 1>(cv, A, smem, w, lane, pb);
    // (every column of the tile holds the same cv: lane (c, q) of wave 0 folds it into rows c, c + 16, ... -- one addition per
    //  row as before, two trips instead of 2 T)
    if constexpr (REC1) {      // (every wave folds it into its own block's copy of the row)
      for (int i = c; i < 2 * A.T; i += 16) {
        float* tb = smem + A.o_rec + (i / A.T) * RECD + (i % A.T + 1) * R + 64 * w + 16 + 4 * q;
        *reinterpret_cast<f4*>(tb) = lds4(tb) + cv[0];
      }
    } else if (w == 0) {
      for (int i = c; i < 2 * A.T; i += 16) {
        float* tb = smem + A.o_rec + (i / A.T) * RECD + (i % A.T + 1) * R + 16 + 4 * q;
        *reinterpret_cast<f4*>(tb) = lds4(tb) + cv[0];
      }
    }
    __syncthreads();
  }
  if constexpr (F16) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      l1h.xa[t] = wsplit16(l1w.xa[t]);
      l1h.xb[t] = wsplit16(l1w.xb[t]);
      l1h.va[t] = wsplit16(l1w.va[t]);
      l1h.vb[t] = wsplit16(l1w.vb[t]);
    }
  }
  // (Measured and not kept, profiles/r04_bf16x3_heads.txt: a head start of 256-1024 cycles for every second workgroup at 8192 chains,
  //  so that one workgroup's MFMA-heavy tails fall into the other's exchange stalls -- 38.9-39.4 us per proposal against 38.1-39.4.)
  PT_DECL;
  PT_MARK(0);      // prologue
  pv[0] = vnet_l1(x, g);
  xchg<NW, 1>(pv, A, smem, w, lane, pb);

  // ---- persistent sampler loop (as traj_kernel) ------------------------------------------------------
  const long long gchain = A.chain_off + chain;
  const bool rng_v = CC || (A.rng_flags & L2HMC_RNG_V) != 0, rng_d = CC || (A.rng_flags & L2HMC_RNG_DIR) != 0;
  const bool rng_u = CC || (A.rng_flags & L2HMC_RNG_U) != 0;
  f4 vn[DT];
  if (!rng_v) load_state<DT, NW>(A.v, A, chain, live, w, q, vn);
  bool fwd_n = (A.dir != nullptr && !rng_d) ? (live ? A.dir[chain] != 0 : true) : (A.dir_all != 0);
  float u_n = (A.u != nullptr && !rng_u && live) ? A.u[chain] : 0.f;
  const bool have_u = CC || A.u != nullptr || rng_u;
  // OW bit 0: both nets' tails once per launch.  The backward direction's cS row is the forward one negated (fc[DPp + dim] = -cs
  // above), so the forward row is held and every proposal flips its sign bit for the lanes that run backward: the same bits.
  constexpr bool ONCE = (OW & 1) != 0;
  static_assert(!ONCE || (DT == 1 && PK == 1), "tails once per launch: the one-tile f16x2 body only");
  TailK<DT, F16> tkx1;
  f4 cSx1[ONCE ? DT : 1], cSv1[ONCE ? DT : 1];
  if constexpr (ONCE) {
    load_tailk<DT>(tkx1, fwx, fcx, 0, NTp, w, lane);
    load_tailk<DT>(tk, fwv, fcv, 0, NTp, w, lane);
#pragma unroll
    for (int t = 0; t < DT; ++t) { cSx1[t] = tkx1.cS[t]; cSv1[t] = tk.cS[t]; }
  }
  for (int m = 0; m < A.M; ++m) {
    const long long moff = (long long)m * A.N;
    const unsigned long long prop = A.rng_prop0 + (unsigned long long)m;
    if (rng_v) {
      rng_state<DT, NW>(A, gchain, prop, w, q, v);
    } else {
#pragma unroll
      for (int t = 0; t < DT; ++t) v[t] = vn[t];
    }
    bool fwd = fwd_n;
    float u_m = u_n;
    if (rng_d || rng_u) {
      bool fr;
      float ur;
      philox_dir_u(A.rng_seed, gchain, prop, fr, ur);
      if (rng_d) fwd = fr;
      if (rng_u) u_m = ur;
    }
    if (m + 1 < A.M) {
      if (!rng_v) load_state<DT, NW>(A.v + (moff + A.N) * A.d, A, chain, live, w, q, vn);
      if (A.dir != nullptr && !rng_d && live) fwd_n = A.dir[moff + A.N + chain] != 0;
      if (A.u != nullptr && !rng_u && live) u_n = A.u[moff + A.N + chain];
    }
    // the start point: a rejected chain resumes from it (sampler.py:53-55)
    // (the diagonal Gaussian's grad U is two packed instructions away from x: it is re-formed from the selected state at the end of
    //  the proposal -- the same expression on the same x, the same bits -- instead of being held in registers through the trajectory)
    constexpr bool KEEP_G0 = EK != L2HMC_ENERGY_GAUSS_DIAG;
    f4 x0[DT], g0[KEEP_G0 ? DT : 1];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      x0[t] = x[t];
      if constexpr (KEEP_G0) g0[t] = g[t];
    }
    const f4 pv0 = pv[0];
    float red[F16 ? 6 : 5];        // U0, K0, U1, K1, logdet (per-lane partial sums); f16x2: + the out-of-range flag
    float amax_l = 0.f;
    if constexpr (F16) {
#pragma unroll
      for (int t = 0; t < DT; ++t) amax_l = fmaxf(amax_l, fmaxf(amax4(x[t]), fmaxf(amax4(v[t]), amax4(g[t]))));
    }
    red[0] = U_start;
    red[1] = 0.f;
#pragma unroll
    for (int t = 0; t < DT; ++t) red[1] += 0.5f * hsum(v[t] * v[t]);
    red[2] = 0.f;
    f4 ldv = splat(0.f);

    // per-lane direction constants and table addresses
    const float ff = fwd ? 1.f : 0.f, nf = ff - 1.f;
    const int dofs = fwd ? 0 : DPp;
    // (REC1: the backward table is stored in the order it is walked -- step s at row s, as the forward one -- so every lane
    //  advances by the same constant and the read-ahead is an immediate)
    const int row0 = (REC1 || fwd) ? A.step_begin : (A.T - 1 - A.step_begin);
    // this lane's record, + 4 q (REC1: + this wave's block -- tbx, tbv, k1 and up at the constant offsets 0, 16, 32, 48)
    const float* rec = smem + A.o_rec + (fwd ? RECD : 0) + (row0 + 1) * R + (REC1 ? 64 * w : 0) + 4 * q;
    const int drec = (REC1 || fwd) ? R : -R;
    f4 tbv = lds4(rec + 16);
    // (the mask row of wave tile t in this lane's record)
    auto k1_of = [&](const float* rc, int t) { return REC1 ? lds4(rc + 32 + 64 * t) : lds4(rc + 32 + 16 * (w * DT + t)); };
    f4 k1_c[PIPE ? DT : 1];
    h8v xb_c[PIPE ? DT : 1];
    if constexpr (PIPE) {
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        k1_c[t] = k1_of(rec, t);
        xb_c[t] = split16<L2HMC_FAST_SPLIT_LAT_L1>(k1_c[t] * x[t]);
      }
    }

    // Resident tails (round 6, profiles/r06_resident_tails.txt): XNet's tail fragments and constants stay in registers for the whole
    // proposal beside VNet's (44 VGPRs per net as f16x2) instead of being re-read from LDS twice per step -- 22 of a step's 37
    // ds_read_b128: ICG-50 20.4 -> 19.4-19.6 us per proposal at 4096 chains, 31.3 -> 30.0 at 8192 (251 VGPRs, no scratch).  Not for
    // the f32-input form of DT = 2, which spills under the two-wave bound already.  Same values, same arithmetic: same bits.
    // (Measured and not kept, profiles/sampler_invariant_work.txt: loading everything but the direction's cS row once per launch, in
    //  front of the proposal loop -- 20 ds_read_b128 fewer per proposal, and 0.7 % SLOWER at 4096 chains: the registers stay live
    //  through the epilogue and the allocator's choices in the step loop change.  The one-workgroup-per-CU body, whose step loop
    //  it leaves alone, does it: ONCE above, 1.2 % faster there, profiles/sampler_one_wave.txt.)
    constexpr bool RT = DT == 1 || PK == 1;
    TailK<DT, F16> tkx;
    if constexpr (RT && !ONCE) load_tailk<DT>(tkx, fwx, fcx, dofs, NTp, w, lane);
    const TailK<DT, F16>& TKX = *(ONCE ? &tkx1 : RT ? &tkx : &tk);
    if constexpr (ONCE) {
      const int sb = fwd ? 0 : (int)0x80000000u;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          tkx1.cS[t][r] = __int_as_float(__float_as_int(cSx1[t][r]) ^ sb);
          tk.cS[t][r] = __int_as_float(__float_as_int(cSv1[t][r]) ^ sb);
        }
      }
    } else {
      load_tailk<DT>(tk, fwv, fcv, dofs, NTp, w, lane);
    }
    // VNet's evaluation for the next step's first half-update rides beside this step's second one (tail_fast2 above; f16x2 with
    // resident tails; -DL2HMC_FAST_SERIAL_TAILS: four tails per step, one after the other)
#ifndef L2HMC_FAST_SERIAL_TAILS
#ifndef L2HMC_FAST_PAIR_DT2
#define L2HMC_FAST_PAIR_DT2 0
#endif
    constexpr bool PAIR = F16 && RT && (DT == 1 || L2HMC_FAST_PAIR_DT2);      // (DT = 2: measured neutral, profiles/r06_paired_tails.txt)
#else
    constexpr bool PAIR = false;
#endif
    f4 aS_n[DT], T_n[DT], EQ_n[DT];
    if constexpr (PAIR) {
      tail_fast<DT, KH>(tk, pv[0] + tbv, [&](int t, f4 aS, f4 T, f4 EQ) { aS_n[t] = aS; T_n[t] = T; EQ_n[t] = EQ; });
    }
    // one leapfrog step.  LAST (paired tails only): a proposal's last step, which has no next step to look ahead to
    auto step = [&](auto LASTC, bool wantU) {
      constexpr bool LAST = decltype(LASTC)::value;
      f4 k1[DT], vh[DT], y[DT], xin[DT];
      f4 upr[REC1 ? DT : 1];
      const f4 tbx = lds4(rec);
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        if constexpr (PIPE) k1[t] = k1_c[t];
        else k1[t] = k1_of(rec, t);
        if constexpr (REC1) upr[t] = lds4(rec + 48 + 64 * t);
      }
      rec += drec;
      const f4 tbv_n = lds4(rec + 16);      // (the last step reads the unused pad row)
      if constexpr (PIPE && !LAST) {
#pragma unroll
        for (int t = 0; t < DT; ++t) k1_c[t] = k1_of(rec, t);      // (k1 holds this step's; read ahead as tbv_n)
      }

      PT_MARK(1);  // step head
      // ---- momentum half-update #1: VNet([x, grad U(x), t])  (dynamics.py:118-125 / :162-170)
      f4 ldp[LDW ? DT : 1];      // (LDW: a tail's log-det term, added under the reads of the exchange that follows it -- the same order)
      auto vhalf1 = [&](int t, f4 aS, f4 T, f4 EQ) {
        const f4 ES = ex2_4(aS);
        if constexpr (LDW) ldp[t] = aS;
        else ldv += aS;
        const f4 tr = T - EQ * g[t];
        vh[t] = ES * (nf * tr + v[t]) + ff * tr;
      };
      if constexpr (PAIR) {
#pragma unroll
        for (int t = 0; t < DT; ++t) vhalf1(t, aS_n[t], T_n[t], EQ_n[t]);
      } else {
        tail_fast<DT, KH>(tk, pv[0] + tbv, vhalf1);
      }
      PT_MARK(2);  // VNet tail #1

      // ---- two masked position updates: XNet([v_h, kept * x, t])  (:127-145 / :172-190)
      if constexpr (!RT) load_tailk<DT>(tk, fwx, fcx, dofs, NTp, w, lane);
      if constexpr (!PIPE) {
#pragma unroll
        for (int t = 0; t < DT; ++t) xin[t] = k1[t] * x[t];
      }
      f4 pa, px[1];
      if constexpr (PIPE) {
        pa = l1_part16<DT>(vh, Z, l1h.xa);
        px[0] = pa;
#pragma unroll
        for (int t = 0; t < DT; ++t) px[0] = mfma16x2(l1h.xb[t], xb_c[t], px[0]);      // (l1_part16 on the split formed a step ago)
      } else if constexpr (F16) {
        pa = l1_part16<DT>(vh, Z, l1h.xa);
        px[0] = l1_part16<DT>(xin, pa, l1h.xb);
      } else {
        pa = l1_part<DT, NW>(nullptr, 0, A, w, lane, vh, Z, l1w.xa);
        px[0] = pa + l1_part<DT, NW>(nullptr, NT, A, w, lane, xin, Z, l1w.xb);
      }
      PT_MARK(3);  // XNet layer-1 partials (a, b)
      // (LDW: the exchange in its parts, the held log-det term added while the reads are in flight)
      auto xchg_ldw = [&](auto BC, f4 (&p)[1]) {
        float* P = smem + A.o_P + (XS ? decltype(BC)::value : pb) * (NW * 256);
        xchg_put<NW>(P, p[0], w, lane);
        f4 part[NW];
        xchg_get_issue<NW>(P, lane, part);
#pragma unroll
        for (int t = 0; t < DT; ++t) ldv += ldp[t];
        __builtin_amdgcn_sched_barrier(0);
        p[0] = xchg_get_sum<NW>(part);
        if constexpr (!XS) pb ^= 1;
      };
      if constexpr (LDW) xchg_ldw(std::integral_constant<int, 0>{}, px);
      else if constexpr (XS) xchg_at<NW, 0>(px, A, smem, w, lane);
      else xchg<NW, 1>(px, A, smem, w, lane, pb);
      PT_MARK(4);  // exchange
      tail_fast<DT, KH>(TKX, px[0] + tbx, [&](int t, f4 aS, f4 T, f4 EQ) {
        f4 up;
        if constexpr (REC1) up = upr[t];
        else up = 1.f - k1[t];
        const f4 aSm = up * aS;
        const f4 ES = ex2_4(aSm);
        if constexpr (LDW) ldp[t] = aSm;
        else ldv += aSm;
        const f4 tr = up * (EQ * vh[t] + T);
        y[t] = ES * (nf * tr + x[t]) + ff * tr;
        xin[t] = up * y[t];
      });
      PT_MARK(5);  // XNet tail #1
      f4 py[1];
      if constexpr (F16) py[0] = l1_part16<DT>(xin, pa, l1h.xb);
      else py[0] = pa + l1_part<DT, NW>(nullptr, NT, A, w, lane, xin, Z, l1w.xb);
      PT_MARK(6);  // XNet layer-1 partial (b only)
      if constexpr (LDW) xchg_ldw(std::integral_constant<int, 1>{}, py);
      else if constexpr (XS) xchg_at<NW, 1>(py, A, smem, w, lane);
      else xchg<NW, 1>(py, A, smem, w, lane, pb);
      PT_MARK(7);  // exchange
      tail_fast<DT, KH>(TKX, py[0] + tbx, [&](int t, f4 aS, f4 T, f4 EQ) {
        const f4 aSm = k1[t] * aS;
        const f4 ES = ex2_4(aSm);
        if constexpr (LDW) ldp[t] = aSm;
        else ldv += aSm;
        const f4 tr = k1[t] * (EQ * vh[t] + T);
        x[t] = ES * (nf * tr + y[t]) + ff * tr;
      });
      PT_MARK(8);  // XNet tail #2

      // ---- momentum half-update #2 at the new position  (:147-153 / :192-199)
      if constexpr (!RT) load_tailk<DT>(tk, fwv, fcv, dofs, NTp, w, lane);
      grad(x, g, red[2], wantU);
      pv[0] = vnet_l1(x, g);
      PT_MARK(9);  // grad U + VNet layer-1 partials
      if constexpr (PIPE) {
        float* P = smem + A.o_P + (XS ? 2 : pb) * (NW * 256);
        xchg_put<NW>(P, pv[0], w, lane);
        f4 part[NW];
        xchg_get_issue<NW>(P, lane, part);
        if constexpr (LDW) {
#pragma unroll
          for (int t = 0; t < DT; ++t) ldv += ldp[t];
          if constexpr (LAST) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (!LAST) {
          // (pinned between the reads' issue and the first use of what they return -- the one place of the step where the wave
          //  has nothing else to issue.  In front of the barrier it delays every wave's arrival there: measured slower than not
          //  doing it at all, profiles/sampler_step_pipeline.txt)
#pragma unroll
          for (int t = 0; t < DT; ++t) xb_c[t] = split16<L2HMC_FAST_SPLIT_LAT_L1>(k1_c[t] * x[t]);
          __builtin_amdgcn_sched_barrier(0);
        }
        pv[0] = xchg_get_sum<NW>(part);
        if constexpr (!XS) pb ^= 1;
      } else if constexpr (XS) {
        xchg_at<NW, 2>(pv, A, smem, w, lane);
      } else {
        xchg<NW, 1>(pv, A, smem, w, lane, pb);
      }
      PT_MARK(10); // exchange
      auto vhalf2 = [&](int t, f4 aS, f4 T, f4 EQ) {
        const f4 ES = ex2_4(aS);
        ldv += aS;
        const f4 tr = T - EQ * g[t];
        v[t] = ES * (nf * tr + vh[t]) + ff * tr;
      };
      if constexpr (PAIR) {
        // (the last step takes the single tail: the same operations on the evaluation that is kept, none on one that is dropped)
        if constexpr (!LAST) {
          tail_fast2<DT, KH>(tk, pv[0] + tbv, pv[0] + tbv_n, vhalf2, [&](int t, f4 aS, f4 T, f4 EQ) { aS_n[t] = aS; T_n[t] = T; EQ_n[t] = EQ; });
        } else {
          tail_fast<DT, KH>(tk, pv[0] + tbv, vhalf2);
        }
      } else {
        tail_fast<DT, KH>(tk, pv[0] + tbv, vhalf2);
      }
      PT_MARK(11); // VNet tail #2
      tbv = tbv_n;
    };
    // the last step peeled: no test inside the step loop.  (Diagonal Gaussian only: Rough Well's kernels spill under the two-wave
    // bound as they are -- they hold the start point's gradient -- and the second copy of the step raised that by 24 bytes per lane.)
    if constexpr (PAIR && EK == L2HMC_ENERGY_GAUSS_DIAG) {
      for (int it = 0; it + 1 < A.n_steps; ++it) step(std::false_type{}, false);
      if (A.n_steps > 0) step(std::true_type{}, need_p);
    } else {
      for (int it = 0; it < A.n_steps; ++it) step(std::false_type{}, need_p && it == A.n_steps - 1);
    }
    if constexpr (EK == L2HMC_ENERGY_GAUSS_DIAG) red[2] = diag_U(x, g);
    const float ld = hsum(ldv) * 0.6931471805599453f;   // the log-det was accumulated in log2 units

    // ---- per-proposal epilogue: proposal, log-det, accept probability, MH select -------------------
    const bool last = m == A.M - 1;
    red[3] = 0.f;
#pragma unroll
    for (int t = 0; t < DT; ++t) red[3] += 0.5f * hsum(v[t] * v[t]);
    red[4] = ld;
    const float U_end = red[2];
    if constexpr (F16) {
#pragma unroll
      for (int t = 0; t < DT; ++t) amax_l = fmaxf(amax_l, fmaxf(amax4(x[t]), fmaxf(amax4(v[t]), amax4(g[t]))));
      red[5] = amax_l < L2HMC_F16_STATE_MAX ? 0.f : 1.f;
    }
    chain_allreduce<NW, F16 ? 6 : 5>(red, smem + A.o_red, w, lane);
    if constexpr (F16) {
      if (red[5] > 0.f) {            // outside the f16x2 range: a loud non-result (see L2HMC_F16_STATE_MAX)
        const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
        for (int t = 0; t < DT; ++t) { x[t] = splat(qnan); v[t] = splat(qnan); }
        red[4] = qnan;
      }
    }
    if (!CC && last) {
      store_state<DT, NW>(A.x_out, A, chain, live, w, q, x);
      store_state<DT, NW>(A.v_out, A, chain, live, w, q, v);
    }
    const bool writer = live && w == 0 && lane < 16;
    if (!CC && A.logjac_out != nullptr && writer) A.logjac_out[moff + chain] = red[4];
    if (need_p) {
      const float val = (red[0] + red[1]) - (red[2] + red[3]) + red[4];       // dynamics.py:302-309
      const float p = accept_prob(val);
      if ((CC || A.p_out != nullptr) && writer) A.p_out[moff + chain] = p;
      if (have_u) {
        const bool acc = live && (p - u_m) >= 0.f;                            // sampler.py:53-55
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          x[t] = sel4(acc, x[t], x0[t]);
          if constexpr (KEEP_G0) g[t] = sel4(acc, g[t], g0[t]);
          else g[t] = er.prec[t] * (x[t] - er.mu[t]);
        }
        pv[0] = sel4(acc, pv[0], pv0);
        U_start = acc ? U_end : U_start;
      } else {
        U_start = U_end;
      }
    } else {
      U_start = U_end;
    }
    if (!CC && A.x_hist != nullptr) store_state<DT, NW>(A.x_hist + moff * A.d, A, chain, live, w, q, x);
  }  // proposals
  PT_FLUSH(w, lane);
  store_state<DT, NW>(A.x_next, A, chain, live, w, q, x);
}

}  // namespace l2hmc
