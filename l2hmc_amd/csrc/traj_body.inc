// traj_body.inc -- the body of the general trajectory kernel, included by traj_kernel (LAD = false, L = NULL) and by its ladder
// form traj_ladder_kernel (LAD = true) in l2hmc_kernels.hpp, which declare `A`, `L`, `LAD` and `smem` in front of it.  Every
// ladder addition sits under `if constexpr (LAD)`.  (The body is textually part of each kernel -- not a function both call --
// because the optimiser treats a separately inlined function differently: as a function of its own it changed traj_kernel's
// instruction stream, included here it does not.)
  const int tid = threadIdx.x, lane = tid & 63, nthr = 64 * NW;
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int c = lane & 15, q = lane >> 4;
  const long long chain = (long long)blockIdx.x * 16 + c;
  const bool live = chain < A.N;
  const int NT = A.NT, DP = 16 * NT;
  const bool has_nets = A.packed != nullptr;
  const int NF = net_floats(NT);

  // ---- prologue: stage weights / masks / time table / energy parameters into LDS ----------
  constexpr bool WG = weights_in_global(DT);
  // Layer-1 groups (the first 2 NT groups of each net) go straight from global memory into
  // registers when L1W is resident, so only the rest of each net is staged in LDS.
  const int skip = (L1W<DT>::RES && !WG) ? 2 * NT * 256 : 0;      // floats not staged per net
  if (has_nets && !WG) {
    const int per = (NF - skip) / 4;
    f4* dst = reinterpret_cast<f4*>(smem);
    for (int i = tid; i < 2 * per; i += nthr) {
      const int net = i >= per, j = i - net * per;
      dst[i] = reinterpret_cast<const f4*>(A.packed + (size_t)net * NF + skip)[j];
    }
  }
  for (int i = tid; i < A.T * DP; i += nthr) {
    const int row = i / DP, dim = i % DP;
    smem[A.o_mask + i] = dim < A.d ? A.masks[row * A.d + dim] : 0.f;
  }
  for (int i = tid; i < 2 * A.T; i += nthr) smem[A.o_trig + i] = A.trig[i];
  stage_energy<EK, weights_in_global(DT)>(A, smem, tid, nthr);

  f4 x[DT], v[DT], g[DT];
  load_state<DT, NW>(A.x, A, chain, live, w, q, x);
  const float eps = A.alpha != nullptr ? expf(*A.alpha) : A.eps_host;
  const float heps = 0.5f * eps;
  const bool need_p = A.p_out != nullptr || A.x_next != nullptr || A.u != nullptr ||
                      (A.rng_flags & L2HMC_RNG_U) != 0;
  float* LT = nullptr;
  int* LI = nullptr;
  if constexpr (LAD) {
    LT = smem + L->o_lad;
    LI = reinterpret_cast<int*>(LT);
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) LT[LAD_TEMP + i] = L->temp[i];
      LI[LAD_FLAG] = 0;
    }
    if (tid < 16) {
      const long long row = (long long)blockIdx.x * 16 + tid;
      const bool lv = row < A.N;
      LI[LAD_LAB + tid] = lv ? (int)L->rung[row] : 0;
      LI[LAD_TRIP + tid] = (lv && L->trip != nullptr) ? (int)L->trip[row] : 0;
      LI[LAD_ACC + tid] = 0;
      LI[LAD_ATT + tid] = 0;
    }
  }
  __syncthreads();
  // ladder mode: this row's rung label and temperature (constant within a round)
  int lab_row = 0;
  float temp_row = 1.f, Uraw_start = 0.f, Uraw_end = 0.f;
  if constexpr (LAD) {
    lab_row = LI[LAD_LAB + c];
    temp_row = LT[LAD_TEMP + lab_row];
  }

  // bases such that `base + group * 256` addresses group `group` (the skipped layer-1 groups lie
  // before the staged region and are never dereferenced through these)
  const float* wx = WG ? A.packed : smem - skip;                    // XNet fragments
  const float* wv = WG ? A.packed + NF : smem + (NF - skip) - skip;  // VNet fragments
  if (has_nets) {
    // time-embedding table TB[net][row s][unit row i] = W3[0,u] cos_s + W3[1,u] sin_s + b1+b2+b3
    // from the packed tau fragment (lane (i, q): q = 0 -> W3[0], 1 -> W3[1], 2 -> biases)
    for (int idx = tid; idx < 2 * A.T * 16; idx += nthr) {
      const int net = idx / (A.T * 16), srow = (idx / 16) % A.T, i = idx & 15;
      const float* tf = (net == 0 ? wx : wv) + (2 * NT * 64) * 4;
      const float ct = smem[A.o_trig + 2 * srow], st = smem[A.o_trig + 2 * srow + 1];
      smem[A.o_tb + idx] = fmaf(tf[i * 4], ct, fmaf(tf[(16 + i) * 4], st, tf[(32 + i) * 4]));
    }
    __syncthreads();
  }
  int pb = 0;
  const f4 Z = splat(0.f);
  float U_start;                 // this lane's share of U at the current state
  EnergyRegs<EK, DT> er;
  load_energy_regs<EK, DT, NW>(er, A, smem, w, lane);
  grad_energy<EK, DT, NW, LAD>(A, smem, w, lane, x, g, U_start, need_p, &er, nullptr, temp_row, &Uraw_start);

  // VNet layer-1 partial at the current (x, grad U): shared by the closing half-update of one
  // step and the opening half-update of the next, and kept across proposals.
  TailW<DT> tw;
  L1W<DT> l1w;
  if (has_nets) load_l1w<DT, NW>(l1w, A.packed, A.packed + NF, A, w, lane);
  f4 pv[1] = {Z};
  PT_DECL;
  PT_MARK(0);      // prologue (staging + first grad)
  if (has_nets && A.n_steps > 0) {
    load_tail<DT, NW>(tw, wv, A, w, lane);
    // (two independent accumulators: the MFMA chain is pipe-bound, not latency-bound)
    pv[0] = l1_part<DT, NW>(wv, 0, A, w, lane, x, Z, l1w.va) + l1_part<DT, NW>(wv, NT, A, w, lane, g, Z, l1w.vb);
    xchg<NW, 1>(pv, A, smem, w, lane, pb);
  }

  // ---- persistent sampler loop: M proposals per launch (M = 1: a single trajectory) ---------
  // This proposal's draws (momenta, direction bit, accept uniform): either injected from HBM --
  // then fetched one proposal ahead so the latency hides under the current trajectory -- or
  // drawn in-kernel from the counter-based Philox stream.
  const long long gchain = A.chain_off + chain;
  const bool rng_v = (A.rng_flags & L2HMC_RNG_V) != 0, rng_d = (A.rng_flags & L2HMC_RNG_DIR) != 0;
  const bool rng_u = (A.rng_flags & L2HMC_RNG_U) != 0;
  f4 vn[DT];
  if (!rng_v) load_state<DT, NW>(A.v, A, chain, live, w, q, vn);
  bool fwd_n = (A.dir != nullptr && !rng_d) ? (live ? A.dir[chain] != 0 : true) : (A.dir_all != 0);
  float u_n = (A.u != nullptr && !rng_u && live) ? A.u[chain] : 0.f;
  const bool have_u = A.u != nullptr || rng_u;
  // AIS mode (utils/ais.py:43-66, HMC transitions): per proposal the bridge moves to beta = ais_beta[m], the
  // log-weight takes dbeta (|x|^2/2 - U_final(x)) at the CURRENT state, the momentum is drawn fresh or partially
  // refreshed, and a rejected chain keeps its state with the NEGATED PROPOSED momentum (ais.py:63).
  const bool ais = A.ais_beta != nullptr;
  float ais_wacc = 0.f, ais_aacc = 0.f, beta_m = A.beta;
  f4 vprev[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) vprev[t] = Z;
  if (ais && A.ais_refresh >= 0.f) {
    if (A.ais_v0 != nullptr) load_state<DT, NW>(A.ais_v0, A, chain, live, w, q, vprev);
    else rng_state<DT, NW>(A, gchain, A.rng_prop0 - 1, w, q, vprev);
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
  if (ais) {
    beta_m = A.ais_beta[m];
    const float one = 1.f;
    float pr[2];
    grad_energy<EK, DT, NW>(A, smem, w, lane, x, g, pr[0], true, &er, &one);      // U_final, grad U_final at x
    pr[1] = 0.f;
#pragma unroll
    for (int t = 0; t < DT; ++t) pr[1] += 0.5f * hsum(x[t] * x[t]);
    U_start = (1.f - beta_m) * pr[1] + beta_m * pr[0];                              // this lane's share of U_beta(x)
#pragma unroll
    for (int t = 0; t < DT; ++t) g[t] = x[t] * (1.f - beta_m) + g[t] * beta_m;
    chain_allreduce<NW, 2>(pr, smem + A.o_red, w, lane);
    ais_wacc += A.ais_dbeta * (-pr[0] + pr[1]);                                     // ais.py:58-59
    if (A.ais_refresh >= 0.f) {                                                     // ais.py:55
      const float keep = sqrtf(1.f - A.ais_refresh), mix = sqrtf(A.ais_refresh);
#pragma unroll
      for (int t = 0; t < DT; ++t) v[t] = vprev[t] * keep + v[t] * mix;
    }
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
  const float sgn = fwd ? 1.f : -1.f;
  // the start point: a rejected chain resumes from it (sampler.py:53-55)
  f4 x0[DT], g0[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) { x0[t] = x[t]; g0[t] = g[t]; }
  const f4 pv0 = pv[0];
  float red[5];                  // U0, K0, U1, K1, logdet (per-lane partial sums)
  red[0] = U_start;
  red[1] = 0.f;
#pragma unroll
  for (int t = 0; t < DT; ++t) red[1] += 0.5f * hsum(v[t] * v[t]);
  red[2] = 0.f;
  f4 ldv = splat(0.f);

  // folded constants: sgn eps log2(e) scales S of XNet, sgn (eps/2) log2(e) S of VNet, eps log2(e) Q
  const float LOG2E = 1.4426950408889634f;
  const float kSx = sgn * eps * LOG2E, kSv = sgn * heps * LOG2E, kQ = eps * LOG2E;
  const f4 O = splat(1.f);

  // schedule row of this chain at iteration `it`: forward chains walk 0..T-1, backward T-1..0
  auto row_of = [&](int it) { const int sf = A.step_begin + it; return fwd ? sf : (A.T - 1 - sf); };
  // time-embedding terms (XNet, VNet) and the first-kept mask of that row; all are PREFETCHED
  // one step ahead so their LDS latency never sits on the critical path
  auto tbx_of = [&](int s) { return lds4(smem + A.o_tb + s * 16 + 4 * q); };
  auto tbv_of = [&](int s) { return lds4(smem + A.o_tb + (A.T + s) * 16 + 4 * q); };
  auto mask_of = [&](int s, f4 (&k)[DT]) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const bool ok = (w * DT + t) < NT;
      const f4 m = ok ? lds4(smem + A.o_mask + s * DP + 16 * (w * DT + t) + 4 * q) : Z;
      k[t] = sel4(fwd, m, O - m);             // forward keeps m first, backward keeps 1-m first
    }
  };
  f4 k1[DT], k1n[DT];
  f4 tbx = Z, tbv = Z, tbxn = Z, tbvn = Z;
  if (A.n_steps > 0) {
    if (has_nets) { tbx = tbx_of(row_of(0)); tbv = tbv_of(row_of(0)); }
    mask_of(row_of(0), k1);
  }

  for (int it = 0; it < A.n_steps; ++it) {
    f4 xin[DT], y[DT], vh[DT];
    if (it + 1 < A.n_steps) {                 // prefetch the next step's schedule row
      if (has_nets) { tbxn = tbx_of(row_of(it + 1)); tbvn = tbv_of(row_of(it + 1)); }
      mask_of(row_of(it + 1), k1n);
    }

    if (has_nets) {
      PT_MARK(1);  // step head
      // ---- momentum half-update #1: VNet([x, grad U(x), t])  (dynamics.py:118-125 / :162-170)
      net_tail<DT, KH>(tw, pv[0], tbv, kSv, kQ, [&](int t, f4 ES, f4 aS, f4 T, f4 EQ) {
        vh[t] = v_half(v[t], g[t], ES, aS, T, EQ, heps, fwd, ldv);
      });
      PT_MARK(2);  // VNet tail #1

      // ---- two masked position updates: XNet([v_h, kept * x, t])  (:127-145 / :172-190);
      //      the v_h contraction is shared by both
      load_tail<DT, NW>(tw, wx, A, w, lane);
#pragma unroll
      for (int t = 0; t < DT; ++t) xin[t] = k1[t] * x[t];
      // the v_h contraction `pa` is computed once and enters both exchanges un-summed, so every
      // exchange carries ONE partial vector per wave
      const f4 pa = l1_part<DT, NW>(wx, 0, A, w, lane, vh, Z, l1w.xa);
      f4 px[1];
      px[0] = pa + l1_part<DT, NW>(wx, NT, A, w, lane, xin, Z, l1w.xb);
      PT_MARK(3);  // XNet layer-1 partials (a, b)
      xchg<NW, 1>(px, A, smem, w, lane, pb);
      PT_MARK(4);  // exchange
      net_tail<DT, KH>(tw, px[0], tbx, kSx, kQ, [&](int t, f4 ES, f4 aS, f4 T, f4 EQ) {
        y[t] = x_half(x[t], k1[t], vh[t], ES, aS, T, EQ, eps, fwd, ldv);
      });
      PT_MARK(5);  // XNet tail #1
#pragma unroll
      for (int t = 0; t < DT; ++t) xin[t] = (O - k1[t]) * y[t];
      f4 py[1];
      py[0] = pa + l1_part<DT, NW>(wx, NT, A, w, lane, xin, Z, l1w.xb);
      PT_MARK(6);  // XNet layer-1 partial (b only)
      xchg<NW, 1>(py, A, smem, w, lane, pb);
      PT_MARK(7);  // exchange
      net_tail<DT, KH>(tw, py[0], tbx, kSx, kQ, [&](int t, f4 ES, f4 aS, f4 T, f4 EQ) {
        x[t] = x_half(y[t], O - k1[t], vh[t], ES, aS, T, EQ, eps, fwd, ldv);
      });
      PT_MARK(8);  // XNet tail #2

      // ---- momentum half-update #2 at the new position  (:147-153 / :192-199); its layer-1
      //      partial is reused by half-update #1 of the next step
      load_tail<DT, NW>(tw, wv, A, w, lane);
      grad_energy<EK, DT, NW, LAD>(A, smem, w, lane, x, g, red[2], need_p && it == A.n_steps - 1, &er, nullptr, temp_row,
                                   &Uraw_end);
      pv[0] = l1_part<DT, NW>(wv, 0, A, w, lane, x, Z, l1w.va) + l1_part<DT, NW>(wv, NT, A, w, lane, g, Z, l1w.vb);
      PT_MARK(9);  // grad U + VNet layer-1 partials
      xchg<NW, 1>(pv, A, smem, w, lane, pb);
      PT_MARK(10); // exchange
      net_tail<DT, KH>(tw, pv[0], tbv, kSv, kQ, [&](int t, f4 ES, f4 aS, f4 T, f4 EQ) {
        v[t] = v_half(vh[t], g[t], ES, aS, T, EQ, heps, fwd, ldv);
      });
      PT_MARK(11); // VNet tail #2
    } else {
      // HMC mode: S = T = Q = 0 (dynamics.py:73-76)
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        vh[t] = v_half(v[t], g[t], O, Z, Z, O, heps, fwd, ldv);
        y[t] = x_half(x[t], k1[t], vh[t], O, Z, Z, O, eps, fwd, ldv);
        x[t] = x_half(y[t], O - k1[t], vh[t], O, Z, Z, O, eps, fwd, ldv);
      }
      grad_energy<EK, DT, NW, LAD>(A, smem, w, lane, x, g, red[2], need_p && it == A.n_steps - 1, &er, &beta_m, temp_row,
                                   &Uraw_end);
#pragma unroll
      for (int t = 0; t < DT; ++t) v[t] = v_half(vh[t], g[t], O, Z, Z, O, heps, fwd, ldv);
    }
    tbx = tbxn;
    tbv = tbvn;
#pragma unroll
    for (int t = 0; t < DT; ++t) k1[t] = k1n[t];
  }
  const float ld = hsum(ldv) * 0.6931471805599453f;   // the log-det was accumulated in log2 units

  // ---- per-proposal epilogue: proposal, log-det, accept probability, MH select ---------------
  const bool last = m == A.M - 1;
  if (last) {
    store_state<DT, NW>(A.x_out, A, chain, live, w, q, x);
    store_state<DT, NW>(A.v_out, A, chain, live, w, q, v);
  }
  if (A.n_steps == 0) red[2] = red[0];
  if constexpr (LAD) {
    if (A.n_steps == 0) Uraw_end = Uraw_start;
  }
  red[3] = 0.f;
#pragma unroll
  for (int t = 0; t < DT; ++t) red[3] += 0.5f * hsum(v[t] * v[t]);
  red[4] = ld;
  const float U_end = red[2];
  chain_allreduce<NW, 5>(red, smem + A.o_red, w, lane);
  const bool writer = live && w == 0 && lane < 16;
  if (A.logjac_out != nullptr && writer) A.logjac_out[moff + chain] = red[4];
  if (need_p) {
    // dynamics.py:302-309
    const float e_new = red[2] + red[3], e_old = red[0] + red[1];
    const float val = e_old - e_new + red[4];
    const float p = accept_prob(val);
    if (A.p_out != nullptr && writer) A.p_out[moff + chain] = p;
    if (have_u) {
      const bool acc = live && (p - u_m) >= 0.f;                      // sampler.py:53-55
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        x[t] = sel4(acc, x[t], x0[t]);
        g[t] = sel4(acc, g[t], g0[t]);
      }
      pv[0] = sel4(acc, pv[0], pv0);
      U_start = acc ? U_end : U_start;
      if constexpr (LAD) Uraw_start = acc ? Uraw_end : Uraw_start;
      if (ais) {
        ais_aacc += p;
#pragma unroll
        for (int t = 0; t < DT; ++t) vprev[t] = acc ? v[t] : -v[t];
      }
    } else {
      U_start = U_end;
    }
  } else {
    U_start = U_end;
  }
  if (A.x_hist != nullptr) store_state<DT, NW>(A.x_hist + moff * A.d, A, chain, live, w, q, x);
  if constexpr (LAD) {
    const int K = L->K;
    const long long nlad = A.N / K;
    if ((m + 1) % L->M == 0) {
      // ---- the round's swap sweep: raw U of every row to LDS, one lane per ladder runs the deterministic even-odd sweep
      const long long jr = m / L->M;                        // round within this launch
      const unsigned long long gr = L->round0 + (unsigned long long)jr;
      float ur[1] = {Uraw_start};
      chain_allreduce<NW, 1>(ur, smem + A.o_red, w, lane);
      if (w == 0 && lane < 16) LT[LAD_U + c] = ur[0];
      __syncthreads();
      if (w == 0 && lane < 16 && c % K == 0 && live) {
        int* lab = LI + LAD_LAB + c;                           // this ladder's K rows
        int* inv = LI + LAD_INV + c;
        int* trip = LI + LAD_TRIP + c;
        const float* Ur = LT + LAD_U + c;
        const long long lloc = chain / K, glad = (A.chain_off + chain) / K;
        for (int i = 0; i < K; ++i) inv[lab[i]] = i;
        bool moved = false;
        for (int k = (int)(gr & 1); k + 1 < K; k += 2) {
          const int a = inv[k], b = inv[k + 1];
          const float uu = L->u != nullptr ? L->u[(jr * nlad + lloc) * (K / 2) + (k >> 1)]
                                              : philox_swap_u(A.rng_seed, glad, gr, k);
          const float db = 1.f / LT[LAD_TEMP + k] - 1.f / LT[LAD_TEMP + k + 1];
          const bool ok = logf(uu) < db * (Ur[a] - Ur[b]);    // (a NaN on either side rejects)
          atomicAdd(&LI[LAD_ATT + k], 1);
          if (ok) {
            atomicAdd(&LI[LAD_ACC + k], 1);
            lab[a] = k + 1;
            lab[b] = k;
            moved = moved || LT[LAD_TEMP + k] != LT[LAD_TEMP + k + 1];
          }
        }
        // round trips: a row that reached rung K - 1 since it last left rung 0 completes one when it is back at rung 0
        int trips = 0;
        for (int i = 0; i < K; ++i) {
          const int lb = lab[i];
          if (lb == K - 1) trip[i] = 1;
          else if (lb == 0) { trips += trip[i]; trip[i] = 0; }
        }
        if (trips != 0 && L->trips != nullptr) L->trips[lloc] += trips;
        if (moved) LI[LAD_FLAG] = 1;
      }
      __syncthreads();
      const int lb = LI[LAD_LAB + c];
      const float tn = LT[LAD_TEMP + lb];
      const bool redo = LI[LAD_FLAG] != 0;                     // (workgroup-uniform)
      __syncthreads();
      if (tid == 0) LI[LAD_FLAG] = 0;
      if (L->rung_hist != nullptr && w == 0 && lane < 16 && live) L->rung_hist[jr * A.N + chain] = (signed char)lb;
      if (redo) {
        // some row of the tile changed temperature: grad U / T, U / T and the VNet layer-1 partial at the new rung (rows whose
        // temperature stayed keep theirs, so equal rungs never come here)
        const bool ch = tn != temp_row;
        f4 gn[DT];
        float Un, Urn;
        grad_energy<EK, DT, NW, LAD>(A, smem, w, lane, x, gn, Un, true, &er, nullptr, tn, &Urn);
#pragma unroll
        for (int t = 0; t < DT; ++t) g[t] = sel4(ch, gn[t], g[t]);
        U_start = ch ? Un : U_start;
        if (has_nets && A.n_steps > 0) {
          f4 pn[1] = {l1_part<DT, NW>(wv, 0, A, w, lane, x, Z, l1w.va) + l1_part<DT, NW>(wv, NT, A, w, lane, gn, Z, l1w.vb)};
          xchg<NW, 1>(pn, A, smem, w, lane, pb);
          pv[0] = sel4(ch, pn[0], pv[0]);
        }
      }
      lab_row = lb;
      temp_row = tn;
    }
    if (L->cold != nullptr && lab_row == 0)
      store_state<DT, NW>(L->cold + moff / K * A.d, A, chain / K, live, w, q, x);
  }
  }  // proposals

  PT_FLUSH(w, lane);
  store_state<DT, NW>(A.x_next, A, chain, live, w, q, x);
  if (ais && live && w == 0 && lane < 16) {
    if (A.ais_w != nullptr) A.ais_w[chain] += ais_wacc;
    if (A.ais_alpha != nullptr) A.ais_alpha[chain] += ais_aacc;
  }
  if constexpr (LAD) {
    if (w == 0 && lane < 16 && live) {
      L->rung[chain] = (signed char)lab_row;
      if (L->trip != nullptr) L->trip[chain] = (signed char)LI[LAD_TRIP + c];
    }
    if (tid < L->K - 1) {
      const int na = LI[LAD_ACC + tid], nt = LI[LAD_ATT + tid];
      if (L->acc != nullptr && na != 0) atomicAdd(reinterpret_cast<unsigned long long*>(L->acc + tid), (unsigned long long)na);
      if (L->att != nullptr && nt != 0) atomicAdd(reinterpret_cast<unsigned long long*>(L->att + tid), (unsigned long long)nt);
    }
  }
