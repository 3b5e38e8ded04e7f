// train_split.hpp -- one proposal + the gradient of its loss term ON THE GEMM ENGINE: the training step for
// samplers the register-resident training kernels (train.hip) cannot hold -- S/T/Q nets of any width H, the shared
// image branch `encoder_sampler(aux)` and the VAE latent-posterior energy (mnist_vae.py:104-226: BASELINE.json
// config 5's "trained sampler"), and the built-in targets with wide nets (SCGExperiment.ipynb `network`, H != 10).
// Included at the end of split.hip (same translation unit: it reuses the forward kernels and the decoder GEMMs).
//
//   loss term   v1_n = sum_k w_nk (Lx_nk - x_nk)^2 p_n + 1e-4;   term = scale mean_n(1 / v1_n) - mean_n(v1_n) / scale
//     w = 1, scale = 0.1: SCGExperiment.ipynb raw 164-169 / utils/losses.py:53-59;
//     w = 1 / (sigma_q^2 + 1e-4), scale = 1: mnist_vae.py:207-214 (energy_scale = 0, the default).
//   gradient w.r.t. XNet, VNet, alpha (as d/d eps) and the image branch; optionally the cotangent a later proposal sends
//   into Lx comes in (dLx_in) and d loss / d x goes out (dx0_out): mnist_vae.py:185-224 chains MH proposals without
//   stop_gradient.
//
// MI355X-first: nothing is recomputed and nothing is checkpointed sparsely -- with 288 GB of HBM the forward pass simply
// keeps every net evaluation's inputs, both hidden activations and head products (4 T evaluations x N chains, 0.75 GB at
// config 5), the reverse sweep leaves the three pre-activation cotangents of every evaluation next to them, and each
// weight matrix's gradient is then ONE contraction over all (evaluation, chain) rows (gemm_tn_kernel, K = 2 T N) instead
// of 4 T small ones.  The reverse sweep itself is, per net evaluation, one adjoint kernel of the leapfrog update (the
// formulas of train.hip's v_half_bwd / x_half_bwd) and three NT GEMMs (d z -> d h2 -> d h1 -> d inputs, relu masks fused
// into the epilogues); the path through grad U is a Hessian-vector product: elementwise for the diagonal Gaussian and the
// Rough Well, a (d x d) product for the dense Gaussian, and for the decoder posterior forward-over-reverse through the
// decoder: 3 tangent GEMMs + 3 reverse-tangent GEMMs around the 5 GEMMs that rebuild the point's activations, the
// softplus'' terms fused into the epilogues (EPI_TAN).  No atomics anywhere: every sum over chains is chunked and added
// in chunk order, so the gradient is bitwise reproducible.
#pragma once

namespace l2hmc {

// flat parameter layout of one net == NET_FIELDS order of include/l2hmc.h (the same as train.hip's)
struct SNetOff { long long W1, b1, W2, b2, W3, b3, W4, b4, Ws, bs, Wt, bt, Wq, bq, ls, lq, total; };
inline SNetOff snet_off(int d, int H) {
  SNetOff o;
  long long p = 0;
  o.W1 = p; p += (long long)d * H; o.b1 = p; p += H; o.W2 = p; p += (long long)d * H; o.b2 = p; p += H;
  o.W3 = p; p += 2 * H; o.b3 = p; p += H; o.W4 = p; p += (long long)H * H; o.b4 = p; p += H;
  o.Ws = p; p += (long long)H * d; o.bs = p; p += d; o.Wt = p; p += (long long)H * d; o.bt = p; p += d;
  o.Wq = p; p += (long long)H * d; o.bq = p; p += d; o.ls = p; p += d; o.lq = p; p += d;
  o.total = p;
  return o;
}
inline long long mlp3_params(const L2hmcMlp3& m) {
  return (long long)m.n_in * m.n_h1 + m.n_h1 + (long long)m.n_h1 * m.n_h2 + m.n_h2 + (long long)m.n_h2 * m.n_out + m.n_out;
}

// ---- adjoint of k_v_half (train.hip v_half_bwd).  out3 holds the head products on entry and the cotangents of the
// three head PRE-activations (d zs | d zt | d zq) on exit; DL = (dS S | dQ Q): its column sums are d lam_s, d lam_q.
__global__ __launch_bounds__(256) void k_tv_half_bwd(float* out3, L2hmcNet w, const float* vin, int ldvi, const float* g,
                                                     int ldg, const float* dout, float* dvin, float* dg, float* DL,
                                                     const float* lam, float* deps, const unsigned char* dir, int dir_all,
                                                     const float* alpha, float eps_host, long long N, int d) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  const bool fwd = dir != nullptr ? dir[n] != 0 : (dir_all != 0);
  const float eps = alpha != nullptr ? expf(*alpha) : eps_host, heps = 0.5f * eps, sg = fwd ? 1.f : -1.f;
  const float lm = lam[n];
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) {
    float* o = out3 + n * 3 * d;
    // (w.lam_s == NULL: out3 holds the FINAL S | T | Q of a caller-supplied net on entry and their cotangents on exit,
    //  L2hmcNetVjpCallback; DL is not written)
    const bool raw = w.lam_s == nullptr;
    const float els = raw ? 1.f : expf(w.lam_s[k]), elq = raw ? 1.f : expf(w.lam_q[k]);
    const float ts = raw ? o[k] : tanhf(o[k] + w.bs[k]), Tt = raw ? o[d + k] : o[d + k] + w.bt[k],
                tq = raw ? o[2 * d + k] : tanhf(o[2 * d + k] + w.bq[k]);
    const float S = els * ts, Q = elq * tq;
    const float ES = expf(sg * heps * S), EQ = expf(eps * Q);
    const float gq = g[n * ldg + k], vi = vin[n * ldvi + k];
    const float cc = heps * (Tt - EQ * gq);
    const float dO = dout[n * d + k];
    const float dES = fwd ? dO * vi : dO * (vi - cc);
    const float dcc = fwd ? dO : -dO * ES;
    const float ds = dES * ES + lm;
    const float dSr = ds * sg * heps;
    const float dq = -dcc * heps * gq * EQ;
    const float dQr = dq * eps;
    dvin[n * d + k] = dO * ES;
    dg[n * d + k] = -dcc * heps * EQ;
    if (!raw) {
      DL[n * 2 * d + k] = dSr * S;
      DL[n * 2 * d + d + k] = dQr * Q;
    }
    o[k] = raw ? dSr : dSr * els * (1.f - ts * ts);
    o[d + k] = dcc * heps;
    o[2 * d + k] = raw ? dQr : dQr * elq * (1.f - tq * tq);
    acc += ds * sg * 0.5f * S + dcc * 0.5f * (Tt - EQ * gq) + dq * Q;
  }
  acc = wave_sum(acc);
  if (lane == 0) deps[n] += acc;
}

// ---- adjoint of k_x_half (train.hip x_half_bwd): dzin_out = direct part of d zin, dvh += ...
__global__ __launch_bounds__(256) void k_tx_half_bwd(float* out3, L2hmcNet w, const float* zin, int ldzi, const float* vh,
                                                     int ldvh, const float* dout, float* dzin_out, float* dvh, float* DL,
                                                     const float* lam, float* deps, const float* masks,
                                                     const unsigned char* dir, int dir_all, int it, int T, int second,
                                                     const float* alpha, float eps_host, long long N, int d) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  bool fwd;
  const int s = row_of(dir, dir_all, n, it, T, fwd);
  const float eps = alpha != nullptr ? expf(*alpha) : eps_host, sg = fwd ? 1.f : -1.f;
  const float lm = lam[n];
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) {
    float* o = out3 + n * 3 * d;
    const float m = masks[s * d + k];
    const float k1 = fwd ? m : 1.f - m;
    const float kp = second ? 1.f - k1 : k1, up = 1.f - kp;
    const bool raw = w.lam_s == nullptr;           // (a caller-supplied net's final S | T | Q: see k_tv_half_bwd)
    const float els = raw ? 1.f : expf(w.lam_s[k]), elq = raw ? 1.f : expf(w.lam_q[k]);
    const float ts = raw ? o[k] : tanhf(o[k] + w.bs[k]), Tt = raw ? o[d + k] : o[d + k] + w.bt[k],
                tq = raw ? o[2 * d + k] : tanhf(o[2 * d + k] + w.bq[k]);
    const float S = els * ts, Q = elq * tq;
    const float ES = expf(sg * eps * S), EQ = expf(eps * Q);
    const float vhq = vh[n * ldvh + k], zi = zin[n * ldzi + k];
    const float tr = eps * (EQ * vhq + Tt);
    const float dO = dout[n * d + k];
    const float dnw = up * dO;
    const float dES = fwd ? dnw * zi : dnw * (zi - tr);
    const float dtr = fwd ? dnw : -dnw * ES;
    const float dsx = dES * ES + up * lm;
    const float dSr = dsx * sg * eps;
    const float dq = dtr * eps * vhq * EQ;
    const float dQr = dq * eps;
    dzin_out[n * d + k] = kp * dO + dnw * ES;
    dvh[n * d + k] += dtr * eps * EQ;
    if (!raw) {
      DL[n * 2 * d + k] = dSr * S;
      DL[n * 2 * d + d + k] = dQr * Q;
    }
    o[k] = raw ? dSr : dSr * els * (1.f - ts * ts);
    o[d + k] = dtr * eps;
    o[2 * d + k] = raw ? dQr : dQr * elq * (1.f - tq * tq);
    acc += dsx * sg * S + dtr * (EQ * vhq + Tt) + dq * Q;
  }
  acc = wave_sum(acc);
  if (lane == 0) deps[n] += acc;
}

// after an XNet evaluation's input cotangents dAB = (d a | d b):  dvh += d a;  tgt += kept-mask * d b
// (the net saw b = k1 x on the first position update and (1 - k1) y on the second)
__global__ void k_comb_x(const float* dAB, float* dvh, float* tgt, const float* masks, const unsigned char* dir,
                         int dir_all, int it, int T, int second, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  bool fwd;
  const int s = row_of(dir, dir_all, n, it, T, fwd);
  const float m = masks[s * d + k];
  const float k1 = fwd ? m : 1.f - m;
  dvh[i] += dAB[n * 2 * d + k];
  tgt[i] += (second ? 1.f - k1 : k1) * dAB[n * 2 * d + d + k];
}
// VNet evaluation at (x, grad U(x)):  u = dg + d b  is the vector of the Hessian-vector product ...
// (+ the vector parked by the point's other VNet evaluation, see through_grad)
__global__ void k_comb_v1(const float* dg, const float* dAB, const float* carry, float* u, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  float a = dg[i] + dAB[(i / d) * 2 * d + d + (i % d)];
  if (carry != nullptr) a += carry[i];
  u[i] = a;
}
// ... and  lx += d a + Hessian(x) u
__global__ void k_comb_v2(float* lx, const float* dAB, const float* hv, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  lx[i] += dAB[(i / d) * 2 * d + (i % d)] + (hv != nullptr ? hv[i] : 0.f);
}

// Hessian-vector products of the built-in targets (oracle/l2hmc_train_oracle.py *Target.hessvec): diagonal Gaussian
// P u; Rough Well (1 - (eta / den^2) cos(x / den)) u; dense Gaussian G u with G = (S + S^T) / 2 of the RAW precision
// (it = 1 / temperature: the products of U / temperature)
__global__ void k_hvp_builtin(int kind, const float* x, int ldx, const float* u, float* hv, const float* prec,
                              const float* hess, float eta, float den, float it, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  float o;
  if (kind == L2HMC_ENERGY_GAUSS_DIAG) {
    o = prec[k] * u[i];
  } else if (kind == L2HMC_ENERGY_ROUGHWELL) {
    o = (1.f - (eta / (den * den)) * cosf(x[n * ldx + k] / den)) * u[i];
  } else {
    o = 0.f;
    for (int j = 0; j < d; ++j) o += 0.5f * (hess[k * d + j] + hess[j * d + k]) * u[n * d + j];
  }
  hv[i] = o * it;
}

// Hessian-vector products that couple the dimensions of a chain (oracle/l2hmc_train_oracle.py GMMTarget / FunnelTarget
// .hessvec); one thread per chain -- these targets live in a handful of dimensions.
//   mixture (distributions.py:104-134): y_i = G_i (x - mu_i), w = softmax_i(-(x - mu_i)^T S_i (x - mu_i) / 2 + logc_i),
//     g = sum_i w_i y_i,   H u = sum_i w_i (G_i u - y_i (y_i . u)) + g (g . u);   G_i = (S_i + S_i^T) / 2 of the RAW S_i
//   funnel (distributions.py:155-180), s = e^{x_0} (constant on the clipped branches), q = sum_{k>=1} x_k^2:
//     (H u)_k = u_k / s - [free] x_k u_0 / s,   (H u)_0 = u_0 (1 / sigma^2 + [free] q / (2 s)) - [free] sum_k x_k u_k / s
constexpr int HVP_MAXC = 32;
//   (it = 1 / temperature multiplies the finished product -- never the mixture's gradient g, which enters twice)
__global__ void k_hvp_chain(int kind, const float* x, int ldx, const float* u, float* hv, float* gs, const float* mu,
                            const float* hess, const float* logc, int ncomp, float sigma, float it, long long N, int d) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* xr = x + n * ldx;
  const float* ur = u + n * d;
  float* o = hv + n * d;
  if (kind == L2HMC_ENERGY_FUNNEL) {
    const float v = xr[0], clip = 4.f * sigma;
    const bool hi = v > clip, lo = -clip > v;
    const float fr = (hi || lo) ? 0.f : 1.f;
    const float inv_s = 1.f / (hi ? expf(clip) : (lo ? expf(-clip) : expf(v)));
    float q = 0.f, dot = 0.f;
    for (int k = 1; k < d; ++k) { q += xr[k] * xr[k]; dot += xr[k] * ur[k]; }
    for (int k = 1; k < d; ++k) o[k] = (ur[k] * inv_s - fr * xr[k] * ur[0] * inv_s) * it;
    o[0] = (ur[0] * (1.f / (sigma * sigma) + fr * 0.5f * q * inv_s) - fr * dot * inv_s) * it;
    return;
  }
  // mixture: y(c, k) = sum_j G_c[k][j] (x_j - mu_c[j])
  auto Gc = [&](int c, int k, int j) { return 0.5f * (hess[((long long)c * d + k) * d + j] + hess[((long long)c * d + j) * d + k]); };
  auto ycomp = [&](int c, int k) {
    float a = 0.f;
    for (int j = 0; j < d; ++j) a += Gc(c, k, j) * (xr[j] - mu[c * d + j]);
    return a;
  };
  float w[HVP_MAXC];
  float m = -INFINITY;
  for (int c = 0; c < ncomp; ++c) {
    float qf = 0.f;
    for (int k = 0; k < d; ++k) qf += (xr[k] - mu[c * d + k]) * ycomp(c, k);
    w[c] = -0.5f * qf + logc[c];
    m = fmaxf(m, w[c]);
  }
  float sum = 0.f;
  for (int c = 0; c < ncomp; ++c) { w[c] = (w[c] == -INFINITY) ? 0.f : expf(w[c] - m); sum += w[c]; }
  for (int c = 0; c < ncomp; ++c) w[c] /= sum;
  float* g = gs + n * d;                       // scratch row: grad U
  float gu = 0.f;
  for (int k = 0; k < d; ++k) {
    float a = 0.f;
    for (int c = 0; c < ncomp; ++c) a += w[c] * ycomp(c, k);
    g[k] = a;
    gu += a * ur[k];
  }
  for (int k = 0; k < d; ++k) o[k] = g[k] * gu;
  for (int c = 0; c < ncomp; ++c) {
    float yu = 0.f;
    for (int k = 0; k < d; ++k) yu += ycomp(c, k) * ur[k];
    for (int k = 0; k < d; ++k) {
      float Gu = 0.f;
      for (int j = 0; j < d; ++j) Gu += Gc(c, k, j) * ur[j];
      o[k] += w[c] * (Gu - ycomp(c, k) * yu);
    }
  }
  if (it != 1.f)
    for (int k = 0; k < d; ++k) o[k] *= it;
}

// U / temperature and grad U / temperature of a point whose energy was evaluated plain (the decoder posterior): rows of g
// (stride ldg) and, when given, U (double); also the decoder's Hessian-vector products (U = NULL)
__global__ void k_temper(float* g, int ldg, double* U, float it, double itd, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  g[n * ldg + k] *= it;
  if (U != nullptr && k == 0) U[n] *= itd;
}

// accept probability (dynamics.py:302-309), the loss argument and the adjoint seeds of the reverse sweep
// (train.hip "accept probability, loss term and the adjoint seeds"); one wave per chain.
//   es > 0: + es inv_n sum_n (1 / ed_n - ed_n),  ed = (U(Lx) - U(x))^2 p + 1e-4   (mnist_vae.py:214-224, energy_scale)
//     U0 / U1 / g1 are those of U / temperature (what the dynamics and the accept probability see); the energy term is built
//     from the PLAIN U (mnist_vae.py:209 calls the untempered closure): dU = temperature (U1 - U0), and its cotangent on the
//     tempered g1 carries the factor temperature
//   no_accept: a link of chain_operator (sampler.py:57-85, propose(log_jac=True)): no accept probability and no loss
//   term of its own -- the seeds are the caller's cotangents on Lx / Lv / the summed log-Jacobian.
__global__ __launch_bounds__(256) void k_train_seed(const float* x0, const float* x1, int ldx1, const float* v1,
                                                    const float* g1, int ldg1, const double* U0, const double* U1,
                                                    const float* K0, const float* ld, const float* wgt,
                                                    const float* dLx_in, const float* dLv_in, const float* dlj_in,
                                                    int no_accept, float scale, float inv_n, float es, float* Lx,
                                                    float* Lv_out, float* lj_out, float* p_out, float* v1_out,
                                                    float* ed_out, float* lam, float* lamU, float* dv1p_out, float* lx,
                                                    float* lv, float* deps, float temp, long long N, int d) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  if (no_accept) {
    if (lane == 0) {
      lam[n] = dlj_in != nullptr ? dlj_in[n] : 0.f;
      lamU[n] = 0.f;
      dv1p_out[n] = 0.f;
      deps[n] = 0.f;
      if (lj_out != nullptr) lj_out[n] = ld[n];
    }
    for (int k = lane; k < d; k += 64) {
      Lx[n * d + k] = x1[n * ldx1 + k];
      if (Lv_out != nullptr) Lv_out[n * d + k] = v1[n * d + k];
      lx[n * d + k] = dLx_in != nullptr ? dLx_in[n * d + k] : 0.f;
      lv[n * d + k] = dLv_in != nullptr ? dLv_in[n * d + k] : 0.f;
    }
    return;
  }
  float K1 = 0.f, sq = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float vv = v1[n * d + k], dx = x1[n * ldx1 + k] - x0[n * d + k];
    K1 += 0.5f * vv * vv;
    sq += (wgt != nullptr ? wgt[n * d + k] : 1.f) * dx * dx;
  }
  K1 = wave_sum(K1);
  sq = wave_sum(sq);
  const float val = (float)((U0[n] - U1[n]) + ((double)K0[n] - (double)K1) + (double)ld[n]);
  const float p = accept_prob(val);
  const float v1o = sq * p + 1e-4f;
  const float dv1 = (scale * (-1.f / (v1o * v1o)) - 1.f / scale) * inv_n;
  const bool pfin = (val == val) && p > 0.f;          // the finite branch of dynamics.py:309 actually taken
  const bool ok = sq < 3.0e38f;                       // a diverged chain contributes no gradient (train.hip)
  // energy term: ed = dU^2 p + 1e-4
  const float dU = (float)((U1[n] - U0[n]) * (double)temp);
  const bool eok = es > 0.f && ok && fabsf(dU) < 1.0e18f;
  const float ed = eok ? dU * dU * p + 1e-4f : 1.f;
  const float de = eok ? es * inv_n * (-1.f / (ed * ed) - 1.f) : 0.f;
  const float eu = de * 2.f * dU * (p * temp);        // d term / d (U(Lx) / temperature) through dU  (= - ... / d U(x))
  const float lm = (ok && pfin && val < 0.f) ? (dv1 * sq + de * dU * dU) * p : 0.f;
  const float dv1p = ok ? dv1 * p * 2.f : 0.f;
  if (lane == 0) {
    p_out[n] = p;
    v1_out[n] = v1o;
    if (ed_out != nullptr) ed_out[n] = eok ? ed : 0.f;
    if (lj_out != nullptr) lj_out[n] = ld[n];
    lam[n] = lm + (dlj_in != nullptr ? dlj_in[n] : 0.f);
    lamU[n] = lm - eu;
    dv1p_out[n] = dv1p;
    deps[n] = 0.f;
  }
  for (int k = lane; k < d; k += 64) {
    const float xe = x1[n * ldx1 + k];
    Lx[n * d + k] = xe;
    if (Lv_out != nullptr) Lv_out[n * d + k] = v1[n * d + k];
    const float wk = wgt != nullptr ? wgt[n * d + k] : 1.f;
    float a = ok ? dv1p * wk * (xe - x0[n * d + k]) + (eu - lm) * g1[n * ldg1 + k] : 0.f;
    if (dLx_in != nullptr) a += dLx_in[n * d + k];
    lx[n * d + k] = a;
    lv[n * d + k] = (ok ? -lm * v1[n * d + k] : 0.f) + (dLv_in != nullptr ? dLv_in[n * d + k] : 0.f);
  }
}
// d loss / d x0 = the sweep's cotangent + the direct paths through (Lx - x0) and through U(x0) (accept ratio, energy term)
__global__ void k_train_dx0(const float* lx, const float* x0, const float* x1, int ldx1, const float* g0, int ldg0,
                            const float* wgt, const float* lamU, const float* dv1p, float* out, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  const float wk = wgt != nullptr ? wgt[i] : 1.f;
  out[i] = lx[i] - dv1p[n] * wk * (x1[n * ldx1 + k] - x0[i]) + lamU[n] * g0[n * ldg0 + k];
}

// ---- chunked column sums (fixed order): part[chunk][col] = sum over the chunk's rows of A[r][col] ----------------
// block = 16 column quads (64 columns) x 16 row lanes; a thread adds its rows of one column quad (dwordx4 when the
// rows are 16-byte aligned), the 16 row lanes are then added in lane order through LDS.  A streaming read: the
// chunking (colsum_chunks) makes enough blocks to pull it at HBM speed.
template <bool V4>
__global__ __launch_bounds__(256) void k_colsum_part(const float* A, int lda, long long R, int cols,
                                                     long long rows_per_chunk, float* part) {
  __shared__ f4 sm[16][16];
  const int cq = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;
  const long long r0 = (long long)blockIdx.y * rows_per_chunk;
  long long r1 = r0 + rows_per_chunk;
  if (r1 > R) r1 = R;
  f4 s = splat(0.f);
  if (col < cols) {
    if (V4 && col + 3 < cols) {
#pragma unroll 4
      for (long long r = r0 + ry; r < r1; r += 16) s = s + *reinterpret_cast<const f4*>(A + r * lda + col);
    } else if (!V4 && col + 3 < cols && lda % 2 == 0 && (col & 1) == 0 && (reinterpret_cast<size_t>(A) & 7) == 0) {
      typedef float f2 __attribute__((ext_vector_type(2)));        // 8-byte rows (the 3 d = 150 head cotangents): two dwordx2
#pragma unroll 4
      for (long long r = r0 + ry; r < r1; r += 16) {
        const f2 a = *reinterpret_cast<const f2*>(A + r * lda + col), b = *reinterpret_cast<const f2*>(A + r * lda + col + 2);
        s = s + f4{a.x, a.y, b.x, b.y};
      }
    } else {
      for (long long r = r0 + ry; r < r1; r += 16) {
        const float* p = A + r * lda + col;
        s.x += p[0];
        if (col + 1 < cols) s.y += p[1];
        if (col + 2 < cols) s.z += p[2];
        if (col + 3 < cols) s.w += p[3];
      }
    }
  }
  sm[ry][cq] = s;
  __syncthreads();
  if (ry == 0 && col < cols) {
    f4 t = sm[0][cq];
#pragma unroll
    for (int i = 1; i < 16; ++i) t = t + sm[i][cq];
    float* o = part + (long long)blockIdx.y * cols + col;
    o[0] = t.x;
    if (col + 1 < cols) o[1] = t.y;
    if (col + 2 < cols) o[2] = t.z;
    if (col + 3 < cols) o[3] = t.w;
  }
}
// d W3 (2, H): the rows of A = d h1_pre are weighted with the time encoding of their schedule step.  A net's stash is
// (evaluation e, chain n); evaluation e belongs to leapfrog iteration e / 2, whose schedule row depends on the chain's
// direction only: blockIdx.y = e * cpe + (row chunk within the evaluation).  part[blockIdx.y][2][H].
__global__ __launch_bounds__(256) void k_w3_part(const float* A, int H, long long N, int cpe, long long rows_per_chunk,
                                                 const float* trig, int T, const unsigned char* dir, int dir_all,
                                                 float* part) {
  __shared__ f4 sm[2][16][16];
  const int cq = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cq;                 // (H % 4 == 0 is not assumed: tail columns are guarded)
  const int e = blockIdx.y / cpe, ch = blockIdx.y % cpe, it = e >> 1;
  const long long n0 = (long long)ch * rows_per_chunk;
  long long n1 = n0 + rows_per_chunk;
  if (n1 > N) n1 = N;
  const float cf = trig[2 * it], sf = trig[2 * it + 1], cb = trig[2 * (T - 1 - it)], sb = trig[2 * (T - 1 - it) + 1];
  f4 sc = splat(0.f), ss = splat(0.f);
  if (col < H && H % 4 == 0 && (reinterpret_cast<size_t>(A) & 15) == 0) {       // whole quads, 16-byte rows: dwordx4, four rows in flight
#pragma unroll 4
    for (long long n = n0 + ry; n < n1; n += 16) {
      const bool fwd = dir != nullptr ? dir[n] != 0 : (dir_all != 0);
      const f4 a = *reinterpret_cast<const f4*>(A + ((long long)e * N + n) * H + col);
      sc = sc + (fwd ? cf : cb) * a;
      ss = ss + (fwd ? sf : sb) * a;
    }
  } else if (col < H)
    for (long long n = n0 + ry; n < n1; n += 16) {
      const bool fwd = dir != nullptr ? dir[n] != 0 : (dir_all != 0);
      const float* p = A + ((long long)e * N + n) * H + col;
      f4 a = splat(0.f);
      a.x = p[0];
      if (col + 1 < H) a.y = p[1];
      if (col + 2 < H) a.z = p[2];
      if (col + 3 < H) a.w = p[3];
      sc = sc + (fwd ? cf : cb) * a;
      ss = ss + (fwd ? sf : sb) * a;
    }
  sm[0][ry][cq] = sc;
  sm[1][ry][cq] = ss;
  __syncthreads();
  if (ry < 2 && col < H) {
    f4 t = sm[ry][0][cq];
#pragma unroll
    for (int i = 1; i < 16; ++i) t = t + sm[ry][i][cq];
    float* o = part + ((long long)blockIdx.y * 2 + ry) * H + col;
    o[0] = t.x;
    if (col + 1 < H) o[1] = t.y;
    if (col + 2 < H) o[2] = t.z;
    if (col + 3 < H) o[3] = t.w;
  }
}
// dst[i] = sum_e X[e][i] + sum_e V[e][i]  (the image branch feeds the first hidden layer of every evaluation)
__global__ void k_sum_evals(const float* X, const float* V, int n_evals, long long stride, float* dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= stride) return;
  float s = 0.f;
  for (int e = 0; e < n_evals; ++e) s += X[(long long)e * stride + i];
  for (int e = 0; e < n_evals; ++e) s += V[(long long)e * stride + i];
  dst[i] = s;
}
// *dst += sum_n a[n]: one workgroup, strided partial sums combined by a fixed tree
__global__ __launch_bounds__(256) void k_sum_chain(const float* a, long long N, float* dst) {
  __shared__ float sm[256];
  float s = 0.f;
  for (long long n = threadIdx.x; n < N; n += 256) s += a[n];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst += sm[0];
}
// beta sigmoid'(logit) from the BCE epilogue's r = sigmoid(logit) - t:  sigma = r + t
__global__ void k_sigd(const float* r, const float* t, float* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float sg = r[i] + t[i];
  out[i] = sg * (1.f - sg);
}
// [W1; W2] stacked (2 d, H) and [Ws | Wt | Wq] side by side (H, 3 d): the B operands of the input-gradient products
__global__ void k_stack_rows(const float* A, const float* B, long long nA, long long nB, float* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nA) out[i] = A[i];
  else if (i < nA + nB) out[i] = B[i - nA];
}
__global__ void k_heads_side(const float* Ws, const float* Wt, const float* Wq, int H, int d, float* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)H * 3 * d) return;
  const int h = (int)(i / (3 * d)), c = (int)(i % (3 * d)), which = c / d, k = c % d;
  const float* W = which == 0 ? Ws : (which == 1 ? Wt : Wq);
  out[i] = W[(long long)h * d + k];
}

// column sums of A (R x cols) into up to three destinations (b1, b2, b3 of a net receive the same sum) or, with
// jblock > 0, scattered in column blocks of jblock to dst0 + block * jstride (the three head biases, the two log-scales)
__global__ void colsum_reduce_kernel(const float* part, int n_chunks, int cols, float* dst0, float* dst1, float* dst2,
                                     int jblock, long long jstride) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  const float s = sum_chunks(part + j, n_chunks, cols);
  if (jblock > 0) {
    dst0[(long long)(j / jblock) * jstride + (j % jblock)] += s;
  } else {
    dst0[j] += s;
    if (dst1 != nullptr) dst1[j] += s;
    if (dst2 != nullptr) dst2[j] += s;
  }
}
inline void colsum_chunks(long long R, int cols, long long part_cap, int& nc, long long& rpc) {
  long long n = (R + 255) / 256;                       // a streaming read: enough chunks to fill the chip, few enough
  if (n > 128) n = 128;                                // that the fixed-order second stage stays short
  if (n * cols > part_cap) n = part_cap / cols;
  if (n < 1) n = 1;
  rpc = ((R + n - 1) / n + 3) / 4 * 4;
  nc = (int)((R + rpc - 1) / rpc);
  if (nc < 1) nc = 1;
}
inline void colsum_into(hipStream_t s, const float* A, int lda, long long R, int cols, float* dst0, float* dst1, float* dst2,
                        int jblock, long long jstride, float* part, long long part_cap) {
  int nc;
  long long rpc;
  colsum_chunks(R, cols, part_cap, nc, rpc);
  const bool v4 = lda % 4 == 0 && (reinterpret_cast<size_t>(A) & 15) == 0;
  if (v4) hipLaunchKernelGGL(k_colsum_part<true>, dim3((unsigned)((cols + 63) / 64), (unsigned)nc), dim3(256), 0, s, A, lda, R, cols, rpc, part);
  else hipLaunchKernelGGL(k_colsum_part<false>, dim3((unsigned)((cols + 63) / 64), (unsigned)nc), dim3(256), 0, s, A, lda, R, cols, rpc, part);
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, part, nc, cols, dst0, dst1, dst2,
                     jblock, jstride);
}

struct TrainSplitPlan {
  long long total;
  SplitPlan fwd;                                    // the forward engine's slices (decoder scratch, time table, ...)
  long long base;                                   // first float after the forward plan
  long long AB[2], H1[2], H2[2], O3[2], DA2[2], DA1[2], DL[2];   // per net [X, V]: (2 T N, .) stashes
  long long VS, YS;                                 // (T + 1, N, d) momenta, (T, N, d) intermediate positions
  long long lx, lv, dvh, dz, dg, u, hv, dAB;        // running cotangents
  long long lam, lamU, dv1p, deps;
  long long w12c[2], whc[2];                        // stacked / side-by-side weight copies per net
  long long w12p[2], w4p[2], whp[2];                // ... and zero-padded to multiples of 16 both ways (net_bwd_kernel)
  long long part;                                   // chunk partials of the TN products and column sums
  long long part_cap;
  long long HD1, HD2, M1, M2, RD;                   // decoder Hessian-vector product: tangents
  long long pHD1, pHD2, pRD, pM2;                   // ... and the ones that only feed the next decoder-sized product, as bf16 planes
  long long pw2t_h, pw3t_h, pw2_h, pw3_h;           // gemm_mode 3: the decoder weights once more as f16x2 planes, for the FORWARD evaluations
  long long PS1, PS2, PRD, PB2, PB1;                // ... and, per trajectory point (T + 1 of them), the decoder's
                                                    // sigmoids, sigma' of the logits and the raw reverse products
  long long carry;                                  // Hessian-vector input carried to the same point's other use
  long long dauxh, es1, es2, de2, de1;              // image branch reverse pass
  long long ew3c, ew2c;                             // 16-byte aligned copies of its W3 / W2 (taken when the caller's are not)
  long long xq;                                     // contiguous copy of a point (built-in Hessians)
};

inline TrainSplitPlan plan_train_split(long long N, int d, int H, int T, const L2hmcMlp3* enc, const L2hmcMlp3* dec) {
  TrainSplitPlan p;
  p.fwd = plan_split(N, d, H, T, enc, dec);
  long long o = (p.fwd.total + 3) & ~3LL;
  p.base = o;
  auto take = [&](long long n) { const long long at = o; o += (n + 3) & ~3LL; return at; };
  const long long R = 2LL * T * N;
  for (int i = 0; i < 2; ++i) {
    p.AB[i] = take(R * 2 * d); p.H1[i] = take(R * H); p.H2[i] = take(R * H); p.O3[i] = take(R * 3 * d);
    p.DA2[i] = take(R * H); p.DA1[i] = take(R * H); p.DL[i] = take(R * 2 * d);
    p.w12c[i] = take(2LL * d * H); p.whc[i] = take(3LL * d * H);
    p.w12p[i] = take((long long)ceil16(2 * d) * ceil16(H)); p.w4p[i] = take((long long)ceil16(H) * ceil16(H));
    p.whp[i] = take((long long)ceil16(H) * ceil16(3 * d));
  }
  p.VS = take((T + 1) * N * d); p.YS = take((long long)T * N * d);
  p.lx = take(N * d); p.lv = take(N * d); p.dvh = take(N * d); p.dz = take(N * d); p.dg = take(N * d);
  p.u = take(N * d); p.hv = take(N * d); p.dAB = take(N * 2 * d); p.carry = take(N * d);
  p.lam = take(N); p.lamU = take(N); p.dv1p = take(N); p.deps = take(N);
  long long big = (long long)H * H;
  if ((long long)2 * d * H > big) big = 2LL * d * H;
  if ((long long)3 * d * H > big) big = 3LL * d * H;
  if (enc) {
    if ((long long)enc->n_in * enc->n_h1 > big) big = (long long)enc->n_in * enc->n_h1;
    if ((long long)enc->n_h1 * enc->n_h2 > big) big = (long long)enc->n_h1 * enc->n_h2;
    if ((long long)enc->n_h2 * enc->n_out > big) big = (long long)enc->n_h2 * enc->n_out;
  }
  p.part_cap = 16 * big;                            // up to 16 row chunks of the largest product (>= 64 of the others)
  if (p.part_cap < (1LL << 20)) p.part_cap = 1LL << 20;
  p.part = take(p.part_cap);
  if (dec) {
    p.HD1 = take(N * dec->n_h1); p.HD2 = take(N * dec->n_h2);
    p.M1 = take(N * dec->n_h1); p.M2 = take(N * dec->n_h2); p.RD = take(N * dec->n_out);
    const long long P = T + 1;
    p.PS1 = take(P * N * dec->n_h1); p.PS2 = take(P * N * dec->n_h2); p.PRD = take(P * N * dec->n_out);
    p.PB2 = take(P * N * dec->n_h2); p.PB1 = take(P * N * dec->n_h1);
    auto takep = [&](long long elems) { return take(p.fwd.planes ? (elems * 3 + 1) / 2 : 0); };
    p.pHD1 = takep(N * pld(dec->n_h1)); p.pHD2 = takep(N * pld(dec->n_h2));
    p.pRD = takep(N * pld(dec->n_out)); p.pM2 = takep(N * pld(dec->n_h2));
    auto takeh = [&](long long elems) { return take(p.fwd.planes ? elems : 0); };          // two f16 planes = elems floats
    p.pw2t_h = takeh(prows(dec->n_h2) * pld(dec->n_h1)); p.pw3t_h = takeh(prows(dec->n_out) * pld(dec->n_h2));
    p.pw2_h = takeh(prows(dec->n_h1) * pld(dec->n_h2)); p.pw3_h = takeh(prows(dec->n_h2) * pld(dec->n_out));
    p.xq = 0;
  } else {
    p.pHD1 = p.pHD2 = p.pRD = p.pM2 = 0;
    p.pw2t_h = p.pw3t_h = p.pw2_h = p.pw3_h = 0;
    p.HD1 = p.HD2 = p.M1 = p.M2 = p.RD = p.PS1 = p.PS2 = p.PRD = p.PB2 = p.PB1 = 0;
    p.xq = take(N * d);
  }
  if (enc) {
    p.dauxh = take(N * H); p.es1 = take(N * enc->n_h1); p.es2 = take(N * enc->n_h2);
    p.de2 = take(N * enc->n_h2); p.de1 = take(N * enc->n_h1);
    p.ew3c = take((long long)enc->n_h2 * enc->n_out); p.ew2c = take((long long)enc->n_h1 * enc->n_h2);
  } else {
    p.dauxh = p.es1 = p.es2 = p.de2 = p.de1 = p.ew3c = p.ew2c = 0;
  }
  p.total = o;
  return p;
}

// hv = Hessian(z) u of the decoder posterior U(z) = sum_pix BCE(aux, dec(z)) + |z|^2 / 2 (mnist_vae.py:122-126) from the
// point's DecPoint.  Forward-over-reverse: with the reverse pass b2 = r W3^T, c2 = s2 b2, b1 = c2 W2^T, c1 = s1 b1,
// grad = c1 W1^T + z, the directional derivative along u is
//   p1. = u W1,  h1. = s1 p1.,  p2. = h1. W2,  h2. = s2 p2.,  l. = h2. W3,  r. = sigma' l.
//   c2. = s2 (1 - s2) p2. b2 + s2 (r. W3^T),   c1. = s1 (1 - s1) p1. b1 + s1 (c2. W2^T),   H u = u + c1. W1^T:
// three tangent GEMMs and three reverse-tangent GEMMs, the softplus'' terms in their epilogues.
void vae_hvp(hipStream_t s, const L2hmcMlp3& dec, long long N, int d, const Mlp3Ws& ws, const DecPoint& pt,
             const TrainSplitPlan& p, float* w, const float* u, float* hv) {
  if (ws.pa1 != nullptr) {       // pre-split form: the tangents between the decoder-sized products travel as planes
    auto us = [&](long long off) { return reinterpret_cast<unsigned short*>(w + off); };
    const int l1 = pld(dec.n_h1), l2 = pld(dec.n_h2), lo = pld(dec.n_out);
    const long long n1 = N * l1, n2 = N * l2, no = N * lo;
    GemmArgs g = gemm_args(u, d, ws.w1t, dec.n_in, nullptr, dec.n_h1, N, dec.n_h1, dec.n_in);
    g.E = pt.s1; g.lde = dec.n_h1; g.E2 = pt.b1; g.lde2 = dec.n_h1; g.C2 = w + p.M1; g.ldc2 = dec.n_h1;
    g.Cp = us(p.pHD1); g.cp_plane = n1; g.ldcp = l1;
    launch_gemm<EPI_TAN>(g, s, dec.n_in <= 64 ? SHAPE_MID : SHAPE_AUTO);                             // h1. (planes), M1
    g = gemm_args(nullptr, 0, nullptr, 0, nullptr, dec.n_h2, N, dec.n_h2, dec.n_h1);
    g.Ap = us(p.pHD1); g.ap_plane = n1; g.ldap = l1; g.Bp = ws.pw2t; g.bp_plane = prows(dec.n_h2) * l1; g.ldbp = l1;
    g.E = pt.s2; g.lde = dec.n_h2; g.E2 = pt.b2; g.lde2 = dec.n_h2; g.C2 = w + p.M2; g.ldc2 = dec.n_h2;
    g.Cp = us(p.pHD2); g.cp_plane = n2; g.ldcp = l2;
    launch_gemm_planes<EPI_TAN>(g, s);                                                               // h2. (planes), M2
    g = gemm_args(nullptr, 0, nullptr, 0, nullptr, dec.n_out, N, dec.n_out, dec.n_h2);
    g.Ap = us(p.pHD2); g.ap_plane = n2; g.ldap = l2; g.Bp = ws.pw3t; g.bp_plane = prows(dec.n_out) * l2; g.ldbp = l2;
    g.E = pt.rd; g.lde = dec.n_out; g.Cp = us(p.pRD); g.cp_plane = no; g.ldcp = lo;
    launch_gemm_planes<EPI_MUL>(g, s);                                                               // r. (planes)
    g = gemm_args(nullptr, 0, nullptr, 0, w + p.M2, dec.n_h2, N, dec.n_h2, dec.n_out);
    g.Ap = us(p.pRD); g.ap_plane = no; g.ldap = lo; g.Bp = ws.pw3; g.bp_plane = prows(dec.n_h2) * lo; g.ldbp = lo;
    g.E = pt.s2; g.lde = dec.n_h2; g.accum = 1; g.Cp = us(p.pM2); g.cp_plane = n2; g.ldcp = l2;
    launch_gemm_planes<EPI_MUL>(g, s);                                                               // c2. (fp32 + planes)
    g = gemm_args(nullptr, 0, nullptr, 0, w + p.M1, dec.n_h1, N, dec.n_h1, dec.n_h2);
    g.Ap = us(p.pM2); g.ap_plane = n2; g.ldap = l2; g.Bp = ws.pw2; g.bp_plane = prows(dec.n_h1) * l2; g.ldbp = l2;
    g.E = pt.s1; g.lde = dec.n_h1; g.accum = 1;
    launch_gemm_planes<EPI_MUL>(g, s);                                                               // c1. (fp32)
    g = gemm_args(w + p.M1, dec.n_h1, dec.W1, dec.n_h1, hv, d, N, d, dec.n_h1);
    g.E = u; g.lde = d;
    launch_gemm<EPI_ADD>(g, s, d <= 64 ? SHAPE_SKINNY : SHAPE_MID);
    return;
  }
  GemmArgs g = gemm_args(u, d, ws.w1t, dec.n_in, w + p.HD1, dec.n_h1, N, dec.n_h1, dec.n_in);
  g.E = pt.s1; g.lde = dec.n_h1; g.E2 = pt.b1; g.lde2 = dec.n_h1; g.C2 = w + p.M1; g.ldc2 = dec.n_h1;
  launch_gemm<EPI_TAN>(g, s, dec.n_in <= 64 ? SHAPE_MID : SHAPE_AUTO);
  g = gemm_args(w + p.HD1, dec.n_h1, ws.w2t, dec.n_h1, w + p.HD2, dec.n_h2, N, dec.n_h2, dec.n_h1);
  g.E = pt.s2; g.lde = dec.n_h2; g.E2 = pt.b2; g.lde2 = dec.n_h2; g.C2 = w + p.M2; g.ldc2 = dec.n_h2;
  launch_gemm<EPI_TAN>(g, s);
  g = gemm_args(w + p.HD2, dec.n_h2, ws.w3t, dec.n_h2, w + p.RD, dec.n_out, N, dec.n_out, dec.n_h2);
  g.E = pt.rd; g.lde = dec.n_out;
  launch_gemm<EPI_MUL>(g, s);
  g = gemm_args(w + p.RD, dec.n_out, dec.W3, dec.n_out, w + p.M2, dec.n_h2, N, dec.n_h2, dec.n_out);
  g.E = pt.s2; g.lde = dec.n_h2; g.accum = 1;
  launch_gemm<EPI_MUL>(g, s);
  g = gemm_args(w + p.M2, dec.n_h2, dec.W2, dec.n_h2, w + p.M1, dec.n_h1, N, dec.n_h1, dec.n_h2);
  g.E = pt.s1; g.lde = dec.n_h1; g.accum = 1;
  launch_gemm<EPI_MUL>(g, s);
  g = gemm_args(w + p.M1, dec.n_h1, dec.W1, dec.n_h1, hv, d, N, d, dec.n_h1);
  g.E = u; g.lde = d;
  launch_gemm<EPI_ADD>(g, s, d <= 64 ? SHAPE_SKINNY : SHAPE_MID);
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_train_split_grad_floats(int32_t d, int32_t H, const L2hmcMlp3* aux_encoder) {
  if (d < 1 || H < 1) return fail(L2HMC_ERR_ARG, "l2hmc_train_split_grad_floats: bad argument%s");
  return 2 * snet_off(d, H).total + 1 + (aux_encoder ? mlp3_params(*aux_encoder) : 0);
}

int64_t l2hmc_train_split_workspace_floats(int64_t n_chains, int32_t d, int32_t H, int32_t T,
                                           const L2hmcMlp3* aux_encoder, const L2hmcMlp3* decoder) {
  if (n_chains < 0 || d < 1 || H < 1 || T < 1) return fail(L2HMC_ERR_ARG, "l2hmc_train_split_workspace_floats: bad argument%s");
  return plan_train_split(n_chains, d, H, T, aux_encoder, decoder).total;
}

int l2hmc_train_split_grad(const L2hmcTrainSplitArgs* a, void* stream) {
  if (a && (a->gemm_mode < 0 || a->gemm_mode > 3)) return fail(L2HMC_ERR_ARG, "gemm_mode must be 0 (f32 MFMA), 1 (bf16x3), 2 (bf16x3, split in the loop) or 3 (f16x2 planes for the forward evaluations, bf16x3 for the reverse sweep)%s");
  if (a && (a->net_mode < 0 || a->net_mode > 1)) return fail(L2HMC_ERR_ARG, "net_mode must be 0 (fused) or 1 (three products)%s");
  t_gemm_bf3 = a ? a->gemm_mode != 0 : 0;
  t_plane_mode = 0;          // (the adjoint planes hold entries scaled by 1 / chains: they need bf16's exponent range)
  if (!a) return fail(L2HMC_ERR_ARG, "args is NULL%s");
  // `energy` of kind 0 next to the decoder posterior or energy_cb: only its temperature is read (the target's own form is the
  // decoder / the callbacks)
  const bool tcarrier = a->energy != nullptr && a->energy->kind == 0;
  EngineCtx c = engine_target(*a, stream, false, tcarrier);
  const bool user = c.user, builtin = c.builtin, vae = c.vae, unets = c.unets;
  int rc;
  // (ABI 6) the caller's own S/T/Q nets (any callable, dynamics.py:69-79): forward by net_cb, reverse by net_vjp_cb
  if (a->net_cb || a->net_vjp_cb) {
    if (!a->net_cb || !a->net_vjp_cb) return fail(L2HMC_ERR_ARG, "training caller-supplied nets needs BOTH net_cb and net_vjp_cb%s");
    if (a->xnet || a->vnet || a->aux_encoder)
      return fail(L2HMC_ERR_ARG, "net_cb excludes xnet / vnet / aux_encoder (an image branch is the caller's net's own business)%s");
  }
  if ((rc = check_dims(c))) return rc;
  const long long N = c.N;
  const int d = c.d, H = c.H, T = c.T, L = c.L;
  if (N == 0) return L2HMC_OK;
  if (tcarrier && (a->energy->anneal_beta != 0.f || !(a->energy->temperature > 0.f && a->energy->temperature < INFINITY)))
    return fail(L2HMC_ERR_ARG, "an energy of kind 0 (the temperature of the decoder posterior / energy_cb) needs a finite "
                "temperature > 0 and anneal_beta = 0%s");
  if (user) {
    if (builtin || a->decoder) return fail(L2HMC_ERR_ARG, "energy_cb excludes a built-in energy and decoder%s");
    if (!a->hvp_cb) return fail(L2HMC_ERR_ARG, "training on a caller-supplied energy needs hvp_cb (the loss differentiates through grad U)%s");
    if (a->aux_encoder && !a->aux) return fail(L2HMC_ERR_ARG, "aux_encoder needs aux%s");
  } else if (builtin) {
    if (a->decoder || a->aux_encoder || a->aux)
      return fail(L2HMC_ERR_UNSUPPORTED, "a built-in energy excludes decoder / aux_encoder / aux%s");
    if (a->energy->kind == L2HMC_ENERGY_POISSON) return fail(L2HMC_ERR_UNSUPPORTED, kPoissonTrainRefusal);
    if (a->energy->kind == L2HMC_ENERGY_BINOMIAL) return fail(L2HMC_ERR_UNSUPPORTED, kBinomialTrainRefusal);
    if (a->energy->kind == L2HMC_ENERGY_PROBIT) return fail(L2HMC_ERR_UNSUPPORTED, kProbitTrainRefusal);
    if ((rc = check_energy(a->energy, d))) return rc;
    const int ek = a->energy->kind;
    if (ek == L2HMC_ENERGY_LOGISTIC)
      return fail(L2HMC_ERR_UNSUPPORTED, "the GEMM engine does not train on the logistic-regression target (its Hessian-vector "
                  "product lives in l2hmc_train_propose_grad's tile kernel): train there, or on the same likelihood as a "
                  "caller-supplied energy%s");
    if ((ek == L2HMC_ENERGY_GAUSS_DENSE || ek == L2HMC_ENERGY_GMM) && !a->hess)
      return fail(L2HMC_ERR_ARG, "dense Gaussian / mixture: hess = the RAW (n_comp, d, d) precisions%s");
    if (ek == L2HMC_ENERGY_GMM && a->energy->n_comp > HVP_MAXC)
      return fail(L2HMC_ERR_UNSUPPORTED, "mixture training: at most %s%lld components", "", (long long)HVP_MAXC);
    if (!(a->energy->temperature < INFINITY)) return fail(L2HMC_ERR_ARG, "temperature must be finite and > 0%s");
    if (a->energy->anneal_beta != 0.f && a->energy->anneal_beta != 1.f)
      return fail(L2HMC_ERR_UNSUPPORTED, "training does not differentiate the annealed energy (anneal_beta)%s");
  } else {
    if ((rc = check_mlp(a->decoder, "decoder"))) return rc;
    if (!a->aux) return fail(L2HMC_ERR_ARG, "the decoder posterior needs aux%s");
    if ((rc = check_decoder_width(c))) return rc;
  }
  if (a->aux_encoder && ((rc = check_mlp(a->aux_encoder, "aux_encoder")) || (rc = check_image_branch(c)))) return rc;
  if ((!unets && (!a->xnet || !a->vnet)) || !a->masks || !a->trig || !a->x || !a->v || !a->Lx || (!a->no_accept && (!a->p || !a->v1)) ||
      !a->grad || !a->workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_train_split_grad: NULL pointer%s");
  if ((rc = check_eps(c))) return rc;
  if (!(a->scale > 0.f) || !(a->inv_n >= 0.f)) return fail(L2HMC_ERR_ARG, "scale must be > 0 and inv_n >= 0%s");
  if (a->inv_n == 0.f && !a->dLx_in) return fail(L2HMC_ERR_ARG, "inv_n = 0 (no loss term of its own) needs dLx_in%s");
  if (a->no_accept && !a->dLx_in) return fail(L2HMC_ERR_ARG, "no_accept (a link of chain_operator) needs dLx_in%s");
  if (!(a->energy_scale >= 0.f)) return fail(L2HMC_ERR_ARG, "energy_scale must be >= 0%s");
  const TrainSplitPlan p = plan_train_split(N, d, H, T, a->aux_encoder, a->decoder);
  if ((rc = check_workspace(a->workspace_floats, p.total))) return rc;
  const SplitPlan& f = p.fwd;
  engine_bind(c, a->workspace, f, a->gemm_mode);
  hipStream_t s = c.s;
  float* w = c.w;
  // training on U / temperature: the built-in energies (l2hmc_energy) and the callbacks return it tempered; the decoder
  // posterior is evaluated plain and tempered behind (k_temper), only when temperature != 1
  const float temp = a->energy != nullptr ? a->energy->temperature : 1.f;
  const float itemp = 1.f / temp;
  const bool temper_dec = vae && temp != 1.f;
  c.temp = temp;
  auto us = [&](long long off) { return reinterpret_cast<unsigned short*>(w + off); };
  // the decoder-sized products of the forward pass and of the Hessian-vector products on pre-split planes (round 5), when the
  // sampler's own planes rule says so (gemm_mode 1, >= 84 tiles: 3072 chains at config 5's widths)
  if (c.use_planes) {
    if ((rc = planes_prepare()) || (rc = gemm_planes_prepare<EPI_TAN>())) return rc;      // ... and the Hessian-vector products' own
    if (a->gemm_mode == 3) { c.dws.pw2t_h = us(p.pw2t_h); c.dws.pw3t_h = us(p.pw3t_h); c.dws.pw2_h = us(p.pw2_h); c.dws.pw3_h = us(p.pw3_h); }
  }
  c.ews.s1 = w + p.es1; c.ews.s2 = w + p.es2;        // the image branch's sigmoids stay for its reverse pass
  const L2hmcMlp3& dec = *c.dec;
  const Mlp3Ws &dws = c.dws, &ews = c.ews;
  const L2hmcNet &xn = *c.nets[0], &vn = *c.nets[1];
  const L2hmcNet* const* nets = c.nets;
  const unsigned char* dir = c.dir;
  const int dall = c.dall;
  const unsigned nw4 = (unsigned)((N + 3) / 4);
  float* ld = c.ld;
  double *U0d = reinterpret_cast<double*>(w + f.U0), *U1d = reinterpret_cast<double*>(w + f.U1);
  const long long NL = N * L, NH = N * H, N3 = N * 3 * d, Nd = N * d;
  // stash slices of evaluation `ne` (= 2 it + which) of net `net` (0 = X, 1 = V)
  auto AB = [&](int net, int ne) { return w + p.AB[net] + ne * NL; };
  auto H1 = [&](int net, int ne) { return w + p.H1[net] + ne * NH; };
  auto H2 = [&](int net, int ne) { return w + p.H2[net] + ne * NH; };
  auto O3 = [&](int net, int ne) { return w + p.O3[net] + ne * N3; };
  auto DA2 = [&](int net, int ne) { return w + p.DA2[net] + ne * NH; };
  auto DA1 = [&](int net, int ne) { return w + p.DA1[net] + ne * NH; };
  auto DL = [&](int net, int ne) { return w + p.DL[net] + ne * NL; };
  auto VS = [&](int it) { return w + p.VS + it * Nd; };
  auto YS = [&](int it) { return w + p.YS + it * Nd; };

  // One net evaluation -- and its reverse -- in ONE launch each (net_eval_kernel with both hidden activations kept,
  // net_bwd_kernel) under the sampler's own rule for the fused form, with the reverse's wider K (plan_nets)
  if ((rc = plan_nets(c, true, a->net_mode))) return rc;
  const bool fused_nets = c.np.fused;
  // ---- weights: the engine's preparation (nothing is kept from an earlier call: a `reuse` of the trainer's own would go
  //      here), then what the reverse sweep needs on top of it -------------------------------------------------------
  prepare_decoder(c, false);
  if (c.use_planes) {          // the padding of the four tangent planes up to whole k-tiles, zeroed once
    planes_zero_pad(s, us(p.pHD1), N, dec.n_h1, pld(dec.n_h1));
    planes_zero_pad(s, us(p.pHD2), N, dec.n_h2, pld(dec.n_h2));
    planes_zero_pad(s, us(p.pRD), N, dec.n_out, pld(dec.n_out));
    planes_zero_pad(s, us(p.pM2), N, dec.n_h2, pld(dec.n_h2));
  }
  prepare_image_branch(c, false, false);
  const int Hp = ceil16(H);
  prepare_nets(c, false, [&](int i) {       // stacked copies for the input-gradient products
    hipLaunchKernelGGL(k_stack_rows, dim3(nblk(2LL * d * H)), dim3(256), 0, s, nets[i]->W1, nets[i]->W2, (long long)d * H,
                       (long long)d * H, w + p.w12c[i]);
    hipLaunchKernelGGL(k_heads_side, dim3(nblk(3LL * d * H)), dim3(256), 0, s, nets[i]->Ws, nets[i]->Wt, nets[i]->Wq, H, d,
                       w + p.whc[i]);
    if (fused_nets) {          // the same three matrices, rows and K zero-padded to multiples of 16 (net_bwd_kernel has no guards)
      const int K3p = ceil16(3 * d);
      (void)hipMemsetAsync(w + p.w12p[i], 0, sizeof(float) * (size_t)(p.whp[i] + (long long)Hp * K3p - p.w12p[i]), s);
      (void)hipMemcpy2DAsync(w + p.w12p[i], sizeof(float) * Hp, w + p.w12c[i], sizeof(float) * H, sizeof(float) * H, (size_t)L,
                             hipMemcpyDeviceToDevice, s);
      (void)hipMemcpy2DAsync(w + p.w4p[i], sizeof(float) * Hp, nets[i]->W4, sizeof(float) * H, sizeof(float) * H, (size_t)H,
                             hipMemcpyDeviceToDevice, s);
      (void)hipMemcpy2DAsync(w + p.whp[i], sizeof(float) * K3p, w + p.whc[i], sizeof(float) * 3 * d, sizeof(float) * 3 * d, (size_t)H,
                             hipMemcpyDeviceToDevice, s);
    }
  });

  // trajectory point j = 0 .. T (the start point and the position after each leapfrog step)
  auto dec_point = [&](int j) {
    DecPoint pt = {};
    if (vae) {
      pt.s1 = w + p.PS1 + (long long)j * N * dec.n_h1; pt.s2 = w + p.PS2 + (long long)j * N * dec.n_h2;
      pt.rd = w + p.PRD + (long long)j * N * dec.n_out;
      pt.b2 = w + p.PB2 + (long long)j * N * dec.n_h2; pt.b1 = w + p.PB1 + (long long)j * N * dec.n_h1;
    }
    return pt;
  };
  // U (double, optional) and grad U at point j, held in columns [0, d) of `ab` -> columns [d, 2 d), its DecPoint kept
  auto energy_eval = [&](float* ab, int j, double* Ud) -> int {
    const DecPoint pt = dec_point(j);
    return energy_at(c, ab, Ud, &pt);
  };
  // one net evaluation with everything kept: h1, h2 and the head products of evaluation (net, ne) (with the fused kernel the
  // raw head products still go to O3 for the reverse sweep), and the half-update that consumes it
  auto net_fwd = [&](int net, int ne, int it, const NetEvalArgs::Update& upd) -> int {
    const NetKeep keep = {H1(net, ne), H2(net, ne), O3(net, ne)};
    return net_eval(c, net, AB(net, ne), it, upd, &keep);
  };
  int cb_rc = 0;                                   // first nonzero return of a net reverse callback (checked after the sweep)
  // reverse of net_fwd for the data path: O3 holds (d zs | d zt | d zq) -> DA2, DA1 (kept for the weight gradients), dAB
  auto net_bwd = [&](int net, int ne) {
    if (unets) {       // (d S | d T | d Q) of evaluation (net, ne) -> (d a | d b); the caller accumulates its parameters' gradients
      if (!cb_rc) cb_rc = a->net_vjp_cb(a->net_cb_user, net, AB(net, ne), L, N, d, ne / 2, dir, dall, O3(net, ne), w + p.dAB, L, stream);
      return;
    }
    if (fused_nets) {
      NetBwdArgs nb = {};
      nb.dO3 = O3(net, ne); nb.ldo = 3 * d; nb.Whc = w + p.whp[net]; nb.W4 = w + p.w4p[net]; nb.W12 = w + p.w12p[net];
      nb.h2 = H2(net, ne); nb.h1 = H1(net, ne); nb.da2 = DA2(net, ne); nb.da1 = DA1(net, ne); nb.dAB = w + p.dAB; nb.ldab = L;
      nb.M = (int)N; nb.d = d; nb.H = H;
      launch_net_bwd(c.np.cb, c.np.blocks, c.np.nb_lds, s, nb);
      return;
    }
    GemmArgs ga = gemm_args(O3(net, ne), 3 * d, w + p.whc[net], 3 * d, DA2(net, ne), H, N, H, 3 * d);
    ga.E = H2(net, ne); ga.lde = H;
    launch_gemm<EPI_MASK>(ga, s, SHAPE_MID);
    ga = gemm_args(DA2(net, ne), H, nets[net]->W4, H, DA1(net, ne), H, N, H, H);
    ga.E = H1(net, ne); ga.lde = H;
    launch_gemm<EPI_MASK>(ga, s, SHAPE_MID);
    ga = gemm_args(DA1(net, ne), H, w + p.w12c[net], H, w + p.dAB, L, N, L, H);
    launch_gemm<EPI_BIAS>(ga, s, SHAPE_MID);
  };

  // ---- forward trajectory, everything kept ------------------------------------------------------------------------
  (void)hipMemcpy2DAsync(AB(1, 0), sizeof(float) * L, a->x, sizeof(float) * d, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, s);
  (void)hipMemcpyAsync(VS(0), a->v, sizeof(float) * Nd, hipMemcpyDeviceToDevice, s);
  launch_kinetic(s, VS(0), w + f.K0, ld, N, d);
  if ((rc = energy_eval(AB(1, 0), 0, U0d))) return rc;
  for (int it = 0; it < T; ++it) {
    const bool last = it == T - 1;
    float *abv0 = AB(1, 2 * it), *abv1 = AB(1, 2 * it + 1), *abx0 = AB(0, 2 * it), *abx1 = AB(0, 2 * it + 1);
    if ((rc = net_fwd(1, 2 * it, it, v_update(L, VS(it), d, abv0 + d, abx0, L, abv0, abx0 + d)))) return rc;     // v_h, xin = k1 x
    if ((rc = net_fwd(0, 2 * it, it, x_update(L, abv0, L, abx0, YS(it), d, abx1 + d, 0)))) return rc;          // y, xin = (1 - k1) y
    (void)hipMemcpy2DAsync(abx1, sizeof(float) * L, abx0, sizeof(float) * L, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, s);
    if ((rc = net_fwd(0, 2 * it + 1, it, x_update(L, YS(it), d, abx0, abv1, L, nullptr, 1)))) return rc;       // x'
    if ((rc = energy_eval(abv1, it + 1, last ? U1d : nullptr))) return rc;
    if ((rc = net_fwd(1, 2 * it + 1, it, v_update(L, abx0, L, abv1 + d, VS(it + 1), d, nullptr, nullptr)))) return rc;   // v'
    if (!last) (void)hipMemcpyAsync(AB(1, 2 * it + 2), abv1, sizeof(float) * NL, hipMemcpyDeviceToDevice, s);
  }

  // ---- accept probability, loss argument, adjoint seeds -----------------------------------------------------------
  float *lx = w + p.lx, *lv = w + p.lv, *dvh = w + p.dvh, *dz = w + p.dz, *dg = w + p.dg, *uu = w + p.u, *hv = w + p.hv;
  float *lam = w + p.lam, *lamU = w + p.lamU, *dv1p = w + p.dv1p, *deps = w + p.deps, *dAB = w + p.dAB;
  {
    const float* abe = AB(1, 2 * T - 1);
    hipLaunchKernelGGL(k_train_seed, dim3(nw4), dim3(256), 0, s, a->x, abe, L, VS(T), abe + d, L, U0d, U1d, w + f.K0, ld,
                       a->dist_weight, a->dLx_in, a->dLv_in, a->dlogjac_in, a->no_accept, a->scale, a->inv_n,
                       a->energy_scale, a->Lx, a->Lv_out, a->logjac_out, a->p, a->v1, a->ediff_out, lam, lamU, dv1p, lx, lv,
                       deps, temp, N, d);
  }
  // VNet evaluation at trajectory point j (inputs (x, grad U(x)) in `ab`):  lx += d a + Hessian(x) (dg + d b).
  // Every interior point is the input of TWO VNet evaluations (the end of one leapfrog step and the start of the next,
  // at different times) whose Hessian-vector products add into the same lx before anything reads it: the later one in
  // the sweep (`defer`) only adds d a and parks its vector in `carry`, the earlier one multiplies the sum -- T + 1
  // Hessian-vector products per trajectory instead of 2 T.
  float* carry = w + p.carry;
  bool have_carry = false;
  auto through_grad = [&](float* ab, int j, bool defer) -> int {
    hipLaunchKernelGGL(k_comb_v1, dim3(nblk(Nd)), dim3(256), 0, s, dg, dAB, have_carry ? carry : (const float*)nullptr,
                       defer ? carry : uu, N, d);
    if (defer) {
      hipLaunchKernelGGL(k_comb_v2, dim3(nblk(Nd)), dim3(256), 0, s, lx, dAB, (const float*)nullptr, N, d);
      have_carry = true;
      return L2HMC_OK;
    }
    have_carry = false;
    if (user) {
      const int r = a->hvp_cb(a->energy_cb_user, ab, L, uu, d, N, d, hv, d, stream);
      if (r) return fail(L2HMC_ERR_ARG, "the Hessian-vector callback failed (returned %s%lld)", "", (long long)r);
    } else if (vae) {
      vae_hvp(s, dec, N, d, dws, dec_point(j), p, w, uu, hv);
      if (temper_dec) hipLaunchKernelGGL(k_temper, dim3(nblk(Nd)), dim3(256), 0, s, hv, d, (double*)nullptr, itemp, 1.0, N, d);
    } else if (a->energy->kind == L2HMC_ENERGY_GMM || a->energy->kind == L2HMC_ENERGY_FUNNEL) {
      hipLaunchKernelGGL(k_hvp_chain, dim3(nblk(N)), dim3(256), 0, s, a->energy->kind, ab, L, uu, hv, dg, a->energy->mu, a->hess,
                         a->energy->logc, a->energy->n_comp, a->energy->eta, itemp, N, d);   // (dg is free: its sum went into uu)
    } else {
      hipLaunchKernelGGL(k_hvp_builtin, dim3(nblk(Nd)), dim3(256), 0, s, a->energy->kind, ab, L, uu, hv, a->energy->prec,
                         a->hess, a->energy->eta, a->energy->kind == L2HMC_ENERGY_ROUGHWELL ? roughwell_den(a->energy) : 1.f, itemp,
                         N, d);
    }
    hipLaunchKernelGGL(k_comb_v2, dim3(nblk(Nd)), dim3(256), 0, s, lx, dAB, hv, N, d);
    return L2HMC_OK;
  };

  // ---- reverse sweep (train.hip "reverse sweep", stages (1)-(4)) ----------------------------------------------------
  for (int it = T - 1; it >= 0; --it) {
    float *abv0 = AB(1, 2 * it), *abv1 = AB(1, 2 * it + 1), *abx0 = AB(0, 2 * it);
    // (1) v' = v_half(vh; g(x'), V(x', g(x')))
    hipLaunchKernelGGL(k_tv_half_bwd, dim3(nw4), dim3(256), 0, s, O3(1, 2 * it + 1), vn, abx0, L, abv1 + d, L, lv, dvh, dg,
                       DL(1, 2 * it + 1), lam, deps, dir, dall, a->alpha, a->eps_host, N, d);
    net_bwd(1, 2 * it + 1);
    if ((rc = through_grad(abv1, it + 1, false))) return rc;        // lx = d x'
    // (2) x' = x_half(y, 1 - k1; vh, X(vh, (1 - k1) y))
    hipLaunchKernelGGL(k_tx_half_bwd, dim3(nw4), dim3(256), 0, s, O3(0, 2 * it + 1), xn, YS(it), d, abx0, L, lx, dz, dvh,
                       DL(0, 2 * it + 1), lam, deps, a->masks, dir, dall, it, T, 1, a->alpha, a->eps_host, N, d);
    net_bwd(0, 2 * it + 1);
    hipLaunchKernelGGL(k_comb_x, dim3(nblk(Nd)), dim3(256), 0, s, dAB, dvh, dz, a->masks, dir, dall, it, T, 1, N, d);
    // (3) y = x_half(x, k1; vh, X(vh, k1 x))
    hipLaunchKernelGGL(k_tx_half_bwd, dim3(nw4), dim3(256), 0, s, O3(0, 2 * it), xn, abv0, L, abx0, L, dz, lx, dvh,
                       DL(0, 2 * it), lam, deps, a->masks, dir, dall, it, T, 0, a->alpha, a->eps_host, N, d);
    net_bwd(0, 2 * it);
    hipLaunchKernelGGL(k_comb_x, dim3(nblk(Nd)), dim3(256), 0, s, dAB, dvh, lx, a->masks, dir, dall, it, T, 0, N, d);
    // (4) vh = v_half(v; g(x), V(x, g(x)))
    hipLaunchKernelGGL(k_tv_half_bwd, dim3(nw4), dim3(256), 0, s, O3(1, 2 * it), vn, VS(it), d, abv0 + d, L, dvh, lv, dg,
                       DL(1, 2 * it), lam, deps, dir, dall, a->alpha, a->eps_host, N, d);
    net_bwd(1, 2 * it);
    if ((rc = through_grad(abv0, it, it > 0))) return rc;
  }
  if (a->dx0_out) {
    const float* ab0 = AB(1, 0);
    hipLaunchKernelGGL(k_train_dx0, dim3(nblk(Nd)), dim3(256), 0, s, lx, a->x, AB(1, 2 * T - 1), L, ab0 + d, L, a->dist_weight,
                       lamU, dv1p, a->dx0_out, N, d);
  }

  if (cb_rc) return fail(L2HMC_ERR_ARG, "the net reverse callback failed (returned %s%lld)", "", (long long)cb_rc);
  if (unets) {         // the nets' parameter gradients were accumulated by the callbacks; what is the library's is d loss / d eps
    hipLaunchKernelGGL(k_sum_chain, dim3(1), dim3(256), 0, s, deps, N, a->grad);
    return launched();
  }
  // ---- parameter gradients: one contraction over all (evaluation, chain) rows per weight matrix ---------------------
  const SNetOff o = snet_off(d, H);
  const long long R = 2LL * T * N;
  float* part = w + p.part;
  for (int net = 0; net < 2; ++net) {
    float* G = a->grad + (long long)net * o.total;
    const float *ab = w + p.AB[net], *h1 = w + p.H1[net], *h2 = w + p.H2[net], *dzs = w + p.O3[net];
    const float *da2 = w + p.DA2[net], *da1 = w + p.DA1[net], *dl = w + p.DL[net];
    // [W1; W2] = [a | b]^T d h1: one product, the two row blocks land d H + H apart (b1 lies between them)
    const TnScatter sc12 = {d, o.W2 - o.W1, H, 0};
    launch_gemm_tn(s, ab, L, da1, H, R, L, H, G + o.W1, H, 1, part, p.part_cap, &sc12);
    launch_gemm_tn(s, h1, H, da2, H, R, H, H, G + o.W4, H, 1, part, p.part_cap);
    // [Ws | Wt | Wq] = h2^T (d zs | d zt | d zq): one product, three column blocks
    const TnScatter sch = {H, 0, d, o.Wt - o.Ws};
    launch_gemm_tn(s, h2, H, dzs, 3 * d, R, H, 3 * d, G + o.Ws, d, 1, part, p.part_cap, &sch);
    colsum_into(s, da1, H, R, H, G + o.b1, G + o.b2, G + o.b3, 0, 0, part, p.part_cap);   // b1, b2, b3 enter the same sum
    colsum_into(s, da2, H, R, H, G + o.b4, nullptr, nullptr, 0, 0, part, p.part_cap);
    colsum_into(s, dzs, 3 * d, R, 3 * d, G + o.bs, nullptr, nullptr, d, o.bt - o.bs, part, p.part_cap);
    colsum_into(s, dl, L, R, L, G + o.ls, nullptr, nullptr, d, o.lq - o.ls, part, p.part_cap);
    {
      // chunks per evaluation: ~ 128 blocks x column blocks in total, within the partial buffer
      int cpe = (int)((128 + 2 * T - 1) / (2 * T));
      if ((long long)cpe * 2 * T * 2 * H > p.part_cap) cpe = (int)(p.part_cap / (4LL * T * H));
      if (cpe < 1) cpe = 1;
      const long long rpc = (N + cpe - 1) / cpe;
      const int nc = 2 * T * cpe;
      hipLaunchKernelGGL(k_w3_part, dim3((unsigned)((H + 63) / 64), (unsigned)nc), dim3(256), 0, s, da1, H, N, cpe, rpc, a->trig, T,
                         dir, dall, part);
      hipLaunchKernelGGL(tn_reduce_kernel, dim3((unsigned)((2 * H + 255) / 256)), dim3(256), 0, s, part, nc, 2, H, G + o.W3, H, 1,
                         TnScatter{2, 0, H, 0});
    }
  }
  hipLaunchKernelGGL(k_sum_chain, dim3(1), dim3(256), 0, s, deps, N, a->grad + 2 * o.total);
  if (a->aux_encoder) {
    // the image branch: d aux_h = sum over all 4 T evaluations of d h1_pre; reverse through the 3-layer MLP
    const L2hmcMlp3& enc = *a->aux_encoder;
    float* G = a->grad + 2 * o.total + 1;
    const long long oW1 = 0, ob1 = oW1 + (long long)enc.n_in * enc.n_h1, oW2 = ob1 + enc.n_h1,
                    ob2 = oW2 + (long long)enc.n_h1 * enc.n_h2, oW3 = ob2 + enc.n_h2, ob3 = oW3 + (long long)enc.n_h2 * enc.n_out;
    float *dauxh = w + p.dauxh, *de2 = w + p.de2, *de1 = w + p.de1;
    hipLaunchKernelGGL(k_sum_evals, dim3(nblk(NH)), dim3(256), 0, s, w + p.DA1[0], w + p.DA1[1], 2 * T, NH, dauxh);
    // The reverse products read W3 / W2 as stored.  A caller that keeps its parameters in one flat buffer behind the single
    // alpha (the native trainer does) hands over 4-byte aligned matrices: the products would take the scalar-load form (83 us
    // each at 8192 chains against ~30) -- a 5 MB copy into aligned slots is cheaper.
    const float *eW3 = enc.W3, *eW2 = enc.W2;
    if ((reinterpret_cast<size_t>(eW3) & 15) != 0) {
      (void)hipMemcpyAsync(w + p.ew3c, enc.W3, sizeof(float) * (size_t)enc.n_h2 * enc.n_out, hipMemcpyDeviceToDevice, s);
      eW3 = w + p.ew3c;
    }
    if ((reinterpret_cast<size_t>(eW2) & 15) != 0) {
      (void)hipMemcpyAsync(w + p.ew2c, enc.W2, sizeof(float) * (size_t)enc.n_h1 * enc.n_h2, hipMemcpyDeviceToDevice, s);
      eW2 = w + p.ew2c;
    }
    GemmArgs ga = gemm_args(dauxh, H, eW3, enc.n_out, de2, enc.n_h2, N, enc.n_h2, enc.n_out);
    ga.E = ews.s2; ga.lde = enc.n_h2;
    launch_gemm<EPI_MUL>(ga, s, SHAPE_MID);
    ga = gemm_args(de2, enc.n_h2, eW2, enc.n_h2, de1, enc.n_h1, N, enc.n_h1, enc.n_h2);
    ga.E = ews.s1; ga.lde = enc.n_h1;
    launch_gemm<EPI_MUL>(ga, s, SHAPE_MID);
    launch_gemm_tn(s, ews.a2, enc.n_h2, dauxh, H, N, enc.n_h2, enc.n_out, G + oW3, enc.n_out, 1, part, p.part_cap);
    colsum_into(s, dauxh, H, N, enc.n_out, G + ob3, nullptr, nullptr, 0, 0, part, p.part_cap);
    launch_gemm_tn(s, ews.a1, enc.n_h1, de2, enc.n_h2, N, enc.n_h1, enc.n_h2, G + oW2, enc.n_h2, 1, part, p.part_cap);
    colsum_into(s, de2, enc.n_h2, N, enc.n_h2, G + ob2, nullptr, nullptr, 0, 0, part, p.part_cap);
    launch_gemm_tn(s, a->aux, enc.n_in, de1, enc.n_h1, N, enc.n_in, enc.n_h1, G + oW1, enc.n_h1, 1, part, p.part_cap);
    colsum_into(s, de1, enc.n_h1, N, enc.n_h1, G + ob1, nullptr, nullptr, 0, 0, part, p.part_cap);
  }
  return launched();
}

}  // extern "C"
