// l2hmc_trajectory_split -- the generalised-leapfrog trajectory for models that do not fit the
// single fused kernel: wide S/T/Q nets (any H), an image-conditioned 4th branch
// (`encoder_sampler(aux)`, mnist_vae.py:134-150) and the VAE latent-posterior energy
// (mnist_vae.py:104-126: decoder 50 -> 1024 -> 1024 -> 784, BCE + prior).  BASELINE.json config 5.
//
// Everything GEMM-shaped here is a dense product over the chain batch -- (N x K)(K x M) with N = thousands
// of chains: our own fp32 MFMA GEMM (gemm_f32.hpp) with bias / softplus / sigmoid / relu / BCE-gradient /
// chain-rule epilogues fused in; what remains between the products (the masked leapfrog updates with
// tanh / exp, log-det, accept probability, MH select) is a handful of small kernels.  No BLAS library.
// One C-ABI call enqueues the whole trajectory on the caller's stream; all intermediates live in
// a caller-provided workspace.  Same per-chain direction mixing as the fused kernel: each chain
// runs only in its drawn direction.
#include "gemm_f32.hpp"
#include "gemm_xl.hpp"

namespace l2hmc {

// Wt[n][k] = W[k][n]  (W is (K, N) row-major): the forward products contract with W^T in the NT GEMM
__global__ void k_transpose(const float* W, int K, int N, float* Wt, int ldt, int col_off) {
  __shared__ float tile[32][33];
  const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + threadIdx.x;
    tile[r][threadIdx.x] = (k < K && n < N) ? W[(long long)k * N + n] : 0.f;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int n = n0 + r, k = k0 + threadIdx.x;
    if (n < N && k < K) Wt[(long long)n * ldt + col_off + k] = tile[threadIdx.x][r];
  }
}
inline void transpose_into(hipStream_t s, const float* W, int K, int N, float* Wt, int ldt, int col_off) {
  hipLaunchKernelGGL(k_transpose, dim3((N + 31) / 32, (K + 31) / 32), dim3(32, 8), 0, s, W, K, N, Wt, ldt, col_off);
}

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// time-embedding table tb[net][s][j] = W3[0][j] cos_s + W3[1][j] sin_s + b1 + b2 + b3
__global__ void k_time_table(L2hmcNet xn, L2hmcNet vn, const float* trig, int T, int H, float* tb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * T * H) return;
  const int net = i / (T * H), s = (i / H) % T, j = i % H;
  const L2hmcNet& w = net == 0 ? xn : vn;
  tb[i] = w.W3[j] * trig[2 * s] + w.W3[H + j] * trig[2 * s + 1] + ((w.b1[j] + w.b2[j]) + w.b3[j]);
}
__device__ __forceinline__ int row_of(const unsigned char* dir, int dir_all, long long n, int it, int T, bool& fwd) {
  fwd = dir != nullptr ? dir[n] != 0 : (dir_all != 0);
  return fwd ? it : (T - 1 - it);
}
// U[n] = sum of the BCE row partials the logits GEMM left (fixed order) + |z|^2 / 2   (mnist_vae.py:122-126)
// (|U| ~ 550 for MNIST-sized images: one fp32 rounding of U is 3e-5, so the partials are added in double and the
//  trajectory keeps U0 / U1 as doubles for the energy DIFFERENCE of p_accept; the fp32 copy is for the API.)
__global__ void k_vae_U(const float* rowsum, int np, const float* z, int ldz, int d, float* U, double* Ud,
                        long long N) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double acc = 0.0;
  for (int k = 0; k < np; ++k) acc += (double)rowsum[n * np + k];
  double qd = 0.0;
  for (int k = 0; k < d; ++k) qd += (double)z[n * ldz + k] * (double)z[n * ldz + k];
  acc += 0.5 * qd;
  if (U != nullptr) U[n] = (float)acc;
  if (Ud != nullptr) Ud[n] = acc;
}
// The per-chain reductions of the engine (energy from its row partials, kinetic energy) as one thread per chain walk 50-odd
// strided words each: 8192 chains = 32 workgroups of pure latency (17 / 10 us, the proposal's MH select 29 us -- round 5 trace).
// Staged forms: a workgroup's ROW_CPB chains are read coalesced into LDS, then thread = chain sums ITS row in the same order as
// before (bit-identical results).  Taken while the rows fit 48 KB.
constexpr int ROW_CPB = 64;
__device__ __forceinline__ void stage_rows(float* sm, const float* src, long long ld, int cols, long long n0, long long N) {
  for (int i = threadIdx.x; i < ROW_CPB * cols; i += blockDim.x) {
    const int r = i / cols, k = i % cols;
    sm[i] = n0 + r < N ? src[(n0 + r) * ld + k] : 0.f;
  }
}
__global__ __launch_bounds__(256) void k_vae_U_staged(const float* rowsum, int np, const float* z, int ldz, int d, float* U,
                                                      double* Ud, long long N) {
  extern __shared__ float rsm[];
  float *sr = rsm, *sz = rsm + ROW_CPB * np;
  const long long n0 = (long long)blockIdx.x * ROW_CPB;
  stage_rows(sr, rowsum, np, np, n0, N);
  stage_rows(sz, z, ldz, d, n0, N);
  __syncthreads();
  const long long n = n0 + threadIdx.x;
  if (threadIdx.x >= ROW_CPB || n >= N) return;
  double acc = 0.0;
  for (int k = 0; k < np; ++k) acc += (double)sr[threadIdx.x * np + k];
  double qd = 0.0;
  for (int k = 0; k < d; ++k) qd += (double)sz[threadIdx.x * d + k] * (double)sz[threadIdx.x * d + k];
  acc += 0.5 * qd;
  if (U != nullptr) U[n] = (float)acc;
  if (Ud != nullptr) Ud[n] = acc;
}
inline void launch_vae_U(hipStream_t s, const float* rowsum, int np, const float* z, int ldz, int d, float* U, double* Ud, long long N) {
  const size_t lds = sizeof(float) * ROW_CPB * (size_t)(np + d);
  if (lds <= 48 * 1024)
    hipLaunchKernelGGL(k_vae_U_staged, dim3((unsigned)((N + ROW_CPB - 1) / ROW_CPB)), dim3(256), lds, s, rowsum, np, z, ldz, d, U, Ud, N);
  else
    hipLaunchKernelGGL(k_vae_U, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, rowsum, np, z, ldz, d, U, Ud, N);
}
// HMC mode (nets identically zero, dynamics.py:73-76): the generalised step is the plain leapfrog
//   v_h = v - (eps/2) g(x);  x' = x + eps v_h     [k_hmc_drift]      v' = v_h - (eps/2) g(x')   [k_hmc_kick]
// and its inverse (dynamics.py:159-201 with S = T = Q = 0: v_h = v + (eps/2) g(x'), x = x' - eps v_h, v = v_h + (eps/2) g(x))
// is the same step with eps -> -eps, per chain by its direction bit.
__device__ __forceinline__ float hmc_eps(const float* alpha, float eps_host, const unsigned char* dir, int dall, long long n) {
  const float eps = alpha != nullptr ? expf(*alpha) : eps_host;
  return (dir != nullptr ? dir[n] != 0 : dall != 0) ? eps : -eps;
}
__global__ void k_hmc_drift(float* x, int ldx, const float* v, const float* g, int ldg, float* vh, const float* alpha,
                            float eps_host, const unsigned char* dir, int dall, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  const float eps = hmc_eps(alpha, eps_host, dir, dall, n);
  const float h = v[i] + 0.5f * eps * (-g[n * ldg + k]);
  vh[i] = h;
  x[n * ldx + k] = x[n * ldx + k] + eps * h;
}
__global__ void k_hmc_kick(float* v, const float* vh, const float* g, int ldg, const float* alpha, float eps_host,
                           const unsigned char* dir, int dall, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const float eps = hmc_eps(alpha, eps_host, dir, dall, i / d);
  v[i] = vh[i] + 0.5f * eps * (-g[(i / d) * ldg + (i % d)]);
}

// Update kernels: ONE WAVE PER CHAIN, lanes over the d dimensions (coalesced rows of every operand), the chain's
// log-det contribution a fixed-order wave reduction.  Every state array carries its row stride: the engine keeps
// [x | grad U] and [v_h | masked x] side by side (row stride 2 d) so that they ARE the K = 2 d inputs of the nets'
// first layer.
__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  return a;
}
// Momentum half-update.  out3 = h2 [Ws|Wt|Wq] (no biases yet).  forward: v' = v e^{eps S/2} + (eps/2)(T - e^{eps Q} g);
// backward: v' = (v - (eps/2)(T - e^{eps Q} g)) e^{-eps S/2}   (dynamics.py:121-125,149-153 / :164-170,194-199)
__global__ __launch_bounds__(256) void k_v_half(const float* out3, L2hmcNet w, const float* vin, int ldvi,
                                                const float* g, int ldg, float* vout, int ldvo, float* ld,
                                                const unsigned char* dir, int dir_all, const float* alpha,
                                                float eps_host, long long N, int d) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  const bool fwd = dir != nullptr ? dir[n] != 0 : (dir_all != 0);
  const float eps = alpha != nullptr ? expf(*alpha) : eps_host, heps = 0.5f * eps, sgn = fwd ? 1.f : -1.f;
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) {
    // (w.lam_s == NULL: out3 already holds the final S | T | Q of a caller-supplied net, L2hmcNetCallback)
    const bool raw = w.lam_s == nullptr;
    const float S = raw ? out3[n * 3 * d + k] : expf(w.lam_s[k]) * tanhf(out3[n * 3 * d + k] + w.bs[k]);
    const float T = raw ? out3[n * 3 * d + d + k] : out3[n * 3 * d + d + k] + w.bt[k];
    const float Q = raw ? out3[n * 3 * d + 2 * d + k] : expf(w.lam_q[k]) * tanhf(out3[n * 3 * d + 2 * d + k] + w.bq[k]);
    const float sv = sgn * heps * S, ES = expf(sv), EQ = expf(eps * Q);
    const float cc = heps * (T - EQ * g[n * ldg + k]);
    const float vi = vin[n * ldvi + k];
    vout[n * ldvo + k] = fwd ? vi * ES + cc : (vi - cc) * ES;
    acc += sv;
  }
  acc = wave_sum(acc);
  if (lane == 0) ld[n] += acc;
}
// Masked position update + the masked input of the NEXT net evaluation.  second = 0: keeps
// k1 = (fwd ? m : 1-m) and emits xin = (1-k1) z'; second = 1: keeps 1-k1.
// (dynamics.py:131-145 / :176-190)
__global__ __launch_bounds__(256) void k_x_half(const float* out3, L2hmcNet w, const float* zin, int ldzi,
                                                const float* vh, int ldvh, float* zout, int ldzo, float* xin_next,
                                                int ldxn, float* ld, const float* masks, const unsigned char* dir,
                                                int dir_all, int it, int T, int second, const float* alpha,
                                                float eps_host, long long N, int d) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  bool fwd;
  const int s = row_of(dir, dir_all, n, it, T, fwd);
  const float eps = alpha != nullptr ? expf(*alpha) : eps_host, sgn = fwd ? 1.f : -1.f;
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float m = masks[s * d + k];
    const float k1 = fwd ? m : 1.f - m;
    const float kp = second ? 1.f - k1 : k1, up = 1.f - kp;
    const bool raw = w.lam_s == nullptr;
    const float S = raw ? out3[n * 3 * d + k] : expf(w.lam_s[k]) * tanhf(out3[n * 3 * d + k] + w.bs[k]);
    const float T_ = raw ? out3[n * 3 * d + d + k] : out3[n * 3 * d + d + k] + w.bt[k];
    const float Q = raw ? out3[n * 3 * d + 2 * d + k] : expf(w.lam_q[k]) * tanhf(out3[n * 3 * d + 2 * d + k] + w.bq[k]);
    const float sx = sgn * eps * S, ES = expf(sx), EQ = expf(eps * Q);
    const float tr = eps * (EQ * vh[n * ldvh + k] + T_);
    const float zi = zin[n * ldzi + k];
    const float nw = fwd ? zi * ES + tr : ES * (zi - tr);
    const float zo = kp * zi + up * nw;
    zout[n * ldzo + k] = zo;
    if (xin_next != nullptr) xin_next[n * ldxn + k] = up * zo;      // next kept mask = this update mask
    acc += up * sx;
  }
  acc = wave_sum(acc);
  if (lane == 0) ld[n] += acc;
}
// xin = k1 * x for the first XNet evaluation of a step
__global__ void k_mask_first(const float* x, int ldx, float* xin, int ldxi, const float* masks, const unsigned char* dir,
                             int dir_all, int it, int T, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  bool fwd;
  const int s = row_of(dir, dir_all, n, it, T, fwd);
  const float m = masks[s * d + k];
  xin[n * ldxi + k] = (fwd ? m : 1.f - m) * x[n * ldx + k];
}
__global__ void k_kinetic(const float* v, float* K, float* ld, long long N, int d) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int k = 0; k < d; ++k) acc += 0.5f * v[n * d + k] * v[n * d + k];
  K[n] = acc;
  if (ld != nullptr) ld[n] = 0.f;
}
__global__ __launch_bounds__(256) void k_kinetic_staged(const float* v, float* K, float* ld, long long N, int d) {
  extern __shared__ float rsm[];
  const long long n0 = (long long)blockIdx.x * ROW_CPB;
  stage_rows(rsm, v, d, d, n0, N);
  __syncthreads();
  const long long n = n0 + threadIdx.x;
  if (threadIdx.x >= ROW_CPB || n >= N) return;
  float acc = 0.f;
  for (int k = 0; k < d; ++k) acc += 0.5f * rsm[threadIdx.x * d + k] * rsm[threadIdx.x * d + k];
  K[n] = acc;
  if (ld != nullptr) ld[n] = 0.f;
}
inline void launch_kinetic(hipStream_t s, const float* v, float* K, float* ld, long long N, int d) {
  const size_t lds = sizeof(float) * ROW_CPB * (size_t)d;
  if (lds <= 48 * 1024) hipLaunchKernelGGL(k_kinetic_staged, dim3((unsigned)((N + ROW_CPB - 1) / ROW_CPB)), dim3(256), lds, s, v, K, ld, N, d);
  else hipLaunchKernelGGL(k_kinetic, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, v, K, ld, N, d);
}
// accept probability (dynamics.py:302-309) + MH select (sampler.py:53-55): one thread per ELEMENT of the state (every thread of a
// chain forms the same p from the same five words; the select is a coalesced copy), dimension 0 writes the chain's outputs
__global__ void k_finish(const double* U0, const float* K0, const double* U1, const float* K1, const float* ld,
                         const float* u, const float* x0, const float* x1, int ldx1, float* p_out, float* logjac_out,
                         float* x_next, long long N, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long long n = i / d;
  const int k = (int)(i % d);
  const float p = accept_prob((float)((U0[n] - U1[n]) + ((double)K0[n] - (double)K1[n]) + (double)ld[n]));
  if (k == 0) {
    if (p_out != nullptr) p_out[n] = p;
    if (logjac_out != nullptr) logjac_out[n] = ld[n];
  }
  if (x_next != nullptr) {
    const bool acc = (p - u[n]) >= 0.f;
    x_next[i] = acc ? x1[n * ldx1 + k] : x0[i];
  }
}

// accept probability from precomputed energies (dynamics.py:302-309): H = U + |v|^2 / 2
__global__ void k_accept_from_energies(const float* U0, const float* v0, const float* U1, const float* v1,
                                       const float* lj, float* p, long long N, int d) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float K0 = 0.f, K1 = 0.f;
  for (int k = 0; k < d; ++k) {
    K0 += 0.5f * v0[n * d + k] * v0[n * d + k];
    K1 += 0.5f * v1[n * d + k] * v1[n * d + k];
  }
  p[n] = accept_prob((U0[n] + K0) - (U1[n] + K1) + lj[n]);
}

inline unsigned nblk(long long n) { return (unsigned)((n + 255) / 256); }

__global__ void k_f2d(const float* a, double* b, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = (double)a[i];
}

// Workspace slices of one 3-layer MLP evaluation: transposed weights (forward products), activations a1 / a2
// and their sigmoids s1 / s2 (= softplus', for the input gradient)
struct Mlp3Ws {
  float *w1t, *w2t, *w3t, *a1, *s1, *a2, *s2;
  // pre-split bf16 planes (gemm_pl_kernel), NULL = the fp32 path: the weights of the two decoder-sized layers in both
  // orientations, and the activations that only ever feed the next product (a1, a2, the BCE gradient, d a2)
  unsigned short *pw2t, *pw3t, *pw2, *pw3, *pa1, *pa2, *plg, *pda2;
  // the trainer's forward evaluations (vae_energy with a DecPoint): the same four weight matrices once more as f16x2 planes (two planes each),
  // NULL = the forward pass uses the bf16x3 planes above like the reverse sweep
  unsigned short *pw2t_h, *pw3t_h, *pw2_h, *pw3_h;
};

// L2hmcSplitArgs.gemm_mode / L2hmcTrainSplitArgs.gemm_mode of the call being served on this thread (set at the top of every
// entry point, so no state survives a call): 1 = the decoder-sized products run as bf16x3 (gemm_f32.hpp)
thread_local int t_gemm_bf3 = 0;
// 1 = the pre-split planes of the call being served are f16x2 (GemmArgs.pm; gemm_mode 3: the sampler only)
thread_local int t_plane_mode = 0;

inline GemmArgs gemm_args(const float* A, int lda, const float* B, int ldb, float* C, int ldc, long long M, int N, int K) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.bf3 = t_gemm_bf3;
  g.pm = t_plane_mode;
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K; g.beta = 1.f;
  return g;
}

void mlp3_transposes(hipStream_t s, const L2hmcMlp3& m, const Mlp3Ws& ws) {
  transpose_into(s, m.W1, m.n_in, m.n_h1, ws.w1t, m.n_in, 0);
  transpose_into(s, m.W2, m.n_h1, m.n_h2, ws.w2t, m.n_h1, 0);
  transpose_into(s, m.W3, m.n_h2, m.n_out, ws.w3t, m.n_h2, 0);
}

// a2 = softplus(softplus(x W1 + b1) W2 + b2)  (sigmoids kept when ws.s1 / ws.s2 are given); x has row stride ldx
void mlp3_hidden(hipStream_t s, const L2hmcMlp3& m, const float* x, int ldx, long long N, const Mlp3Ws& ws) {
  GemmArgs g = gemm_args(x, ldx, ws.w1t, m.n_in, ws.a1, m.n_h1, N, m.n_h1, m.n_in);
  g.bias = m.b1; g.C2 = ws.s1; g.ldc2 = m.n_h1;
  launch_gemm<EPI_BIAS_SOFTPLUS>(g, s, m.n_in <= 64 ? SHAPE_MID : SHAPE_AUTO);
  g = gemm_args(ws.a1, m.n_h1, ws.w2t, m.n_h1, ws.a2, m.n_h2, N, m.n_h2, m.n_h1);
  g.bias = m.b2; g.C2 = ws.s2; g.ldc2 = m.n_h2;
  launch_gemm<EPI_BIAS_SOFTPLUS>(g, s);
}

// out (N x n_out) = Linear-softplus-Linear-softplus-Linear(x)
void mlp3_forward(hipStream_t s, const L2hmcMlp3& m, const float* x, long long N, const Mlp3Ws& ws, float* out) {
  mlp3_hidden(s, m, x, m.n_in, N, ws);
  GemmArgs g = gemm_args(ws.a2, m.n_h2, ws.w3t, m.n_h2, out, m.n_out, N, m.n_out, m.n_h2);
  g.bias = m.b3;
  launch_gemm<EPI_BIAS>(g, s, m.n_out <= 256 ? SHAPE_MID : SHAPE_AUTO);
}

// column tiles of the logits GEMM (EPI_BCE leaves 2 row partials per tile): the shape launch_gemm picks for (N, n_pix)
inline int bce_tiles(long long N, int n_pix) { return (n_pix + gemm_tile_n(gemm_auto_shape(N, n_pix)) - 1) / gemm_tile_n(gemm_auto_shape(N, n_pix)); }
inline int bce_partials(long long N, int n_pix) { return gemm_waves_n(gemm_auto_shape(N, n_pix)) * bce_tiles(N, n_pix); }   // per chain
inline int bce_tiles_max(int n_pix) { return (n_pix + 63) / 64; }
// bf16 planes (gemm_xl.hpp): row stride of a K-extent, rows of a weight matrix with N outputs
inline int pld(int K) { return ceil_to(K, 32); }
inline long long prows(int N) { return ceil_to(N, XLP_TN); }

// The decoder's share of one trajectory point, kept for the trainer's reverse sweep (train_split.hpp): s1, s2 (sigmoids =
// softplus'), sigma' of the logits, and the raw reverse products b2 = r W3^T, b1 = c2 W2^T (r = sigmoid(logit) - aux, c2 = s2 b2)
struct DecPoint { float *s1, *s2, *rd, *b2, *b1; };
__global__ void k_sigd(const float* r, const float* t, float* out, long long n);     // train_split.hpp

// U (N) and grad (N x d, row stride ldg) of the VAE latent posterior at z (row stride ldz) (mnist_vae.py:122-126):
// six GEMMs, every bias / softplus / sigmoid / BCE / chain-rule product fused into their epilogues; lg (N x n_pix)
// and rowsum (N x 2 tiles) are scratch.  The transposed decoder weights must already be in ws (mlp3_transposes).
// With `pt` the point's DecPoint is left behind: the sigmoids go to pt, lg is written in fp32 on the planes path too (k_sigd
// reads it) and the two reverse products leave their raw form through C2; the weight planes are the f16x2 ones where ws has them.
// Returns the first error of the pre-split launches (their LDS-size request can be refused by a device), L2HMC_OK otherwise.
int vae_energy(hipStream_t s, const L2hmcMlp3& dec, const float* aux, const float* z, int ldz, long long N, int d,
               const Mlp3Ws& ws0, float* lg, float* rowsum, float* U, double* Ud, float* grad, int ldg, float beta = 1.f,
               const DecPoint* pt = nullptr) {
  Mlp3Ws ws = ws0;
  if (pt != nullptr) { ws.s1 = pt->s1; ws.s2 = pt->s2; }
  const long long npix = N * dec.n_out;
  if (ws.pa1 != nullptr) {
    int rc = L2HMC_OK, r1;
    // ---- pre-split form (gemm_mode 1 / 3 at decoder sizes, gemm_xl.hpp): every activation that only feeds the next product is
    //      written as planes by its producer's epilogue; the four decoder-sized products read planes on both sides
    //      (gemm_xlp_kernel: bit-identical per product to the in-loop split).  Plane row strides are whole k-tiles (pld) and
    //      the weight planes whole tiles of rows (prows), zero-padded.
    const int l1 = pld(dec.n_h1), l2 = pld(dec.n_h2), lo = pld(dec.n_out);
    const long long n1 = N * l1, n2 = N * l2, no = N * lo;
    // (the trainer's gemm_mode 3: this evaluation is the SAMPLER's -- activations, logits, BCE gradients of O(1) -- and runs on
    //  f16x2 planes like it, with the weights' f16 planes; the reverse sweep's tangents and adjoints keep bf16x3: t_plane_mode)
    const int pm_keep = t_plane_mode;
    const bool h16 = ws.pw2t_h != nullptr;
    if (h16) t_plane_mode = 1;
    const unsigned short *qw2t = h16 ? ws.pw2t_h : ws.pw2t, *qw3t = h16 ? ws.pw3t_h : ws.pw3t, *qw2 = h16 ? ws.pw2_h : ws.pw2,
                         *qw3 = h16 ? ws.pw3_h : ws.pw3;
    GemmArgs g = gemm_args(z, ldz, ws.w1t, dec.n_in, nullptr, dec.n_h1, N, dec.n_h1, dec.n_in);
    g.bias = dec.b1; g.C2 = ws.s1; g.ldc2 = dec.n_h1; g.Cp = ws.pa1; g.cp_plane = n1; g.ldcp = l1;
    launch_gemm<EPI_BIAS_SOFTPLUS>(g, s, dec.n_in <= 64 ? SHAPE_MID : SHAPE_AUTO);                 // a1 (planes), s1
    g = gemm_args(nullptr, 0, nullptr, 0, nullptr, dec.n_h2, N, dec.n_h2, dec.n_h1);
    g.Ap = ws.pa1; g.ap_plane = n1; g.ldap = l1; g.Bp = qw2t; g.bp_plane = prows(dec.n_h2) * l1; g.ldbp = l1;
    g.bias = dec.b2; g.C2 = ws.s2; g.ldc2 = dec.n_h2; g.Cp = ws.pa2; g.cp_plane = n2; g.ldcp = l2;
    if ((r1 = launch_gemm_planes<EPI_BIAS_SOFTPLUS>(g, s)) != L2HMC_OK) rc = rc ? rc : r1;          // a2 (planes), s2
    g = gemm_args(nullptr, 0, nullptr, 0, pt != nullptr ? lg : nullptr, dec.n_out, N, dec.n_out, dec.n_h2);
    g.Ap = ws.pa2; g.ap_plane = n2; g.ldap = l2; g.Bp = qw3t; g.bp_plane = prows(dec.n_out) * l2; g.ldbp = l2;
    g.bias = dec.b3; g.E = aux; g.lde = dec.n_out; g.rowsum = rowsum; g.n_tiles = bce_tiles_planes(dec.n_out); g.beta = beta;
    g.Cp = ws.plg; g.cp_plane = no; g.ldcp = lo;
    if ((r1 = launch_gemm_planes<EPI_BCE>(g, s)) != L2HMC_OK) rc = rc ? rc : r1;                    // beta (sigmoid(logit) - aux) (planes)
    if (U != nullptr || Ud != nullptr)
      launch_vae_U(s, rowsum, 2 * bce_tiles_planes(dec.n_out), z, ldz, d, U, Ud, N);
    if (pt != nullptr) hipLaunchKernelGGL(k_sigd, dim3(nblk(npix)), dim3(256), 0, s, lg, aux, pt->rd, npix);
    if (grad == nullptr) { t_plane_mode = pm_keep; return rc; }
    g = gemm_args(nullptr, 0, nullptr, 0, nullptr, dec.n_h2, N, dec.n_h2, dec.n_out);
    g.Ap = ws.plg; g.ap_plane = no; g.ldap = lo; g.Bp = qw3; g.bp_plane = prows(dec.n_h2) * lo; g.ldbp = lo;
    g.E = ws.s2; g.lde = dec.n_h2; g.Cp = ws.pda2; g.cp_plane = n2; g.ldcp = l2;
    if (pt != nullptr) { g.C2 = pt->b2; g.ldc2 = dec.n_h2; }
    if ((r1 = launch_gemm_planes<EPI_MUL>(g, s)) != L2HMC_OK) rc = rc ? rc : r1;                    // d a2 = s2 b2 (planes), b2
    g = gemm_args(nullptr, 0, nullptr, 0, ws.a1, dec.n_h1, N, dec.n_h1, dec.n_h2);
    g.Ap = ws.pda2; g.ap_plane = n2; g.ldap = l2; g.Bp = qw2; g.bp_plane = prows(dec.n_h1) * l2; g.ldbp = l2;
    g.E = ws.s1; g.lde = dec.n_h1;
    if (pt != nullptr) { g.C2 = pt->b1; g.ldc2 = dec.n_h1; }
    if ((r1 = launch_gemm_planes<EPI_MUL>(g, s)) != L2HMC_OK) rc = rc ? rc : r1;                    // d a1 = s1 b1 (fp32: the K = 1024, N = d product reads it), b1
    t_plane_mode = pm_keep;
    g = gemm_args(ws.a1, dec.n_h1, dec.W1, dec.n_h1, grad, ldg, N, d, dec.n_h1);
    g.E = z; g.lde = ldz;
    launch_gemm<EPI_ADD>(g, s, d <= 64 ? SHAPE_SKINNY : SHAPE_MID);
    return rc;
  }
  mlp3_hidden(s, dec, z, ldz, N, ws);
  GemmArgs g = gemm_args(ws.a2, dec.n_h2, ws.w3t, dec.n_h2, lg, dec.n_out, N, dec.n_out, dec.n_h2);
  g.bias = dec.b3; g.E = aux; g.lde = dec.n_out; g.rowsum = rowsum; g.n_tiles = bce_tiles(N, dec.n_out); g.beta = beta;
  launch_gemm<EPI_BCE>(g, s);                                     // lg := beta (sigmoid(logit) - aux)
  if (U != nullptr || Ud != nullptr)
    launch_vae_U(s, rowsum, bce_partials(N, dec.n_out), z, ldz, d, U, Ud, N);
  if (pt != nullptr) hipLaunchKernelGGL(k_sigd, dim3(nblk(npix)), dim3(256), 0, s, lg, aux, pt->rd, npix);
  if (grad == nullptr) return L2HMC_OK;
  // d a2 = dl W3^T (.) sigmoid(p2);  d a1 = d a2 W2^T (.) sigmoid(p1);  d z = d a1 W1^T + z
  g = gemm_args(lg, dec.n_out, dec.W3, dec.n_out, ws.a2, dec.n_h2, N, dec.n_h2, dec.n_out);
  g.E = ws.s2; g.lde = dec.n_h2;
  if (pt != nullptr) { g.C2 = pt->b2; g.ldc2 = dec.n_h2; }
  launch_gemm<EPI_MUL>(g, s);
  g = gemm_args(ws.a2, dec.n_h2, dec.W2, dec.n_h2, ws.a1, dec.n_h1, N, dec.n_h1, dec.n_h2);
  g.E = ws.s1; g.lde = dec.n_h1;
  if (pt != nullptr) { g.C2 = pt->b1; g.ldc2 = dec.n_h1; }
  launch_gemm<EPI_MUL>(g, s);
  g = gemm_args(ws.a1, dec.n_h1, dec.W1, dec.n_h1, grad, ldg, N, d, dec.n_h1);
  g.E = z; g.lde = ldz;
  launch_gemm<EPI_ADD>(g, s, d <= 64 ? SHAPE_SKINNY : SHAPE_MID);
  return L2HMC_OK;
}

struct SplitPlan {
  long long total;
  long long abv, abx, vc, y, h1, h2, out3, aux_h, tb, U0, K0, U1, K1, ld, rowsum, lg;   // abv = [x | grad U], abx = [v_h | masked x]
  long long xp, gp, uf;                                          // built-in energies: contiguous x, grad U, fp32 U
  long long dw1t, dw2t, dw3t, a1, s1, a2, s2;                    // decoder
  long long ew1t, ew2t, ew3t, e1, e2;                            // image branch
  long long nx12t, nx4t, nxht, nv12t, nv4t, nvht;                // S/T/Q nets: [W1; W2]^T, W4^T, [Ws | Wt | Wq]^T
  bool planes;                                                   // the decoder products can take the pre-split form at this size
  long long pw2t, pw3t, pw2, pw3, pa1, pa2, plg, pda2;           // bf16 planes (3 x elements x 2 bytes each), in floats
};

SplitPlan plan_split(long long N, int d, int H, int T, const L2hmcMlp3* enc, const L2hmcMlp3* dec) {
  SplitPlan p;
  long long o = 0;
  auto take = [&](long long n) { const long long at = o; o += (n + 3) & ~3LL; return at; };
  p.abv = take(N * 2 * d); p.abx = take(N * 2 * d); p.vc = take(N * d); p.y = take(N * d);
  p.h1 = take(N * H); p.h2 = take(N * H); p.out3 = take(N * 3 * d);
  p.aux_h = take(enc ? N * H : 0); p.tb = take(2LL * T * H);
  p.U0 = take(2 * N); p.K0 = take(N); p.U1 = take(2 * N); p.K1 = take(N); p.ld = take(N);      // U0 / U1: doubles
  p.rowsum = take(dec ? N * 2 * bce_tiles_max(dec->n_out) : 0);
  p.lg = take(dec ? N * dec->n_out : 0);
  p.dw1t = take(dec ? (long long)dec->n_in * dec->n_h1 : 0); p.dw2t = take(dec ? (long long)dec->n_h1 * dec->n_h2 : 0);
  p.dw3t = take(dec ? (long long)dec->n_h2 * dec->n_out : 0);
  p.a1 = take(dec ? N * dec->n_h1 : 0); p.s1 = take(dec ? N * dec->n_h1 : 0);
  p.a2 = take(dec ? N * dec->n_h2 : 0); p.s2 = take(dec ? N * dec->n_h2 : 0);
  p.xp = take(dec ? 0 : N * d); p.gp = take(dec ? 0 : N * d); p.uf = take(dec ? 0 : N);
  p.ew1t = take(enc ? (long long)enc->n_in * enc->n_h1 : 0); p.ew2t = take(enc ? (long long)enc->n_h1 * enc->n_h2 : 0);
  p.ew3t = take(enc ? (long long)enc->n_h2 * enc->n_out : 0);
  p.e1 = take(enc ? N * enc->n_h1 : 0); p.e2 = take(enc ? N * enc->n_h2 : 0);
  // S/T/Q nets: transposed copies, rows and K zero-padded to multiples of 16 (net_eval_kernel has no guards)
  const long long n12 = (long long)ceil16(H) * ceil16(2 * d), n4 = (long long)ceil16(H) * ceil16(H), nh = (long long)ceil16(3 * d) * ceil16(H);
  p.nx12t = take(n12); p.nx4t = take(n4); p.nxht = take(nh);
  p.nv12t = take(n12); p.nv4t = take(n4); p.nvht = take(nh);
  // bf16 planes of the decoder's two big layers and of the activations between them (gemm_xl.hpp): 3 planes x 2 bytes
  p.planes = dec != nullptr && gemm_planes_ok(N, dec->n_h2, dec->n_h1) && gemm_planes_ok(N, dec->n_out, dec->n_h2) &&
             gemm_planes_ok(N, dec->n_h2, dec->n_out) && gemm_planes_ok(N, dec->n_h1, dec->n_h2) && dec->n_h1 % 4 == 0;
  auto takep = [&](long long elems) { return take(p.planes ? (elems * 3 + 1) / 2 : 0); };
  if (dec != nullptr) {
    p.pw2t = takep(prows(dec->n_h2) * pld(dec->n_h1)); p.pw3t = takep(prows(dec->n_out) * pld(dec->n_h2));
    p.pw2 = takep(prows(dec->n_h1) * pld(dec->n_h2)); p.pw3 = takep(prows(dec->n_h2) * pld(dec->n_out));
    p.pa1 = takep(N * pld(dec->n_h1)); p.pa2 = takep(N * pld(dec->n_h2));
    p.plg = takep(N * pld(dec->n_out)); p.pda2 = takep(N * pld(dec->n_h2));
  } else {
    p.pw2t = p.pw3t = p.pw2 = p.pw3 = p.pa1 = p.pa2 = p.plg = p.pda2 = o;
  }
  p.total = o;
  return p;
}

int check_mlp(const L2hmcMlp3* m, const char* what) {
  if (!m || !m->W1 || !m->b1 || !m->W2 || !m->b2 || !m->W3 || !m->b3 || m->n_in < 1 || m->n_h1 < 1 ||
      m->n_h2 < 1 || m->n_out < 1)
    return fail(L2HMC_ERR_ARG, "%s: incomplete 3-layer MLP description", what);
  return L2HMC_OK;
}

// ---- the host path of the engine: what l2hmc_trajectory_split (below) and l2hmc_train_split_grad (train_split.hpp) share -----
// the launch form of the S/T/Q net evaluations of a call (plan_nets)
struct NetPlan {
  int cb;                    // chain blocks of 16 per workgroup
  unsigned blocks;
  size_t ne_lds, nb_lds;     // dynamic LDS of net_eval_kernel / net_bwd_kernel (nb_lds = 0: no reverse in this call)
  bool fused;                // one launch per evaluation (and per reverse); else three products each
};
// where an evaluation's hidden activations and raw head products go when the caller keeps them (the trainer's stash)
struct NetKeep { float *h1, *h2, *out3; };

// Everything both entry points derive from their argument block.  engine_target fills the upper half from the block alone
// (nothing is dereferenced: the checks come after it), engine_bind the workspace views once the block has passed them.
struct EngineCtx {
  long long N;
  int d, H, T, L;                                   // L = 2 d: row stride of [x | grad U] and [v_h | masked x]
  hipStream_t s;
  void* stream;                                     // the same stream as the callbacks and l2hmc_energy take it
  bool user, builtin, vae, unets, hmc;              // energy by callback / built-in target / decoder posterior; nets by callback; HMC mode
  const unsigned char* dir;
  int dall;
  const float *masks, *trig, *alpha, *aux;
  float eps_host, beta, temp;                       // beta: bce_scale of the decoder posterior; temp: the decoder posterior is tempered behind
  const L2hmcEnergy* energy;
  L2hmcEnergyCallback energy_cb;
  void* energy_cb_user;
  L2hmcNetCallback net_cb;
  void* net_cb_user;
  const L2hmcMlp3 *dec, *enc;
  const L2hmcNet* nets[2];                          // [X, V]; an empty net (lam_s == NULL) in HMC mode and with net_cb
  // ---- engine_bind
  float* w;
  SplitPlan p;
  bool use_planes;                                  // the decoder-sized products take the pre-split form in this call
  Mlp3Ws dws, ews;                                  // decoder (with its plane views) and image branch
  float *w12t[2], *w4t[2], *wht[2];                 // per net: [W1; W2]^T (H x 2d), W4^T (H x H), [Ws | Wt | Wq]^T (3d x H)
  float *ld, *tb, *aux_h, *h1, *h2, *out3;          // h1 / h2 / out3: scratch of an evaluation nobody keeps
  NetPlan np;                                       // plan_nets
};

// `temperature_only`: the block's `energy` only carries a temperature (the trainer's kind 0), the target is one of the others
template <class A>
EngineCtx engine_target(const A& a, void* stream, bool hmc, bool temperature_only) {
  static const L2hmcNet no_net = {};
  EngineCtx c = {};
  c.user = a.energy_cb != nullptr;
  c.builtin = a.energy != nullptr && !temperature_only;
  c.vae = !c.user && !c.builtin;
  c.unets = a.net_cb != nullptr;
  c.hmc = hmc;
  c.N = a.n_chains; c.d = a.d; c.H = c.unets ? 4 : a.H; c.T = a.T; c.L = 2 * a.d;    // (caller-supplied nets: no hidden activations are planned for)
  c.s = (hipStream_t)stream; c.stream = stream;
  c.dir = a.direction; c.dall = a.direction_all; c.masks = a.masks; c.trig = a.trig; c.alpha = a.alpha; c.eps_host = a.eps_host;
  c.aux = a.aux; c.beta = 1.f; c.temp = 1.f;
  c.energy = a.energy; c.energy_cb = a.energy_cb; c.energy_cb_user = a.energy_cb_user;
  c.net_cb = a.net_cb; c.net_cb_user = a.net_cb_user;
  c.dec = a.decoder; c.enc = a.aux_encoder;
  c.nets[0] = (hmc || c.unets) ? &no_net : a.xnet;
  c.nets[1] = (hmc || c.unets) ? &no_net : a.vnet;
  return c;
}

// The refusals both entry points make in the same words.  Each entry point calls them where it has always made them, between
// the checks that are its own: the first complaint about a block with several faults stays what it was.
inline int check_dims(const EngineCtx& c) {
  return (c.N < 0 || c.d < 1 || c.H < 1 || c.T < 1) ? fail(L2HMC_ERR_ARG, "bad n_chains / d / H / T%s") : L2HMC_OK;
}
inline int check_decoder_width(const EngineCtx& c) {
  return (c.vae && c.dec->n_in != c.d) ? fail(L2HMC_ERR_ARG, "decoder input width != d%s") : L2HMC_OK;
}
inline int check_image_branch(const EngineCtx& c) {
  return (c.enc && (c.enc->n_out != c.H || (c.vae && c.enc->n_in != c.dec->n_out)))
             ? fail(L2HMC_ERR_ARG, "aux_encoder must map (N, n_pix) -> (N, H)%s") : L2HMC_OK;
}
inline int check_eps(const EngineCtx& c) {
  return (!c.alpha && !(c.eps_host > 0.f)) ? fail(L2HMC_ERR_ARG, "eps must be > 0%s") : L2HMC_OK;
}
inline int check_workspace(long long have, long long need) {
  return have < need ? fail(L2HMC_ERR_ARG, "workspace too small: need %s%lld floats", "", need) : L2HMC_OK;
}

// the workspace views of a block that passed its checks; gemm_mode 1 / 3 take the planes where the plan has them
inline void engine_bind(EngineCtx& c, float* w, const SplitPlan& p, int gemm_mode) {
  static const L2hmcMlp3 no_dec = {};
  if (!c.vae) c.dec = &no_dec;
  c.w = w; c.p = p;
  c.use_planes = c.vae && p.planes && (gemm_mode == 1 || gemm_mode == 3);
  c.dws = Mlp3Ws{w + p.dw1t, w + p.dw2t, w + p.dw3t, w + p.a1, w + p.s1, w + p.a2, w + p.s2};
  if (c.use_planes) {
    auto us = [&](long long off) { return reinterpret_cast<unsigned short*>(w + off); };
    c.dws.pw2t = us(p.pw2t); c.dws.pw3t = us(p.pw3t); c.dws.pw2 = us(p.pw2); c.dws.pw3 = us(p.pw3);
    c.dws.pa1 = us(p.pa1); c.dws.pa2 = us(p.pa2); c.dws.plg = us(p.plg); c.dws.pda2 = us(p.pda2);
  }
  c.ews = Mlp3Ws{w + p.ew1t, w + p.ew2t, w + p.ew3t, w + p.e1, nullptr, w + p.e2, nullptr};
  c.w12t[0] = w + p.nx12t; c.w12t[1] = w + p.nv12t; c.w4t[0] = w + p.nx4t; c.w4t[1] = w + p.nv4t;
  c.wht[0] = w + p.nxht; c.wht[1] = w + p.nvht;
  c.ld = w + p.ld; c.tb = w + p.tb; c.aux_h = c.enc ? w + p.aux_h : nullptr;
  c.h1 = w + p.h1; c.h2 = w + p.h2; c.out3 = w + p.out3;
}

// the LDS-size requests of the three epilogues the decoder posterior launches on planes, up front: a device that refuses
// them refuses the call before anything is enqueued
inline int planes_prepare() {
  int rc;
  if (t_plane_mode) {
    if ((rc = gemm_planes_prepare<EPI_BIAS_SOFTPLUS, 1>()) != L2HMC_OK || (rc = gemm_planes_prepare<EPI_BCE, 1>()) != L2HMC_OK ||
        (rc = gemm_planes_prepare<EPI_MUL, 1>()) != L2HMC_OK)
      return rc;
  } else if ((rc = gemm_planes_prepare<EPI_BIAS_SOFTPLUS>()) != L2HMC_OK || (rc = gemm_planes_prepare<EPI_BCE>()) != L2HMC_OK ||
             (rc = gemm_planes_prepare<EPI_MUL>()) != L2HMC_OK)
    return rc;
  return L2HMC_OK;
}

// One net evaluation is out3 = relu(relu([a | b] [W1; W2] + time + aux_h) W4 + b4) [Ws|Wt|Wq] (the head biases are added by
// the update).  H % 4 == 0, d even, K <= 256 and tiles that fit the LDS: ONE launch of net_eval_kernel (activations resident in
// LDS, the half-update fused behind the heads) -- and of net_bwd_kernel for its reverse; otherwise three GEMMs with fused
// epilogues on 64 x 64 tiles.  The widest K is 2 d forward (the first layer's inputs) and 3 d once the reverse runs (the head
// cotangents): `with_reverse` is the trainer's.  net_mode 1 asks for the three products (A/B measurements and tests).
// (32 chains per workgroup -- every weight fragment streamed from L2 feeding two MFMAs, net_eval_kernel<2> -- was
//  measured twice at 8192 chains: with one workgroup per CU (88 KB of LDS) the evaluation is 25 % slower than with 16
//  chains, with two per CU (69 KB after the head products moved into the dead first activation) still 8 % slower:
//  occupancy, not L2 traffic, is what this kernel lives on)
// 32 chains on 8 waves (one workgroup per CU, half the L2 weight traffic) once that still fills the chip
// (Round 5: at config 5's shapes the 120 launches of 64 x 64-tile products these replace were 2.5 ms of a 10.5 ms step.)
inline int plan_nets(EngineCtx& c, bool with_reverse, int net_mode) {
  const int d = c.d, H = c.H;
  NetPlan& n = c.np;
  n.cb = c.N >= 32LL * device_cus() ? 2 : 1;        // (32 chains per CU = one 8-wave workgroup each; 8192 on 256 CUs)
  n.blocks = (unsigned)((c.N + 16 * n.cb - 1) / (16 * n.cb));
  n.ne_lds = net_eval_lds_bytes(d, H, n.cb);
  n.nb_lds = with_reverse ? net_bwd_lds_bytes(d, H, n.cb) : 0;
  n.fused = !c.unets && (H % 4 == 0) && (d % 2 == 0) && ceil16(H) <= 16 * NE_MAXKT && ceil16((with_reverse ? 3 : 2) * d) <= 16 * NE_MAXKT &&
            n.ne_lds <= 160 * 1024 && n.nb_lds <= 160 * 1024 && net_mode == 0;
  if (!n.fused || c.hmc) return L2HMC_OK;
  hipError_t e = hipSuccess;
  if (n.ne_lds > 48 * 1024)
    e = hipFuncSetAttribute(net_eval_fn(n.cb, d, H), hipFuncAttributeMaxDynamicSharedMemorySize, (int)n.ne_lds);
  if (e == hipSuccess && n.nb_lds > 48 * 1024)
    e = hipFuncSetAttribute(net_bwd_fn(n.cb, d, H), hipFuncAttributeMaxDynamicSharedMemorySize, (int)n.nb_lds);
  return e != hipSuccess ? fail(L2HMC_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e)) : L2HMC_OK;
}

// ---- preparation, once per call; `kept`: still in the workspace from the previous call (L2hmcSplitArgs.reuse: the caller vouches)
// decoder: transposed copies; on the planes path the two decoder-sized layers in both orientations as planes of the call's
// arithmetic (t_plane_mode) -- and once more as f16x2 planes where dws has room for them (the trainer's gemm_mode 3) --, and the
// activations' padding up to a whole k-tile zeroed (the epilogues write the columns of an activation only)
inline void prepare_decoder(const EngineCtx& c, bool kept) {
  if (!c.vae || kept) return;
  const L2hmcMlp3& dec = *c.dec;
  const Mlp3Ws& ws = c.dws;
  mlp3_transposes(c.s, dec, ws);
  if (!c.use_planes) return;
  auto weight_planes = [&](unsigned short* p2t, unsigned short* p3t, unsigned short* p2, unsigned short* p3, int pm) {
    to_planes(c.s, ws.w2t, dec.n_h1, dec.n_h2, dec.n_h1, p2t, prows(dec.n_h2), pld(dec.n_h1), pm);
    to_planes(c.s, ws.w3t, dec.n_h2, dec.n_out, dec.n_h2, p3t, prows(dec.n_out), pld(dec.n_h2), pm);
    to_planes(c.s, dec.W2, dec.n_h2, dec.n_h1, dec.n_h2, p2, prows(dec.n_h1), pld(dec.n_h2), pm);
    to_planes(c.s, dec.W3, dec.n_out, dec.n_h2, dec.n_out, p3, prows(dec.n_h2), pld(dec.n_out), pm);
  };
  weight_planes(ws.pw2t, ws.pw3t, ws.pw2, ws.pw3, t_plane_mode);
  if (ws.pw2t_h != nullptr) weight_planes(ws.pw2t_h, ws.pw3t_h, ws.pw2_h, ws.pw3_h, 1);
  planes_zero_pad(c.s, ws.pa1, c.N, dec.n_h1, pld(dec.n_h1));
  planes_zero_pad(c.s, ws.pa2, c.N, dec.n_h2, pld(dec.n_h2));
  planes_zero_pad(c.s, ws.plg, c.N, dec.n_out, pld(dec.n_out));
  planes_zero_pad(c.s, ws.pda2, c.N, dec.n_h2, pld(dec.n_h2));
}
// the image branch is step-invariant: once per trajectory, not 4T times
inline void prepare_image_branch(const EngineCtx& c, bool kept_weights, bool kept_aux_h) {
  if (!c.enc || c.hmc) return;
  if (!kept_weights) mlp3_transposes(c.s, *c.enc, c.ews);
  if (!kept_aux_h) mlp3_forward(c.s, *c.enc, c.aux, c.N, c.ews, c.aux_h);
}
// S/T/Q nets: the time table and the zero-padded transposed copies; after_net(i) follows net i's copies on the stream
template <class F>
inline void prepare_nets(const EngineCtx& c, bool kept, F&& after_net) {
  if (c.hmc || c.unets || kept) return;
  const int d = c.d, H = c.H, K1p = ceil16(c.L), Hp = ceil16(H);
  hipLaunchKernelGGL(k_time_table, dim3(nblk(2LL * c.T * H)), dim3(256), 0, c.s, *c.nets[0], *c.nets[1], c.trig, c.T, H, c.tb);
  (void)hipMemsetAsync(c.w12t[0], 0, sizeof(float) * (size_t)(c.p.nvht + (long long)ceil16(3 * d) * Hp - c.p.nx12t), c.s);
  for (int i = 0; i < 2; ++i) {
    transpose_into(c.s, c.nets[i]->W1, d, H, c.w12t[i], K1p, 0);
    transpose_into(c.s, c.nets[i]->W2, d, H, c.w12t[i], K1p, d);
    transpose_into(c.s, c.nets[i]->W4, H, H, c.w4t[i], Hp, 0);
    transpose_into(c.s, c.nets[i]->Ws, H, d, c.wht[i], Hp, 0);
    transpose_into(c.s, c.nets[i]->Wt, H, d, c.wht[i] + (long long)d * Hp, Hp, 0);
    transpose_into(c.s, c.nets[i]->Wq, H, d, c.wht[i] + 2LL * d * Hp, Hp, 0);
    after_net(i);
  }
}

// U (double, optional) and grad U at the point held in columns [0, d) of `ab` (row stride L) -> columns [d, 2 d): the caller's
// callback, the decoder posterior (six GEMMs; `keep`: the point's DecPoint stays behind) or one of the built-in targets (the
// fused kernels' own energy kernel on a contiguous copy of x)
__global__ void k_temper(float* g, int ldg, double* U, float it, double itd, long long N, int d);     // train_split.hpp
inline int energy_at(const EngineCtx& c, float* ab, double* Ud, const DecPoint* keep = nullptr) {
  const long long N = c.N;
  const int d = c.d, L = c.L;
  float* w = c.w;
  if (c.user) {      // the caller enqueues U / grad U of the (N, d) block at ab (row stride L) on this stream
    const int r = c.energy_cb(c.energy_cb_user, ab, L, N, d, Ud, ab + d, L, c.stream);
    return r ? fail(L2HMC_ERR_ARG, "the energy callback failed (returned %s%lld)", "", (long long)r) : L2HMC_OK;
  }
  if (c.vae) {
    const int r = vae_energy(c.s, *c.dec, c.aux, ab, L, N, d, c.dws, w + c.p.lg, w + c.p.rowsum, nullptr, Ud, ab + d, L, c.beta, keep);
    if (r) return r;
    if (c.temp != 1.f)     // evaluated plain and tempered behind; the built-in energies and the callbacks return U / temperature themselves
      hipLaunchKernelGGL(k_temper, dim3(nblk(N * d)), dim3(256), 0, c.s, ab + d, L, Ud, 1.f / c.temp, 1.0 / (double)c.temp, N, d);
    return L2HMC_OK;
  }
  (void)hipMemcpy2DAsync(w + c.p.xp, sizeof(float) * d, ab, sizeof(float) * L, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, c.s);
  const int r = l2hmc_energy(c.energy, w + c.p.xp, N, d, Ud ? w + c.p.uf : nullptr, w + c.p.gp, c.stream);
  if (r) return r;
  (void)hipMemcpy2DAsync(ab + d, sizeof(float) * L, w + c.p.gp, sizeof(float) * d, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, c.s);
  if (Ud) hipLaunchKernelGGL(k_f2d, dim3(nblk(N)), dim3(256), 0, c.s, w + c.p.uf, Ud, N);
  return L2HMC_OK;
}

// the half-update that consumes a net evaluation: momentum (optionally with xin = k1 x for the X-net evaluation that
// follows) and masked position (optionally with the masked input of the next evaluation)
inline NetEvalArgs::Update v_update(int L, const float* vin, int ldvi, const float* g, float* vout, int ldvo, const float* x, float* xin) {
  NetEvalArgs::Update u = {};
  u.mode = 1; u.vin = vin; u.ldvi = ldvi; u.g = g; u.ldg = L; u.vout = vout; u.ldvo = ldvo;
  if (xin != nullptr) { u.x = x; u.ldx = L; u.xin = xin; u.ldxi = L; }
  return u;
}
inline NetEvalArgs::Update x_update(int L, const float* zin, int ldzi, const float* vh, float* zout, int ldzo, float* xin_next, int second) {
  NetEvalArgs::Update u = {};
  u.mode = 2; u.zin = zin; u.ldzi = ldzi; u.vh = vh; u.ldvh = L; u.zout = zout; u.ldzo = ldzo;
  u.xin_next = xin_next; u.ldxn = L; u.second = second;
  return u;
}

// One evaluation of net `net` (0 = X, 1 = V) on the inputs `ab` at leapfrog step `it`, and the half-update `upd` that consumes
// it: fused into net_eval_kernel when that kernel runs (plan_nets), else the stand-alone update kernel(s) follow the three
// GEMMs or the caller's net.  `keep`: both hidden activations and the raw head products also go to HBM (the trainer's stash).
inline int net_eval(const EngineCtx& c, int net, const float* ab, int it, NetEvalArgs::Update upd, const NetKeep* keep = nullptr) {
  const long long N = c.N;
  const int d = c.d, H = c.H, L = c.L, T = c.T;
  const L2hmcNet& nw = *c.nets[net];
  float *h1 = keep ? keep->h1 : c.h1, *h2 = keep ? keep->h2 : c.h2, *out3 = keep ? keep->out3 : c.out3;
  const float* tb = c.tb + (long long)net * T * H;
  upd.bs = nw.bs; upd.bt = nw.bt; upd.bq = nw.bq; upd.lam_s = nw.lam_s; upd.lam_q = nw.lam_q;
  upd.alpha = c.alpha; upd.eps_host = c.eps_host; upd.ld = c.ld; upd.masks = c.masks;
  if (c.np.fused) {
    NetEvalArgs na = {};
    na.AB = ab; na.ldab = L; na.W12t = c.w12t[net]; na.W4t = c.w4t[net]; na.Wht = c.wht[net]; na.b4 = nw.b4; na.tb = tb; na.auxh = c.aux_h;
    na.dir = c.dir; na.dir_all = c.dall; na.it = it; na.T = T; na.out3 = out3; na.M = (int)N; na.d = d; na.H = H;
    if (keep) { na.keep_h1 = h1; na.keep_h2 = h2; na.keep_out3 = out3; }
    na.upd = upd;
    launch_net_eval(c.np.cb, c.np.blocks, c.np.ne_lds, c.s, na);
    return L2HMC_OK;
  }
  if (c.unets) {     // the caller's net writes the final S | T | Q into out3 (nw is empty: the update kernels take them as they are)
    const int r = c.net_cb(c.net_cb_user, net, ab, L, N, d, it, c.dir, c.dall, out3, c.stream);
    if (r) return fail(L2HMC_ERR_ARG, "the net callback failed (returned %s%lld)", "", (long long)r);
  } else {
    GemmArgs ga = gemm_args(ab, L, c.w12t[net], ceil16(L), h1, H, N, H, L);
    ga.E = c.aux_h; ga.lde = H; ga.tb = tb; ga.dir = c.dir; ga.dir_all = c.dall; ga.it = it; ga.T = T;
    launch_gemm<EPI_NET1>(ga, c.s, SHAPE_MID);
    ga = gemm_args(h1, H, c.w4t[net], ceil16(H), h2, H, N, H, H);
    ga.bias = nw.b4;
    launch_gemm<EPI_BIAS_RELU>(ga, c.s, SHAPE_MID);
    ga = gemm_args(h2, H, c.wht[net], ceil16(H), out3, 3 * d, N, 3 * d, H);
    launch_gemm<EPI_BIAS>(ga, c.s, SHAPE_MID);
  }
  const unsigned nw4 = (unsigned)((N + 3) / 4);                  // one wave per chain, 4 per workgroup
  if (upd.mode == 1) {
    hipLaunchKernelGGL(k_v_half, dim3(nw4), dim3(256), 0, c.s, out3, nw, upd.vin, upd.ldvi, upd.g, upd.ldg, upd.vout, upd.ldvo, c.ld,
                       c.dir, c.dall, c.alpha, c.eps_host, N, d);
    if (upd.xin != nullptr)
      hipLaunchKernelGGL(k_mask_first, dim3(nblk(N * d)), dim3(256), 0, c.s, upd.x, upd.ldx, upd.xin, upd.ldxi, c.masks, c.dir, c.dall,
                         it, T, N, d);
  } else {
    hipLaunchKernelGGL(k_x_half, dim3(nw4), dim3(256), 0, c.s, out3, nw, upd.zin, upd.ldzi, upd.vh, upd.ldvh, upd.zout, upd.ldzo,
                       upd.xin_next, upd.ldxn, c.ld, c.masks, c.dir, c.dall, it, T, upd.second, c.alpha, c.eps_host, N, d);
  }
  return L2HMC_OK;
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" {

int64_t l2hmc_split_workspace_floats(int64_t n_chains, int32_t d, int32_t H, int32_t T,
                                     const L2hmcMlp3* aux_encoder, const L2hmcMlp3* decoder) {
  if (n_chains < 0 || d < 1 || H < 1 || T < 1) return fail(L2HMC_ERR_ARG, "l2hmc_split_workspace_floats: bad argument%s");
  return plan_split(n_chains, d, H, T, aux_encoder, decoder).total;
}

int l2hmc_bf16_planes(const float* W, int32_t ld, int64_t rows, int32_t K, uint16_t* planes, int64_t rows_pad, int32_t ld_planes,
                      void* stream) {
  if (!W || !planes || rows < 1 || K < 1 || ld < K || rows_pad < rows || ld_planes < K || (ld_planes & 3))
    return fail(L2HMC_ERR_ARG, "l2hmc_bf16_planes: bad argument%s");
  to_planes((hipStream_t)stream, W, ld, rows, K, planes, rows_pad, ld_planes);
  return L2HMC_OK;
}

int l2hmc_vae_energy(const L2hmcMlp3* decoder, const float* aux, const float* x, int64_t n_chains, int32_t d,
                     float* U_out, float* grad_out, float* workspace, float bce_scale, void* stream) {
  t_gemm_bf3 = 0;
  t_plane_mode = 0;
  int rc = check_mlp(decoder, "l2hmc_vae_energy");
  if (rc) return rc;
  if (!aux || !x || !workspace || n_chains < 0 || d != decoder->n_in) return fail(L2HMC_ERR_ARG, "l2hmc_vae_energy: bad argument%s");
  if (!(bce_scale >= 0.f && bce_scale <= 1.f)) return fail(L2HMC_ERR_ARG, "bce_scale must be in [0, 1] (0 = off)%s");
  const float beta = bce_scale > 0.f ? bce_scale : 1.f;
  if (n_chains == 0) return L2HMC_OK;
  hipStream_t s = (hipStream_t)stream;
  const SplitPlan p = plan_split(n_chains, d, 1, 1, nullptr, decoder);
  float* w = workspace;
  const Mlp3Ws ws = {w + p.dw1t, w + p.dw2t, w + p.dw3t, w + p.a1, w + p.s1, w + p.a2, w + p.s2};
  mlp3_transposes(s, *decoder, ws);
  rc = vae_energy(s, *decoder, aux, x, d, n_chains, d, ws, w + p.lg, w + p.rowsum, U_out, nullptr, grad_out, d, beta);
  if (rc) return rc;
  return launched();
}

int l2hmc_p_accept_energies(const float* U0, const float* v0, const float* U1, const float* v1, const float* log_jac,
                            int64_t n_chains, int32_t d, float* p_out, void* stream) {
  if (!U0 || !v0 || !U1 || !v1 || !log_jac || !p_out || n_chains < 0 || d < 1)
    return fail(L2HMC_ERR_ARG, "l2hmc_p_accept_energies: bad argument%s");
  if (n_chains == 0) return L2HMC_OK;
  hipLaunchKernelGGL(k_accept_from_energies, dim3(nblk(n_chains)), dim3(256), 0, (hipStream_t)stream, U0, v0, U1, v1,
                     log_jac, p_out, (long long)n_chains, d);
  return launched();
}

int l2hmc_trajectory_split(const L2hmcSplitArgs* a, void* stream) {
  if (!a) return fail(L2HMC_ERR_ARG, "args is NULL%s");
  if (a->gemm_mode < 0 || a->gemm_mode > 3) return fail(L2HMC_ERR_ARG, "gemm_mode must be 0 (f32 MFMA), 1 (bf16x3), 2 (bf16x3, split in the loop) or 3 (f16x2 planes)%s");
  t_gemm_bf3 = a->gemm_mode != 0;
  t_plane_mode = a->gemm_mode == 3;
  EngineCtx c = engine_target(*a, stream, a->hmc != 0, false);
  int rc;
  // (round 6: also with the decoder posterior -- the caller's nets then receive the images themselves, e.g. two nets with
  //  SEPARATE image branches, which the fused form does not have)
  if (c.unets && (a->xnet || a->vnet || a->aux_encoder || a->hmc))
    return fail(L2HMC_ERR_ARG, "net_cb excludes xnet / vnet / aux_encoder / hmc%s");
  if (c.user) {
    if (a->decoder || a->energy) return fail(L2HMC_ERR_ARG, "energy_cb excludes decoder and energy%s");
    if (a->bce_scale != 0.f) return fail(L2HMC_ERR_UNSUPPORTED, "bce_scale with a caller-supplied energy (anneal it in the callback)%s");
    if (a->aux_encoder && !a->aux) return fail(L2HMC_ERR_ARG, "aux_encoder needs aux%s");
  } else if (c.builtin) {
    if (a->decoder || a->aux_encoder || a->hmc)
      return fail(L2HMC_ERR_UNSUPPORTED, "a built-in energy excludes decoder / aux_encoder / hmc (HMC mode runs on l2hmc_trajectory)%s");
    if ((rc = check_energy(a->energy, a->d))) return rc;       // (a tempered target: l2hmc_energy divides U and grad U, dynamics.py:203-212)
  } else if ((rc = check_mlp(a->decoder, "decoder"))) {
    return rc;
  }
  if (a->aux_encoder && (rc = check_mlp(a->aux_encoder, "aux_encoder"))) return rc;
  if ((rc = check_dims(c))) return rc;
  const long long N = c.N;
  const int d = c.d, L = c.L;
  if (N == 0) return L2HMC_OK;
  if ((!c.hmc && ((!c.unets && (!a->xnet || !a->vnet)) || !a->masks || !a->trig)) || (c.vae && !a->aux) || !a->x || !a->v || !a->workspace)
    return fail(L2HMC_ERR_ARG, "l2hmc_trajectory_split: NULL pointer%s");
  if (!(a->bce_scale >= 0.f && a->bce_scale <= 1.f)) return fail(L2HMC_ERR_ARG, "bce_scale must be in [0, 1] (0 = off)%s");
  c.beta = a->bce_scale > 0.f ? a->bce_scale : 1.f;
  if ((rc = check_decoder_width(c)) || (rc = check_image_branch(c))) return rc;
  if (a->step_begin < 0 || a->n_steps < 0 || a->step_begin + a->n_steps > c.T) return fail(L2HMC_ERR_ARG, "steps outside the schedule%s");
  if (a->x_next && !a->u) return fail(L2HMC_ERR_ARG, "x_next needs u%s");
  if ((rc = check_eps(c))) return rc;
  const SplitPlan p = plan_split(N, d, c.H, c.T, a->aux_encoder, a->decoder);
  if ((rc = check_workspace(a->workspace_floats, p.total))) return rc;
  engine_bind(c, a->workspace, p, a->gemm_mode);
  // (what l2hmc_last_kernel reports for this engine: the kernel of the decoder-sized products, or the net evaluation)
  note_kernel(!c.vae ? "net_eval_kernel" : c.use_planes ? "gemm_xlp_kernel" : "gemm_nt_kernel");
  if (c.use_planes && (rc = planes_prepare())) return rc;
  hipStream_t s = c.s;
  float* w = c.w;
  // [x | grad U] and [v_h | masked x] live side by side (row stride L = 2 d): they are the first-layer inputs
  float *xc = w + p.abv, *g = xc + d, *vh = w + p.abx, *xin = vh + d, *vc = w + p.vc, *y = w + p.y;

  (void)hipMemcpy2DAsync(xc, sizeof(float) * L, a->x, sizeof(float) * d, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, s);
  (void)hipMemcpyAsync(vc, a->v, sizeof(float) * N * d, hipMemcpyDeviceToDevice, s);
  const bool have_w = (a->reuse & 1) != 0, have_auxh = (a->reuse & 2) != 0;    // still in the workspace (caller vouches)
  prepare_decoder(c, have_w);
  prepare_image_branch(c, have_w, have_auxh);
  prepare_nets(c, have_w, [](int) {});
  launch_kinetic(s, vc, w + p.K0, c.ld, N, d);
  double *U0d = reinterpret_cast<double*>(w + p.U0), *U1d = reinterpret_cast<double*>(w + p.U1);
  if ((rc = energy_at(c, xc, U0d))) return rc;
  if (a->n_steps == 0) (void)hipMemcpyAsync(U1d, U0d, sizeof(double) * N, hipMemcpyDeviceToDevice, s);
  if ((rc = plan_nets(c, false, 0))) return rc;

  for (int k = 0; k < a->n_steps; ++k) {
    const int it = a->step_begin + k;
    const bool last = k == a->n_steps - 1;
    if (c.hmc) {
      hipLaunchKernelGGL(k_hmc_drift, dim3(nblk(N * d)), dim3(256), 0, s, xc, L, vc, g, L, y, c.alpha, c.eps_host, c.dir, c.dall, N, d);
      if ((rc = energy_at(c, xc, last ? U1d : nullptr))) return rc;
      hipLaunchKernelGGL(k_hmc_kick, dim3(nblk(N * d)), dim3(256), 0, s, vc, y, g, L, c.alpha, c.eps_host, c.dir, c.dall, N, d);
      continue;
    }
    if ((rc = net_eval(c, 1, xc, it, v_update(L, vc, d, g, vh, L, xc, xin)))) return rc;          // v_h, and xin = k1 x for the next evaluation
    if ((rc = net_eval(c, 0, vh, it, x_update(L, xc, L, vh, y, d, xin, 0)))) return rc;           // y, xin = (1 - k1) y
    if ((rc = net_eval(c, 0, vh, it, x_update(L, y, d, vh, xc, L, nullptr, 1)))) return rc;       // x'
    if ((rc = energy_at(c, xc, last ? U1d : nullptr))) return rc;
    if ((rc = net_eval(c, 1, xc, it, v_update(L, vh, L, g, vc, d, nullptr, nullptr)))) return rc; // v'
  }
  launch_kinetic(s, vc, w + p.K1, (float*)nullptr, N, d);
  if (a->x_out) (void)hipMemcpy2DAsync(a->x_out, sizeof(float) * d, xc, sizeof(float) * L, sizeof(float) * d, (size_t)N, hipMemcpyDeviceToDevice, s);
  if (a->v_out) (void)hipMemcpyAsync(a->v_out, vc, sizeof(float) * N * d, hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(k_finish, dim3(nblk(N * d)), dim3(256), 0, s, U0d, w + p.K0, U1d, w + p.K1, c.ld, a->u, a->x,
                     xc, L, a->p_out, a->logjac_out, a->x_next, N, d);
  return launched();
}

}  // extern "C"

#include "train_split.hpp"
