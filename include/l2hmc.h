/*
 * l2hmc.h -- C ABI of libl2hmc_hip.so: the MI355X (gfx950) L2HMC leapfrog hot path.
 *
 * The reference (brain-research/l2hmc) has no native/FFI layer: its hot path is the
 * Python API of utils/dynamics.py + utils/sampler.py.  This header is the boundary a
 * drop-in replacement binds instead (ctypes from Python -- see INTEGRATION.md): every
 * entry point names the reference function(s) it replaces.  All paths below are relative
 * to the reference tree (/root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in `_host`;
 *     the caller (torch) owns all buffers; the library allocates nothing and keeps no
 *     pointer after a call returns;
 *   - all arrays are float32, row-major, C-contiguous; chains are rows: x is (N, d);
 *   - calls are asynchronous on `stream` (a hipStream_t; NULL = default stream), never
 *     synchronise, and may run concurrently on distinct streams/devices;
 *   - return value: 0 on success, a negative L2HMC_ERR_* code otherwise; the message is
 *     available from l2hmc_last_error() (thread-local).  Nothing throws or aborts.
 */
#ifndef L2HMC_H_
#define L2HMC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2HMC_ABI_VERSION 6

enum {
  L2HMC_OK = 0,
  L2HMC_ERR_ARG = -1,          /* null / inconsistent argument                       */
  L2HMC_ERR_UNSUPPORTED = -2,  /* shape outside what the fused kernels cover          */
  L2HMC_ERR_HIP = -3           /* HIP runtime error (launch, attribute, no device)    */
};

/* Target energies of utils/distributions.py that are fused into the kernels. */
enum {
  L2HMC_ENERGY_GAUSS_DIAG = 1,  /* Gaussian, diagonal precision   distributions.py:41-57,31-32 */
  L2HMC_ENERGY_GAUSS_DENSE = 2, /* Gaussian, dense precision      distributions.py:41-57,31-32 */
  L2HMC_ENERGY_GMM = 3,         /* mixture of Gaussians           distributions.py:104-134     */
  L2HMC_ENERGY_ROUGHWELL = 4,   /* rough well                     distributions.py:84-97       */
  L2HMC_ENERGY_FUNNEL = 5,      /* Gaussian funnel                distributions.py:155-180     */
  /* (6 is the Python binding's tag of the VAE decoder posterior, which runs on the GEMM engine) */
  L2HMC_ENERGY_LOGISTIC = 7,    /* Bayesian logistic regression   (l2hmc_pack_logistic)        */
  L2HMC_ENERGY_POISSON = 8,     /* Bayesian Poisson regression, log link and offsets (l2hmc_pack_logistic) */
  L2HMC_ENERGY_BINOMIAL = 9,    /* Bayesian binomial (trials) / negative-binomial (fixed dispersion) regression: logit link, per-row
                                   offsets and weights (l2hmc_pack_logistic, l2hmc_binomial_aux_floats) */
  L2HMC_ENERGY_PROBIT = 10      /* Bayesian binomial (trials) regression with the probit link: per-row offsets and trials in
                                   BINOMIAL's layout (l2hmc_pack_logistic, l2hmc_binomial_aux_floats) */
};

/* One S/T/Q network in the reference's own parameter layout: `Linear` keeps W as
 * (in, out) row-major and b as (out,) (utils/layers.py:29-37); `ScaleTanh` keeps a (1, d)
 * log-scale (utils/layers.py:81-86).  Architecture = SCGExperiment.ipynb `network`:
 *   h1 = relu(a W1 + b1 + b W2 + b2 + tau W3 + b3);  h2 = relu(h1 W4 + b4);
 *   S = exp(lam_s) * tanh(h2 Ws + bs);  T = h2 Wt + bt;  Q = exp(lam_q) * tanh(h2 Wq + bq)
 * Shapes: W1, W2 (d,H); W3 (2,H); W4 (H,H); Ws, Wt, Wq (H,d); b1,b2,b3,b4 (H); bs,bt,bq (d);
 * lam_s, lam_q (d). */
typedef struct L2hmcNet {
  const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
  const float *Ws, *bs, *Wt, *bt, *Wq, *bq, *lam_s, *lam_q;
} L2hmcNet;

/* Target energy U(x) (dynamics.py:203-212 `energy`, :217-218 `grad_energy`).
 *   GAUSS_DIAG : mu (d), prec (d) = diagonal of the fp32 precision matrix
 *   GAUSS_DENSE: mu (d), prec = buffer written by l2hmc_pack_gaussian (n_comp = 1)
 *   GMM        : mu (n_comp, d), prec = n_comp packed precisions back to back
 *                (stride l2hmc_packed_gaussian_floats(d)), logc (n_comp) = log(pi_i / sqrt((2 pi)^d det Sigma_i))
 *   ROUGHWELL  : eta, easy (distributions.py:84-97: U = |x|^2/2 + eta sum cos(x / eta^2), or x / eta if easy);
 *                den = the divisor of the cosine argument as the reference rounds it: the Python-DOUBLE product
 *                eps * eps (or eps if easy) converted to float32 ONCE (`x / (self.eps * self.eps)`, :93).  A binding
 *                that holds the caller's double passes float(eps * eps); 0 = derive from the float `eta`
 *                (identical whenever eps is exactly a float; last-bit different for e.g. eps = 0.1)
 *   FUNNEL     : eta = sigma (distributions.py:155-180; clip = 4 sigma)
 *   LOGISTIC   : Bayesian logistic regression on n data rows x_i (d features) with labels y_i in {0, 1} and a N(0, sigma^2 I)
 *                prior:  U(w) = sum_i [softplus(x_i . w) - y_i x_i . w] + |w|^2 / (2 sigma^2),
 *                        grad U = X^T (sigmoid(X w) - y) + w / sigma^2;
 *                n_comp = n (>= 1), mu = the buffer written by l2hmc_pack_logistic, eta = sigma^2 (> 0), prec = logc = NULL
 *                (ignored), easy = 0 (ignored).  d <= 128.  Runs on the general trajectory kernel (and its ladder, energy and
 *                p_accept forms) only -- `variant` 8, 16, 32 return L2HMC_ERR_UNSUPPORTED; the training entry points return
 *                L2HMC_ERR_UNSUPPORTED for it.  The packed data is staged in LDS when it fits, else streamed from L2
 *                (L2HMC_LOGISTIC_LDS=0 in the environment: always streamed)
 *   POISSON    : Bayesian Poisson regression with the log link on n data rows x_i (d features), counts y_i, per-row offsets o_i
 *                (log exposure) and a N(0, sigma^2 I) prior:  with h_i = x_i . w + o_i and mu_i = exp(h_i),
 *                        U(w) = sum_i [mu_i - y_i h_i] + |w|^2 / (2 sigma^2),   grad U = X^T (mu - y) + w / sigma^2;
 *                n_comp = n (>= 1), mu = the buffer written by l2hmc_pack_logistic with the counts in the label slot (the buffer the
 *                l2hmc_glm_* entries read), prec = the offsets: l2hmc_poisson_offset_floats(n) = 16 ceil(n / 16) floats, o_i then
 *                zeros (required: pass zeros for a model without offsets), eta = sigma^2 (> 0), logc = NULL (ignored), easy = 0
 *                (ignored).  d <= 128.  Runs where LOGISTIC runs, with the data and the offsets staged in LDS or streamed by the
 *                same rule; exp overflows as IEEE float32 does (mu = inf: U and grad U are non-finite, the accept rule rejects).
 *                Every training entry point returns L2HMC_ERR_UNSUPPORTED for it: train on the same likelihood as a
 *                caller-supplied energy (energy_cb), then sample with the trained nets on this kind
 *   BINOMIAL   : one energy for two regressions on n data rows x_i (d features) with a N(0, sigma^2 I) prior: with a per-row
 *                offset o_i and weight m_i, t_i = x_i . w + o_i,
 *                        U(w) = sum_i [m_i softplus(t_i) - y_i t_i] + |w|^2 / (2 sigma^2),   grad U = X^T (m sigmoid(t) - y) + w / sigma^2.
 *                Binomial regression with the logit link: y_i successes out of m_i trials, o_i the offset.  Negative-binomial
 *                regression (NB2: mean mu_i = exp(x_i . w + offset_i), variance mu + mu^2 / phi, phi fixed): m_i = y_i + phi,
 *                o_i = offset_i - log phi, so that sigmoid(t) = mu / (mu + phi).  The log-likelihood is -[m softplus(t) - y t]
 *                plus a constant of the row (log C(m, y); lgamma(y + phi) - lgamma(phi) - lgamma(y + 1)), which the energy drops.
 *                n_comp = n (>= 1), mu = the buffer written by l2hmc_pack_logistic with y in the label slot, prec = the row
 *                constants: l2hmc_binomial_aux_floats(n) = 32 ceil(n / 16) floats, per 16-row block [16 offsets | 16 weights],
 *                zero beyond n (required), eta = sigma^2 (> 0), logc = NULL (ignored), easy = 0 (ignored).  d <= 128.  Runs where
 *                POISSON runs, the data and the row constants staged in LDS or streamed by the same rule.  Nothing overflows:
 *                the residual is bounded by max(m, y) and softplus(t) = max(t, 0) + log(1 + exp(-|t|)).  Every training entry
 *                point returns L2HMC_ERR_UNSUPPORTED for it: train on the same likelihood as a caller-supplied energy
 *                (energy_cb), then sample with the trained nets on this kind
 *   PROBIT     : binomial regression with the probit link on n data rows x_i (d features) with a N(0, sigma^2 I) prior: y_i
 *                successes out of m_i trials (binary probit: m_i = 1), t_i = x_i . w + o_i, Phi the standard normal distribution
 *                function and lam(t) = phi(t) / Phi(t),
 *                        U(w) = -sum_i [y_i log Phi(t_i) + (m_i - y_i) log Phi(-t_i)] + |w|^2 / (2 sigma^2),
 *                        grad U = X^T ((m - y) lam(-t) - y lam(t)) + w / sigma^2
 *                (the row constant log C(m, y) is dropped).  The buffers are BINOMIAL's: n_comp = n (>= 1), mu = the buffer
 *                written by l2hmc_pack_logistic with y in the label slot, prec = l2hmc_binomial_aux_floats(n) floats, per 16-row
 *                block [16 offsets | 16 trials], zero beyond n (required), eta = sigma^2 (> 0), logc = NULL, easy = 0.  d <= 128.
 *                Runs where BINOMIAL runs.  log Phi and lam are formed from one float32 erfcx(|t| / sqrt 2) and are accurate to
 *                a few ulps in both tails (ProbitLink, csrc/l2hmc_kernels.hpp); nothing overflows for |t| up to about 1e19,
 *                beyond 2.6e19 t^2 / 2 is inf and U is non-finite, which the accept rule rejects.  Every training entry point
 *                returns L2HMC_ERR_UNSUPPORTED for it: train on the same likelihood as a caller-supplied energy (energy_cb),
 *                then sample with the trained nets on this kind
 * temperature divides U and grad U (dynamics.py:204-212); 1.0 when unused.
 * anneal_beta in (0, 1): the AIS bridge of utils/ais.py:46-47 with the standard-normal initial
 * energy its caller uses (eval_vae.py:55-56):  U := (1 - beta) |x|^2 / 2 + beta U(x);  0 (or 1) = off. */
typedef struct L2hmcEnergy {
  int32_t kind;
  int32_t n_comp;
  const float* mu;
  const float* prec;
  const float* logc;
  float eta;
  int32_t easy;
  float temperature;
  float anneal_beta;
  float den;               /* ROUGHWELL only (ABI 5); 0 = derive from eta */
  int32_t reserved_;       /* keeps the struct a multiple of 8 bytes; must be 0 */
} L2hmcEnergy;

/* Arguments of l2hmc_trajectory (passed by pointer; a HOST struct of device pointers). */
typedef struct L2hmcTrajectoryArgs {
  /* ---- model ------------------------------------------------------------------------- */
  const float* packed_nets; /* from l2hmc_pack_nets; NULL = HMC mode (nets == 0, dynamics.py:73-76) */
  L2hmcEnergy energy;
  const float* masks;       /* (T, d) 0/1 rows, `Dynamics.mask` (dynamics.py:84-97)          */
  const float* trig;        /* (T, 2) [cos(2 pi t/T), sin(2 pi t/T)] (dynamics.py:99-105)    */
  const float* alpha;       /* device scalar log(eps) (dynamics.py:50-58) or NULL ...        */
  float eps_host;           /* ... then this step size is used                               */
  /* ---- state -------------------------------------------------------------------------- */
  int64_t n_chains;
  int32_t d, H, T;
  int32_t step_begin;       /* leapfrog iterations [step_begin, step_begin + n_steps) of the  */
  int32_t n_steps;          /* T-step schedule; a full trajectory is (0, T)                   */
  const float* x;           /* (N, d) start positions                                         */
  const float* v;           /* (N, d) start momenta (the injected N(0,I) draw)                */
  const uint8_t* direction; /* (N) 1 = forward, 0 = backward (sampler.py:34) or NULL ...      */
  int32_t direction_all;    /* ... then every chain runs forward (1) or backward (0)          */
  const float* u;           /* (N) accept uniforms (sampler.py:54) or NULL (no MH step)       */
  /* ---- outputs (any may be NULL) ------------------------------------------------------- */
  float* x_out;             /* (N, d) proposal Lx                                             */
  float* v_out;             /* (N, d) proposal Lv                                             */
  float* logjac_out;        /* (N) summed log|det J| of the executed steps                    */
  float* p_out;             /* (N) accept prob, dynamics.py:302-309                           */
  float* x_next;            /* (N, d) MH-selected state, sampler.py:53-55 (needs u and p)     */
  /* ---- tuning ---------------------------------------------------------------------------- */
  int32_t variant;          /* kernel choice.  0 = automatic (measured rules): d <= 4 the
                             *   one-dimension-per-lane kernel; d <= 64 the instruction-lean tile kernel on 1 or 4
                             *   waves per 16-chain tile, from 16 384 chains with 33 <= d <= 64 and an elementwise
                             *   target one wave per tile; d > 128 the LDS-resident-state kernel (Gaussians incl. dense, mixtures, Rough Well); d <= 2 from 65 536
                             *   chains (d <= 4 from 131 072) ONE CHAIN PER LANE: the nets on packed VALU FMAs with
                             *   wave-uniform weights, no MFMA padding.  32 = force one chain per lane (d <= 4);
                             *   33 = the automatic choice among the MFMA kernels only.  1 / 4 = force
                             *   that many waves per tile; 16 = one wave per tile, 4 or 8 tiles per workgroup (every
                             *   contraction as f16x2; it parks the rejected chains' start point in x_next, so x_next must come
                             *   with u -- the automatic choice falls back to the 4-wave tile otherwise); 8 = the
                             *   LDS-resident-state kernel; 100 + v = geometry v on the general kernel (which also
                             *   serves HMC mode, AIS mode and tempered energies); 200 + v = choice v with the
                             *   f32-input MFMA forced: the tile kernels of the elementwise targets (diagonal Gaussian,
                             *   Rough Well: four-wave, one-wave and LDS-resident-state forms) and the d <= 4 kernel of
                             *   every target it serves otherwise run their contractions as f16x2 -- two f16 MFMAs on an
                             *   two-term split of both operands (22 significand bits worst case: fp32-level, measured equal
                             *   to the f32-input MFMA against float64) for |state|, |grad U| < 2.5e5 (activations < 4.2e6)
                             *   and |weight| < 1023; a proposal whose end points leave that range comes back as NaN
                             *   with accept probability 0 (csrc/traj_fast.hpp; L2HMC_F32_MFMA=1 in the environment =
                             *   200 + v for every call)                                                            */
  /* ---- persistent sampler loop (the notebook's per-MH-step sess.run loop, nb raw 288-298) -- */
  int32_t n_proposals;      /* M >= 1 proposals per launch (0 = 1).  With M > 1: v is (M,N,d),  */
                            /* direction (M,N), u (M,N) [required], p_out / logjac_out (M,N);   */
                            /* each proposal starts from the previous MH-selected state;        */
                            /* x_out / v_out hold the LAST proposal, x_next the final state     */
  float* x_hist;            /* (M, N, d) MH-selected state after every proposal, or NULL        */
  /* ---- in-kernel randomness (replaces tf.random_normal / random_uniform of dynamics.py:247-250, */
  /*      sampler.py:34,54): counter-based Philox4x32-10, keyed by (seed), counter = (global chain, */
  /*      dim/4, proposal index, stream) => independent of kernel geometry and of chain sharding.   */
  uint32_t rng_flags;       /* L2HMC_RNG_V | L2HMC_RNG_DIR | L2HMC_RNG_U: draw that input in-kernel  */
                            /* (the corresponding pointer v / direction / u is then ignored)          */
  uint64_t rng_seed;
  uint64_t rng_proposal0;   /* stream index of this launch's first proposal                          */
  int64_t chain_offset;     /* global index of row 0 (rank r owning rows [lo, hi) passes lo)          */
  /* ---- AIS mode of the persistent loop (utils/ais.py:43-66; HMC mode only: packed_nets = NULL) ------------- */
  /* ais_beta != NULL: proposal m is anneal step m.  Before its transition the log-weight takes                 */
  /*   w += ais_dbeta (|x|^2 / 2 - U(x))  (ais.py:58-59), the momentum is the step's draw z (ais_refreshment    */
  /*   < 0, ais.py:57) or  v sqrt(1 - r) + z sqrt(r)  (ais.py:55), the transition uses the bridge energy        */
  /*   (1 - beta) |x|^2 / 2 + beta U  with beta = ais_beta[m] (energy.anneal_beta is ignored), and after the MH */
  /*   step a rejected chain keeps x with the NEGATED proposed momentum (ais.py:62-65).  One launch replaces     */
  /*   the five per-step launches of l2hmc_ais_begin_step / l2hmc_energy / l2hmc_trajectory / l2hmc_ais_end_step.*/
  const float* ais_beta;    /* (M) bridge schedule, float32(linspace(0, 1, K + 1)[1:])                          */
  const float* ais_v0;      /* (N, d) momentum before step 0 (read only when refreshing), or NULL: the Philox    */
                            /*   draw of proposal index rng_proposal0 - 1                                        */
  float ais_dbeta;          /* beta[1] - beta[0]                                                                 */
  float ais_refreshment;    /* r in [0, 1], or < 0 for fresh momenta                                             */
  float* ais_w;             /* (N) log-weights, accumulated (+=)                                                 */
  float* ais_alpha;         /* (N) summed accept probabilities, accumulated (+=), or NULL                        */
} L2hmcTrajectoryArgs;

enum { L2HMC_RNG_V = 1, L2HMC_RNG_DIR = 2, L2HMC_RNG_U = 4 };

/* Parallel tempering (replica exchange over a temperature ladder) on the persistent sampler loop: l2hmc_trajectory_ladder.
 * Layout: N = n_ladders * K rows; row r belongs to ladder r / K and never moves.  Each row carries a rung label
 * rung_of_row[r] (initially r % K, unless the caller passes others); its temperature is temperatures[rung_of_row[r]].
 * Global round g = round0 + j (j = 0 .. n_rounds - 1) is proposals_per_round = M proposals -- each the proposal + MH step
 * of l2hmc_trajectory with U / T of the row's current rung in the leapfrog, the nets' grad U input and the accept
 * probability -- then one deterministic even-odd swap sweep: for every k = g mod 2, g mod 2 + 2, ... with k + 1 < K, in
 * every ladder, the rows a (rung k) and b (rung k + 1) exchange labels iff
 *     log u < (1 / T_k - 1 / T_{k+1}) (U_a - U_b),
 * U the untempered energy of each row's current state; a NaN on either side rejects.  u is injected (swap_u) or drawn from
 * the Philox stream keyed by (rng_seed, global ladder index, g) -- stream 2 of csrc/l2hmc_kernels.hpp (philox_swap_u):
 * counter (chain_offset / K + ladder, 0xFFFFFFFF, g mod 2^32, (g >> 32) << 4 | (k >> 1) << 1 | 1), u = (word 0 >> 8) 2^-24.
 * Proposal draws are keyed as in l2hmc_trajectory (global chain, proposal index rng_proposal0 + j M + m), so splitting the
 * ladders over launches or ranks (chain_offset a multiple of K) gives the same bits.
 * Round trips: a row that has reached rung K - 1 since it last left rung 0 completes one when it is back at rung 0
 * (evaluated on the labels after every sweep; trip_state[r] = 1 while the row is on its way down). */
typedef struct L2hmcLadderArgs {
  int32_t n_rungs;              /* K: 2, 4, 8 or 16                                                                      */
  int32_t n_rounds;             /* R >= 1                                                                                */
  int32_t proposals_per_round;  /* M >= 1; the launch runs R * M proposals (L2hmcTrajectoryArgs.n_proposals is ignored:  */
                                /* injected v / direction / u are (R M, N, ...), p_out / logjac_out (R M, N))            */
  int32_t reserved_;            /* must be 0                                                                             */
  float temperatures[16];       /* T_0 .. T_{K-1}: positive, finite, non-decreasing (equal rungs allowed); rest ignored  */
  uint64_t round0;              /* global index of this launch's first round                                             */
  int8_t* rung_of_row;          /* (N) labels, read and updated in place                                                 */
  int8_t* trip_state;           /* (N) round-trip states, read and updated in place, or NULL (all 0, not kept)           */
  const float* swap_u;          /* (R, n_ladders, K / 2) uniforms of the pairs (k, k + 1) at index k / 2, or NULL        */
  float* cold_hist;             /* (R M, n_ladders, d) the rung-0 state of every ladder after every proposal (after the  */
                                /* round's sweep at its last proposal), or NULL                                          */
  int8_t* rung_hist;            /* (R, N) the labels after every sweep, or NULL                                          */
  int64_t* swaps_accepted;      /* (K - 1) accepted swaps of the pair (k, k + 1), accumulated (+=), or NULL              */
  int64_t* swaps_attempted;     /* (K - 1) attempted swaps, accumulated (+=), or NULL                                    */
  int64_t* round_trips;         /* (n_ladders) completed round trips, accumulated (+=), or NULL                          */
} L2hmcLadderArgs;

int l2hmc_abi_version(void);
const char* l2hmc_last_error(void);
/* Name of the kernel the last l2hmc_trajectory / l2hmc_train_propose_grad / l2hmc_train_step call of THIS thread chose
 * (e.g. "traj_fast_kernel<1, 1, 4, 3>", spelt as rocprofv3 prints the instantiation; "" before the first call): what a
 * profile of the call has to be matched against.  l2hmc_trajectory_split reports the template of its dominant kernel
 * without arguments: "gemm_xlp_kernel" (decoder products on pre-split bf16 planes, from 3072 chains at config 5's widths
 * in gemm_mode 1), "gemm_nt_kernel", or "net_eval_kernel" for a built-in / caller-supplied energy.  Copies at most n - 1 characters, returns the full length. */
int32_t l2hmc_last_kernel(char* buf, int32_t n);
/* The same call's __global__ function.  It differs from l2hmc_last_kernel where a kernel has a second body that computes the same
 * bits: "traj_fast_cc_kernel<1, 1, 4, 3, 1, 1>" (one workgroup per CU; PK last, the bound in front of it) for a common sampler
 * launch of "traj_fast_kernel<1, 1, 4, 3, 1>" whose grid has at most one workgroup per CU (L2HMC_FAST_ONE_WAVE=0 / 1 in the
 * environment forces the choice for such a launch). */
int32_t l2hmc_last_kernel_body(char* buf, int32_t n);
/* The LDS plan of the diagonal Gaussian's one-tile four-wave f16x2 sampler kernel (d <= 64, a schedule of T steps), from the
 * planner's own function; no GPU needed.  one_wave = 0: "traj_fast_kernel<1, 1, 4, ., 1>", 1: its one-workgroup-per-CU body.
 * what = 0: the dynamic LDS in bytes, 1: the K-split exchange buffers (4 KB each), 2: the bytes of the schedule records.
 * L2HMC_ERR_ARG on bad arguments. */
int64_t l2hmc_sampler_lds_plan(int32_t d, int32_t T, int32_t one_wave, int32_t what);

/* Number of floats of the fragment-ordered weight buffer for both nets, or a negative
 * L2HMC_ERR_* if (d, H) is outside the fused kernels' range. */
int64_t l2hmc_packed_nets_floats(int32_t d, int32_t H);

/* Re-orders XNet and VNet (utils/layers.py parameter layout, built by the `net_factory`
 * of dynamics.py:78-79) into MFMA A-operand fragment order.  Run once per weight update. */
int l2hmc_pack_nets(const L2hmcNet* xnet, const L2hmcNet* vnet, int32_t d, int32_t H,
                    float* packed, void* stream);

int64_t l2hmc_packed_gaussian_floats(int32_t d);
/* i_sigma: (d, d) fp32 precision matrix `Gaussian.i_sigma.astype('float32')`
 * (distributions.py:48,52); packs (S + S^T)/2 in fragment order. */
int l2hmc_pack_gaussian(const float* i_sigma, int32_t d, float* packed, void* stream);

/* Bayesian logistic regression data (L2HMC_ENERGY_LOGISTIC) in the order the kernels read it: X (n_data, d) row-major and
 * y (n_data) in {0, 1}, both device float32, padded to 16-row blocks.  Per block the rows as the A operand of the logits
 * X w (contraction over the d features), the same rows as the A operand of the gradient X^T r (contraction over the rows),
 * then the block's 16 labels; rows beyond n_data are zero and the kernels mask them by n_comp = n_data (they would
 * otherwise add softplus(0) = log 2 each).  Run once per data set.  L2HMC_ERR_ARG: n_data < 1 or > 1048576, d outside
 * 1 ... 128, a NULL buffer. */
int64_t l2hmc_packed_logistic_floats(int32_t n_data, int32_t d);
int l2hmc_pack_logistic(const float* X, const float* y, int32_t n_data, int32_t d, float* packed, void* stream);
/* Floats of the offset buffer of L2HMC_ENERGY_POISSON (L2hmcEnergy.prec): 16 ceil(n_data / 16), the tail zero-padded. */
int64_t l2hmc_poisson_offset_floats(int32_t n_data);
/* Floats of the row-constant buffer of L2HMC_ENERGY_BINOMIAL and L2HMC_ENERGY_PROBIT (L2hmcEnergy.prec): 32 ceil(n_data / 16) -- per 16-row data block
 * [16 offsets | 16 weights], rows beyond n_data zero.  L2HMC_ERR_ARG for n_data outside 1 ... 1048576. */
int64_t l2hmc_binomial_aux_floats(int32_t n_data);

/* The fused generalised-leapfrog trajectory:
 *   Dynamics.forward / .backward           dynamics.py:246-300  (n_steps = T)
 *   Dynamics._forward_step/_backward_step  dynamics.py:115-201  (n_steps = 1; a backward
 *       step at schedule index s is step_begin = T-1-s with direction 0)
 *   Dynamics.p_accept                      dynamics.py:302-309  (p_out)
 *   propose + tf_accept                    sampler.py:28-55     (direction, u, x_next)
 * Each chain runs only in its drawn direction (the reference runs both and discards one). */
int l2hmc_trajectory(const L2hmcTrajectoryArgs* args, void* stream);

/* l2hmc_trajectory on a temperature ladder (parallel tempering, L2hmcLadderArgs above): the general trajectory kernel
 * (variant 0 or 100 + v picks its geometry as for l2hmc_trajectory's 100 + v) with HMC or fused S/T/Q nets (H <= 15) and
 * every built-in energy.  Needs u (or L2HMC_RNG_U).  L2HMC_ERR_ARG: K not in {2, 4, 8, 16}, N or chain_offset not a
 * multiple of K, a bad ladder, energy.temperature != 1 (the ladder replaces it); L2HMC_ERR_UNSUPPORTED: AIS fields set,
 * energy.anneal_beta != 0, any other variant. */
int l2hmc_trajectory_ladder(const L2hmcTrajectoryArgs* args, const L2hmcLadderArgs* ladder, void* stream);

/* ONE generalised leapfrog step straight from the reference-layout weights -- the per-step entry point
 * SURVEY.md 8(b) names: Dynamics._forward_step (dynamics.py:115-157; dir = 1) / ._backward_step (:159-201;
 * dir = 0) at the schedule row whose mask (dynamics.py:95-97) and time encoding (:99-105) are passed in.
 * xnet = vnet = NULL is HMC mode (dynamics.py:73-76).  logjac_inout (N) is ACCUMULATED (+=) or NULL.
 * `workspace`: l2hmc_workspace_bytes(n_chains, d, H) bytes of device memory (packed fragments, the schedule
 * row, a log-det temporary); the library allocates nothing.  Callers that take many steps should pack once
 * (l2hmc_pack_nets) and use l2hmc_trajectory, which fuses the whole trajectory. */
int64_t l2hmc_workspace_bytes(int64_t n_chains, int32_t d, int32_t H);
int l2hmc_step(const L2hmcNet* xnet, const L2hmcNet* vnet, const L2hmcEnergy* energy, const float* x, const float* v,
               float* x_out, float* v_out, float* logjac_inout, const float* mask_row, float cos_t, float sin_t,
               float eps, const uint8_t* dir_or_null, int32_t dir_all, int64_t n_chains, int32_t d, int32_t H,
               void* workspace, void* stream);

/* Dynamics.energy / Dynamics.grad_energy (dynamics.py:203-218).  U_out (N) and/or
 * grad_out (N, d) may be NULL. */
int l2hmc_energy(const L2hmcEnergy* energy, const float* x, int64_t n_chains, int32_t d,
                 float* U_out, float* grad_out, void* stream);

/* Dynamics.p_accept (dynamics.py:302-309) on arbitrary end points. */
int l2hmc_p_accept(const L2hmcEnergy* energy, const float* x0, const float* v0,
                   const float* x1, const float* v1, const float* logjac,
                   int64_t n_chains, int32_t d, float* p_out, void* stream);

/* tf_accept (sampler.py:53-55): x_next[n,:] = (px[n] - u[n] >= 0) ? Lx[n,:] : x[n,:]. */
int l2hmc_mh_select(const float* x, const float* Lx, const float* px, const float* u,
                    int64_t n_chains, int32_t d, float* x_next, void* stream);

/* The notebook loss from the per-chain arguments v1 the training entry points leave behind (SCGExperiment.ipynb raw 156-169:
 * loss = scale * mean(1 / v1) - mean(v1) / scale over x- and z-proposals): out3 = { sum 1 / v1, sum v1,
 * inv_n * (scale * out3[0] - out3[1] / scale) } in double, one fixed-order reduction (bitwise reproducible) -- ONE launch
 * instead of a dozen elementwise framework kernels per optimiser step.  Sharded runs all-reduce out3[0..1] themselves. */
int l2hmc_loss_terms(const float* v1, int64_t n, float scale, double inv_n, double* out3, void* stream);

/* ---- split engine: wide / image-conditioned nets + VAE latent-posterior energy (config 5) ------ */
/* Linear-softplus-Linear-softplus-Linear with reference-layout weights W (in, out), b (out):
 * the VAE decoder (mnist_vae.py:104-111) and the sampler's image branch `encoder_sampler`
 * (mnist_vae.py:134-140). */
typedef struct L2hmcMlp3 {
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  int32_t n_in, n_h1, n_h2, n_out;
} L2hmcMlp3;

/* l2hmc_trajectory_split: same contract as l2hmc_trajectory (steps [step_begin, +n_steps) of the
 * T-step schedule, per-chain direction, accept probability, MH select) for
 *   energy  U(z; aux) = sum_pix BCE_with_logits(aux, decoder(z)) + |z|^2 / 2   (mnist_vae.py:122-126)
 *   nets    the S/T/Q architecture with ANY hidden width H and, if aux_encoder != NULL, the 4th Zip
 *           branch aux_encoder(aux) added into the first hidden layer (mnist_vae.py:142-167);
 *           RAW reference-layout weights (not the packed buffer).
 * The dense products run in this library's own fp32 MFMA GEMM (csrc/gemm_f32.hpp) with the bias / softplus /
 * sigmoid / relu / BCE-gradient / chain-rule work fused into its epilogues; no BLAS library is used. */
/* A caller-supplied target energy: the `energy_function` protocol of utils/dynamics.py:203-218 (`self._fn(x[, aux])`
 * and tf.gradients of it) for energies OUTSIDE the fused set -- e.g. a closure like mnist_vae.py:122-126 or any density
 * the caller can differentiate.  The library calls it on the HOST, between kernel launches, whenever the trajectory
 * needs grad U (once per leapfrog step + once at the start) and U (at the two end points):
 *   x        (n_chains, d) current positions, row stride ldx floats (device memory inside the workspace)
 *   U_out    NULL, or (n_chains) DOUBLES to fill with U(x) (|U| can be ~1e3: the accept probability takes a
 *            difference of two of them)
 *   grad_out (n_chains, d) floats, row stride ldg, to fill with grad U(x)
 * All work must be enqueued on `stream` (no synchronisation needed); return 0, or non-zero to abort the trajectory
 * (l2hmc_trajectory_split then returns L2HMC_ERR_ARG).  Tempering / annealing of a user energy is the callback's own
 * business.  This is the SLOW path by construction (a host round trip per gradient); the leapfrog half-updates and the
 * S/T/Q nets stay on the library's kernels. */
typedef int (*L2hmcEnergyCallback)(void* user, const float* x, int64_t ldx, int64_t n_chains, int32_t d,
                                   double* U_out, float* grad_out, int64_t ldg, void* stream);

/* Hessian-vector product of a caller-supplied energy, for TRAINING on it (l2hmc_train_split_grad): the loss
 * back-propagates through grad U (utils/dynamics.py:218 inside the differentiated graph), so the reverse sweep needs
 *   hv_out (n_chains, d; row stride ldhv) = (d^2 U / dx^2)(x) u      for x (row stride ldx) and u (row stride ldu)
 * once per leapfrog step -- e.g. torch.autograd.grad of sum(grad U * u) in a binding.  Same rules as
 * L2hmcEnergyCallback (enqueue on `stream`, return 0 or non-zero to abort). */
typedef int (*L2hmcHvpCallback)(void* user, const float* x, int64_t ldx, const float* u, int64_t ldu, int64_t n_chains,
                                int32_t d, float* hv_out, int64_t ldhv, void* stream);

/* A caller-supplied S/T/Q net (the reference's `net_factory` may return ANY callable [a, b, tau, aux] -> [S, T, Q],
 * utils/dynamics.py:69-79; only the notebook's architecture is fused into kernels).  Called on the host between launches, like
 * the energy callback: `ab` is the (n_chains, 2 d) block [a | b] of first-layer inputs on the device (row stride ldab floats):
 * a = ab[:, :d], b = ab[:, d:]; net = 0 (XNet: a = v_h, b = kept * x) or 1 (VNet: a = x, b = grad U); chain n sits at schedule
 * row `it` if it runs forward (direction[n] != 0, or direction == NULL and direction_all != 0), else T - 1 - it: its time input
 * is tau = (cos, sin)(2 pi row / T) (dynamics.py:99-105).  The callback enqueues, on `stream`, the FINAL S, T, Q (dynamics.py's
 * `scale, translation, transformed`) as the three (n_chains, d) column blocks of stq_out (row stride 3 d).  Nonzero return
 * aborts the trajectory.  Training such nets: L2hmcNetVjpCallback below (ABI 6). */
typedef int (*L2hmcNetCallback)(void* user, int32_t net, const float* ab, int64_t ldab, int64_t n_chains, int32_t d, int32_t it,
                                const uint8_t* direction, int32_t direction_all, float* stq_out, void* stream);
/* (ABI 6) The reverse of ONE evaluation of a caller-supplied net, for l2hmc_train_split_grad: the reference minimises its loss
 * over whatever variables `net_factory` created (utils/dynamics.py:78-79; SCGExperiment.ipynb raw 178-181 `minimize(loss)`;
 * mnist_vae.py:254-262), so the adjoint of an opaque net is the caller's to form.  `ab`, `it`, `direction` identify the
 * evaluation exactly as in L2hmcNetCallback (the library hands back the SAME inputs it kept from the forward pass);
 * d_stq (n_chains, 3 d, row stride 3 d) holds the cotangents of the net's outputs (d S | d T | d Q) -- already weighted by
 * inv_n and the loss.  The callback enqueues on `stream`: (i) the cotangents of the inputs, (d a | d b), into d_ab
 * (n_chains, 2 d, row stride ld_dab); (ii) the accumulation of its OWN parameters' gradients wherever it keeps them (with
 * torch: one `torch.autograd.backward` of the re-evaluated net) -- the library never sees those parameters.  Nonzero return
 * aborts the call. */
typedef int (*L2hmcNetVjpCallback)(void* user, int32_t net, const float* ab, int64_t ldab, int64_t n_chains, int32_t d, int32_t it,
                                   const uint8_t* direction, int32_t direction_all, const float* d_stq, float* d_ab,
                                   int64_t ld_dab, void* stream);

typedef struct L2hmcSplitArgs {
  const L2hmcNet* xnet;
  const L2hmcNet* vnet;
  int32_t H;
  const L2hmcMlp3* aux_encoder;  /* (n_pix -> H) or NULL                                    */
  const L2hmcMlp3* decoder;      /* (d -> n_pix)                                            */
  const float* aux;              /* (N, n_pix) conditioning images                          */
  const float* masks;            /* (T, d) */
  const float* trig;             /* (T, 2) */
  const float* alpha;
  float eps_host;
  int64_t n_chains;
  int32_t d, T, step_begin, n_steps;
  const float* x;
  const float* v;
  const uint8_t* direction;
  int32_t direction_all;
  const float* u;
  float *x_out, *v_out, *logjac_out, *p_out, *x_next;
  float* workspace;              /* l2hmc_split_workspace_floats(...) floats                */
  int64_t workspace_floats;
  int32_t hmc;                   /* 1: nets identically zero (dynamics.py:73-76) = plain leapfrog, forward
                                  *    only; xnet / vnet / masks / trig / aux_encoder are ignored         */
  float bce_scale;               /* AIS bridge from N(0, I) (ais.py:46-47, eval_vae.py:55-62): the BCE term
                                  *    of the energy is scaled by beta in (0, 1); 0 (or 1) = off          */
  const L2hmcEnergy* energy;     /* NULL: the decoder posterior above.  Else one of the built-in targets of
                                  *    utils/distributions.py (decoder / aux / aux_encoder = NULL): the S/T/Q
                                  *    nets of ANY width H on the GEMM engine, grad U from l2hmc_energy's kernels
                                  *    (SCGExperiment.ipynb `network` with H != 10)                       */
  int32_t reuse;                 /* what the SAME workspace still holds from the previous call with the same shapes
                                  *    (the library keeps no state of its own; the caller vouches):
                                  *    1: the prepared weights (transposed copies, time table) -- no weight changed;
                                  *    2: the image branch aux_encoder(aux) -- aux and aux_encoder unchanged.
                                  *    A sampling loop passes 3 from its second proposal on (mnist_vae.py:185-224:
                                  *    weights and images are fixed while the chain runs)                  */
  L2hmcEnergyCallback energy_cb; /* non-NULL: the caller's energy (see L2hmcEnergyCallback); decoder = energy = NULL.
                                  *    aux_encoder + aux may still be given (image-conditioned nets,
                                  *    mnist_vae.py:134-150: aux is (N, aux_encoder->n_in)); HMC mode is allowed  */
  void* energy_cb_user;          /* passed back as the callback's first argument                              */
  int32_t gemm_mode;             /* arithmetic of the decoder-sized dense products (M x 1024 x 1024 ...):
                                  *    0: f32-input MFMA (v_mfma_f32_16x16x4_f32), bit-exact fp32 FMA chains;
                                  *    1: "bf16x3" -- every fp32 operand split EXACTLY into three bf16 terms, the six
                                  *       significant cross products on the bf16 MFMA (16x the f32 MFMA rate), fp32
                                  *       accumulation: dropped terms <= 3 x 2^-24 |x y| per product, i.e. fp32-level
                                  *       accuracy (measured against float64 in profiles/ and the config-5 parity tests);
                                  *       from 3072 chains at config 5's widths on operands PRE-SPLIT into bf16 planes
                                  *    2: the same six products with the split inside the k loop at every size -- bit-identical
                                  *       results to mode 1 (the planes only move where the split happens); kept for tests and A/B
                                  *    3: "f16x2 planes" (round 6; what l2hmc_amd.Dynamics asks for): x = X1 + X2 / 64 with X1 =
                                  *       f16(x), X2 = f16(64 (x - X1)), stored as the three f16 planes X1 | X1 / 64 | X2, so that
                                  *       x y = X1 Y1 + (X1 / 64) Y2 + X2 (Y1 / 64) is THREE f16 MFMAs on one accumulator: half of
                                  *       mode 1's matrix-pipe work at fp32-level accuracy (22 significand bits per operand in the worst case)
                                  *       for operand entries in [4e-3, 65504) -- smaller entries keep an absolute error of
                                  *       2^-30, larger ones overflow to inf.  The sampler's activations, logits and BCE
                                  *       gradients live there; the TRAINER's tangent / adjoint planes (entries scaled by 1 / chains)
                                  *       do not: under L2hmcTrainSplitArgs.gemm_mode 3 its forward evaluations run on f16x2
                                  *       planes, its reverse sweep as mode 1 (csrc/gemm_f32.hpp, gemm_xl.hpp, train_split.hpp)   */
  L2hmcNetCallback net_cb;       /* (ABI 5) non-NULL: the caller's nets (see L2hmcNetCallback); xnet = vnet = aux_encoder = NULL,
                                  *    H is ignored, hmc = 0.  With any target: energy_cb, a built-in energy, or (round 6) the
                                  *    decoder posterior -- the callback's nets then read the images on their own           */
  void* net_cb_user;             /* passed back as the callback's first argument                                         */
} L2hmcSplitArgs;

int64_t l2hmc_split_workspace_floats(int64_t n_chains, int32_t d, int32_t H, int32_t T,
                                     const L2hmcMlp3* aux_encoder, const L2hmcMlp3* decoder);
int l2hmc_trajectory_split(const L2hmcSplitArgs* args, void* stream);
/* Dynamics.energy / grad_energy for the VAE posterior; workspace as for the split trajectory;
 * bce_scale as in L2hmcSplitArgs (0 = off). */
int l2hmc_vae_energy(const L2hmcMlp3* decoder, const float* aux, const float* x, int64_t n_chains,
                     int32_t d, float* U_out, float* grad_out, float* workspace, float bce_scale, void* stream);

/* The operand form of gemm_mode 1 at decoder sizes, exposed for inspection and tests: the exact three-way bf16 split
 * x = h + m + l (round-to-nearest-even at each level) of the fp32 matrix W (rows x K, row stride ld) as three planes of
 * rows_pad x ld_planes bf16 bit patterns (uint16), plane p at planes + p * rows_pad * ld_planes, zero beyond the matrix
 * (rows_pad >= rows; ld_planes >= K, a multiple of 4).  This is what l2hmc_trajectory_split converts the decoder weights
 * to once per call (csrc/gemm_xl.hpp); oracle/bf16x3_oracle.py restates it in numpy. */
int l2hmc_bf16_planes(const float* W, int32_t ld, int64_t rows, int32_t K, uint16_t* planes, int64_t rows_pad,
                      int32_t ld_planes, void* stream);

/* Dynamics.p_accept (dynamics.py:302-309) for energies evaluated separately (l2hmc_vae_energy):
 * p = exp(min(U0 + |v0|^2/2 - U1 - |v1|^2/2 + log_jac, 0)), non-finite -> 0. */
int l2hmc_p_accept_energies(const float* U0, const float* v0, const float* U1, const float* v1, const float* log_jac,
                            int64_t n_chains, int32_t d, float* p_out, void* stream);

/* ---- training (next-row f1): one proposal + the gradient of its loss term ------------------- */
/* Loss of SCGExperiment.ipynb raw lines 156-169 for ONE of its two proposals:
 *   v1_n = |x_n - Lx_n|^2 p_n + 1e-4;   term = scale * mean_n(1 / v1_n) - mean_n(v1_n) / scale
 * (the notebook adds the term of `propose(x)` and of `propose(z), z ~ N(0, I)`; call twice).
 * `grad` (l2hmc_train_grad_floats(d, H) floats) is ACCUMULATED (+=) without atomics -- every workgroup
 * writes its partial gradient to the workspace and a second tiny kernel adds them in block order, so the
 * result is bitwise reproducible --: the flat layout is
 * [XNet | VNet | d/d eps], each net in the field order of L2hmcNet (W1, b1, ..., lam_q);
 * d/d alpha = eps * d/d eps (dynamics.py:50-58).  inv_n = 1 / (chains over ALL ranks) so that
 * per-rank gradients simply all-reduce(sum).  The nets are the RAW reference-layout weights
 * (not the packed buffer); for the dense Gaussian `energy.prec` is the raw (d, d) precision.
 * Targets with analytic Hessian-vector products: Gaussian (diag / dense), GMM (prec = RAW (k,d,d)
 * precisions, logc, n_comp <= 8), Rough Well, logistic regression (see l2hmc_train_logistic_lds_bytes below);
 * any d, H whose 16-chain tile fits the 160 KiB LDS
 * (d = 50, H = 10 uses 122 KiB; larger shapes return L2HMC_ERR_UNSUPPORTED).  Every chain runs in
 * its own direction.
 * energy.temperature is honoured: the dynamics, the accept probability and the gradient are those of
 * U / temperature (a finite temperature > 0; else L2HMC_ERR_ARG).  energy.anneal_beta is not: training on the
 * AIS bridge returns L2HMC_ERR_UNSUPPORTED. */
typedef struct L2hmcTrainArgs {
  const L2hmcNet* xnet;
  const L2hmcNet* vnet;
  L2hmcEnergy energy;
  const float* masks;       /* (T, d)   */
  const float* trig;        /* (T, 2)   */
  const float* alpha;       /* device log(eps) or NULL -> eps_host */
  float eps_host;
  int64_t n_chains;
  int32_t d, H, T;
  const float* x;           /* (N, d) start points                                   */
  const float* v;           /* (N, d) momenta of each chain's own direction          */
  const uint8_t* direction; /* (N) or NULL -> direction_all                          */
  int32_t direction_all;
  float scale;              /* 0.1 in the notebook                                   */
  float inv_n;
  float* Lx;                /* (N, d) proposal                                       */
  float* p;                 /* (N) accept probability                                */
  float* v1;                /* (N) per-chain loss argument                           */
  float* grad;              /* flat gradient, accumulated                            */
  float* workspace;         /* l2hmc_train_workspace_floats(N, d, H, T) floats       */
  int32_t variant;          /* 0 = auto: d <= 4 (Gaussians, GMM, Rough Well) the one-dimension-per-lane kernel; else the
                             *   register-resident kernel (elementwise targets d <= 64, dense Gaussians d <= 16,
                             *   H <= 15); else the general LDS-matrix tile kernel.  1 = as 0 without the d <= 4
                             *   form; 100 = always the general kernel                                      */
} L2hmcTrainArgs;

int64_t l2hmc_train_workspace_floats(int64_t n_chains, int32_t d, int32_t H, int32_t T);
int64_t l2hmc_train_grad_floats(int32_t d, int32_t H);
/* LDS bytes of the fused training kernel l2hmc_train_propose_grad would launch for this shape (> 0), or
 * L2HMC_ERR_UNSUPPORTED when no fused kernel holds it (d / H beyond the 16-chain tile's 160 KiB plan, the funnel beyond
 * d = 16): the host then trains on the GEMM engine (l2hmc_train_split_grad below), which takes any d and H. */
int64_t l2hmc_train_fused_lds_bytes(int32_t energy_kind, int32_t n_comp, int32_t d, int32_t H, int32_t T);
/* Logistic regression (L2HMC_ENERGY_LOGISTIC) trains on a form of the general tile kernel of its own (l2hmc_last_kernel:
 * "train_kernel<7>"): energy.mu = the packed data (l2hmc_pack_logistic), 1 <= energy.n_comp = n_data <= 2^20, energy.eta =
 * sigma^2 > 0 and finite, d <= 128 -- the trajectory entry's rules.  grad U, U and the Hessian-vector product
 * H(w) u = X^T [s (1 - s) (X u)] + u / sigma^2 are f32 MFMA contractions over the data streamed from L2, split over the four
 * waves and summed in wave order (no atomics).  This query gives the dynamic LDS bytes of that kernel (> 0),
 * L2HMC_ERR_UNSUPPORTED with the bytes quoted in l2hmc_last_error when the 16-chain tile does not fit 160 KiB (d = 50, H = 10,
 * T = 10 does), L2HMC_ERR_ARG on bad arguments.  (l2hmc_train_fused_lds_bytes keeps refusing kind 7.) */
int64_t l2hmc_train_logistic_lds_bytes(int32_t n_data, int32_t d, int32_t H, int32_t T);
int l2hmc_train_propose_grad(const L2hmcTrainArgs* args, void* stream);

/* One optimiser step's device work in as few launches as the data flow allows (ABI 4; SCGExperiment.ipynb raw 156-181,
 * 254-271: propose(x) and propose(z), the loss of both, Adam, the MH-selected continuation of the x chains):
 *   launch 1  l2hmc_train_propose_grad's kernel over `args` -- with the start points of chains [0, n_head) read from
 *             `x_head` (no staging copy of the caller's state next to z);
 *   launch 2  the fixed-order slot reduction, which OVERWRITES args->grad (no zero fill), with
 *             - the Metropolis select of chains [0, n_head) (sampler.py:53-55) in extra workgroups of the same launch
 *               when u / x_next are given;
 *             - the loss terms of args->v1 (as l2hmc_loss_terms) -> `loss` and, split into float (hi, lo) pairs,
 *               -> `terms` = {sum 1/v1, sum v1, n_head}: the tail of the ONE buffer a sharded step all-reduces;
 *             - Adam on theta / m / v (as l2hmc_adam_step) in the same launch when `theta` is given (a single-process
 *               step; a sharded one all-reduces first and calls l2hmc_adam_step_terms).
 * `terms` may point right behind the gradient (args->grad + l2hmc_train_grad_floats). */
typedef struct L2hmcTrainStep {
  const float* x_head;      /* (n_head, d) or NULL: start points of chains [0, n_head); the others stay in args->x  */
  int64_t n_head;
  const float* u;           /* (n_head) uniforms and ...                                                           */
  float* x_next;            /* ... (n_head, d) selected states; both or neither                                     */
  float* terms;             /* 6 floats or NULL                                                                     */
  double* loss;             /* 3 doubles {sum 1/v1, sum v1, inv_n (scale sum 1/v1 - sum v1 / scale)} or NULL; inv_n =
                             * 1 / k in double when args.inv_n is the float rounding of 1 / k (= l2hmc_loss_terms)   */
  float* theta;             /* flat parameters [XNet | VNet | alpha] or NULL (no optimiser in this call)            */
  float* m;
  float* v;
  float lr, beta1, beta2, epsilon;
  int64_t step;             /* Adam's t (>= 1)                                                                      */
  int32_t train_alpha;      /* 1: the last gradient entry is d/d eps, the parameter is log eps                      */
} L2hmcTrainStep;
int l2hmc_train_step(const L2hmcTrainArgs* args, const L2hmcTrainStep* step, void* stream);
/* Adam after a sharded step's all-reduce: grad = the reduced gradient, terms6 = the reduced tail written by
 * l2hmc_train_step; the loss of the GLOBAL batch, (scale sum 1/v1 - sum v1 / scale) / count, lands in loss_out[2]
 * ([0], [1]: the two sums). */
int l2hmc_adam_step_terms(float* params, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                          float beta2, float epsilon, int64_t step, int32_t last_is_log_eps, const float* terms6,
                          float scale, double* loss_out, void* stream);

/* ---- training on the GEMM engine (next-row f1 for config 5 and for wide nets) ----------------------------------
 * l2hmc_train_propose_grad's contract -- ONE proposal per chain in the chain's own direction, its accept
 * probability, the loss argument and the gradient of the loss term (accumulated into `grad`) -- for the samplers the
 * register-resident kernels cannot hold: S/T/Q nets of any width H, the shared image branch aux_encoder(aux) in their
 * first hidden layer, and the VAE latent-posterior energy (mnist_vae.py:104-226, the "trained sampler" of BASELINE.json
 * config 5); or, with `energy` set, any built-in target of utils/distributions.py with wide nets.
 *   v1_n = sum_k w_nk (Lx_nk - x_nk)^2 p_n + 1e-4;      term = scale * mean_n(1 / v1_n) - mean_n(v1_n) / scale
 *   w = dist_weight (N, d) or NULL (= 1).  SCGExperiment.ipynb raw 164-169: w = 1, scale = 0.1;
 *   mnist_vae.py:207-214 (energy_scale = 0): w = 1 / (exp(2 log_sigma) + 1e-4), scale = 1.
 * grad layout: [XNet | VNet | d/d eps | aux_encoder (W1, b1, W2, b2, W3, b3)], each net in NET_FIELDS order;
 * l2hmc_train_split_grad_floats(d, H, aux_encoder) floats (l2hmc_adam_step applies it, last_is_log_eps = 0 when the
 * image branch follows -- multiply the eps entry by eps first).  The decoder is NOT trained here (the reference trains
 * it by a separate optimiser on the ELBO, mnist_vae.py:229-262).
 * dLx_in (N, d) or NULL: a cotangent added to d loss / d Lx -- what a LATER proposal of the same step sends back when
 * proposals are chained without stop_gradient (mnist_vae.py:185-224); dx0_out (N, d) or NULL receives d loss / d x.
 * inv_n = 0 with dLx_in: the proposal has no loss term of its own (an earlier link of such a chain).
 * Every sum over chains is chunked and added in chunk order: the gradient is bitwise reproducible. */
typedef struct L2hmcTrainSplitArgs {
  const L2hmcNet* xnet;
  const L2hmcNet* vnet;
  int32_t H;
  const L2hmcMlp3* aux_encoder;  /* (n_pix -> H) or NULL                                                   */
  const L2hmcMlp3* decoder;      /* (d -> n_pix); NULL with `energy`                                       */
  const float* aux;              /* (N, n_pix)                                                             */
  const L2hmcEnergy* energy;     /* NULL: the decoder posterior.  Else a built-in target (as l2hmc_energy takes it),
                                  * its temperature honoured (anneal_beta is not).  An energy of kind 0 next to the decoder
                                  * posterior or energy_cb carries only the temperature (anneal_beta = 0): the library
                                  * tempers the decoder's U, grad U and Hessian-vector products itself, the callbacks
                                  * return those of U / temperature; the energy_scale term uses the plain U either way */
  const float* hess;             /* GAUSS_DENSE / GMM: the RAW (n_comp, d, d) precisions (Hessian-vector products)   */
  const float* masks;            /* (T, d) */
  const float* trig;             /* (T, 2) */
  const float* alpha;            /* device log(eps) or NULL -> eps_host */
  float eps_host;
  int64_t n_chains;
  int32_t d, T;
  const float* x;                /* (N, d) start points                          */
  const float* v;                /* (N, d) momenta of each chain's own direction */
  const uint8_t* direction;      /* (N) or NULL -> direction_all                 */
  int32_t direction_all;
  const float* dist_weight;      /* (N, d) or NULL */
  float scale, inv_n;
  const float* dLx_in;           /* (N, d) or NULL */
  float *Lx, *p, *v1;            /* (N, d), (N), (N) */
  float* dx0_out;                /* (N, d) or NULL */
  float* grad;                   /* accumulated */
  float* workspace;              /* l2hmc_train_split_workspace_floats(...) floats */
  int64_t workspace_floats;
  /* ---- the rest of mnist_vae.py:185-226's sampler objective ---------------------------------------------------- */
  float energy_scale;            /* es >= 0 (0 = off): + es inv_n sum_n (1 / ed_n - ed_n) with
                                  *    ed = (U(Lx) - U(x))^2 p + 1e-4   (mnist_vae.py:214,218,224)               */
  float* ediff_out;              /* (N) ed_n, or NULL                                                          */
  /* links of chain_operator (sampler.py:57-85; mnist_vae.py:193-196 `random_lf_composition`): the composed proposals
   * run with log_jac = True and have no accept probability of their own; the ONE accept probability of the
   * composition (and the loss) is formed by the caller from the links' outputs, its cotangents come back in here */
  int32_t no_accept;             /* 1: no p / v1 / loss term; seeds = dLx_in (required), dLv_in, dlogjac_in     */
  const float* dLv_in;           /* (N, d) or NULL: cotangent on the proposal's momentum Lv                     */
  const float* dlogjac_in;       /* (N) or NULL: cotangent on the proposal's summed log-Jacobian                */
  float* Lv_out;                 /* (N, d) or NULL                                                              */
  float* logjac_out;             /* (N) or NULL                                                                 */
  int32_t gemm_mode;             /* as L2hmcSplitArgs.gemm_mode                                                 */
  int32_t net_mode;              /* 0: one launch per S/T/Q net evaluation and one per its reverse wherever the
                                  *    shapes allow (H % 4 == 0, d even, widths <= 256); 1: three GEMM launches each
                                  *    (the form every other shape takes; here for A/B measurements and tests)     */
  /* ---- training on a caller-supplied energy (energy = decoder = NULL; aux only feeds aux_encoder, if any) ------- */
  L2hmcEnergyCallback energy_cb; /* U / grad U at a trajectory point (as in L2hmcSplitArgs), or NULL              */
  L2hmcHvpCallback hvp_cb;       /* its Hessian-vector product; required with energy_cb                          */
  void* energy_cb_user;          /* first argument of both callbacks                                              */
  /* ---- (ABI 6) training caller-supplied nets: xnet = vnet = aux_encoder = NULL, H ignored; with any target (a built-in
   *      `energy`, energy_cb + hvp_cb, or the decoder posterior).  Every net evaluation of the forward pass is net_cb (final S | T | Q into the library's
   *      stash), every one of the reverse sweep net_vjp_cb; `grad` then holds ONE float, d loss / d eps (accumulated) --
   *      the nets' parameter gradients are accumulated by the callback on the caller's side ---------------------------- */
  L2hmcNetCallback net_cb;
  L2hmcNetVjpCallback net_vjp_cb;
  void* net_cb_user;             /* first argument of both                                                        */
} L2hmcTrainSplitArgs;

int64_t l2hmc_train_split_grad_floats(int32_t d, int32_t H, const L2hmcMlp3* aux_encoder);
int64_t l2hmc_train_split_workspace_floats(int64_t n_chains, int32_t d, int32_t H, int32_t T,
                                           const L2hmcMlp3* aux_encoder, const L2hmcMlp3* decoder);
int l2hmc_train_split_grad(const L2hmcTrainSplitArgs* args, void* stream);

/* One Adam update as tf.train.AdamOptimizer applies it (SCGExperiment.ipynb raw 178-181) over the flat parameter
 * vector laid out like the gradient of l2hmc_train_propose_grad ([XNet | VNet | alpha]):
 *   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr_t m / (sqrt(v) + eps)
 * step = t >= 1.  last_is_log_eps: the last parameter is alpha = log eps while grad holds d/d eps there, so its
 * gradient is multiplied by exp(alpha) first (dynamics.py:50-58). */
int l2hmc_adam_step(float* params, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float epsilon, int64_t step, int32_t last_is_log_eps, void* stream);

/* AIS bookkeeping around one annealed HMC transition (utils/ais.py:44-66), initial energy N(0, I):
 *   begin: w += dbeta (|x|^2 / 2 - U_final(x))                                   (ais.py:58-59)
 *          v  = normals                          if refreshment < 0               (ais.py:57)
 *             = v sqrt(1 - r) + normals sqrt(r)  otherwise                        (ais.py:55)
 *   end:   accept = p - u >= 0;  x = accept ? Lx : x;  v = accept ? Lv : -Lv;  alpha_sum += p   (ais.py:62-66)
 * The transition itself is l2hmc_trajectory in HMC mode with energy.anneal_beta = beta. */
int l2hmc_ais_begin_step(const float* x, const float* U_final, const float* normals, float refreshment,
                         float dbeta, float* w, float* v, int64_t n_chains, int32_t d, void* stream);
int l2hmc_ais_end_step(const float* Lx, const float* Lv, const float* p, const float* u, float* x, float* v,
                       float* alpha_sum, int64_t n_chains, int32_t d, void* stream);

/* The draws the sampler loop would use, written out ((M,N,d) normals, (M,N) direction bits,
 * (M,N) uniforms; any output may be NULL): for tests, and for reproducing a run's randomness. */
int l2hmc_rng_fill(uint64_t seed, uint64_t proposal0, int64_t chain_offset, int64_t n_chains,
                   int32_t d, int32_t n_proposals, float* v_out, uint8_t* dir_out, float* u_out,
                   void* stream);

/* autocovariance / acl_spectrum (utils/func_utils.py:45-54,114-116) of a recorded chain history
 * X (steps, N, d) kept on the device:
 *   A_out[tau] = mean_t [ sum_{n,k} X[t,n,k] X[t+tau,n,k] / N ] / scale^2,  tau = 0 .. steps-2
 * (no mean subtraction, like the reference).  sums_out (steps-1 doubles) receives the raw
 * sums S(tau) = sum_t sum_{n,k} X[t] X[t+tau] -- the quantity ranks all-reduce when the chains
 * are sharded; pass n_total = chains over ALL ranks for the normalisation of A_out (A_out may be
 * NULL when only the partial sums are wanted).
 * `workspace`: l2hmc_autocov_workspace_doubles(steps, n_chains, d) doubles -- every block writes its partial
 * sums there and a second kernel adds them in block order, so S (and with it the thresholded ESS) is bitwise
 * reproducible; NULL = accumulate with double atomics instead (order-dependent in the last bits). */
int64_t l2hmc_autocov_workspace_doubles(int64_t steps, int64_t n_chains, int32_t d);
int l2hmc_autocov(const float* X, int64_t steps, int64_t n_chains, int32_t d, double scale,
                  int64_t n_total, double* sums_out, double* A_out, double* workspace, void* stream);

/* Per-coordinate convergence diagnostics of a recorded chain history X (steps, N, d) kept on the device: the raw sums behind
 * split R-hat and the effective sample size of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), without rank
 * normalisation (l2hmc_amd/diagnostics.py `finish` turns them into numbers on the host).  Unlike l2hmc_autocov the series are
 * centred with their own means and the lag sums are kept apart by coordinate.
 *   split = 1: Mh = steps / 2 and every chain is two series, rows [0, Mh) and [steps - Mh, steps) (an odd `steps` drops the
 *              middle row): C = 2 N series per coordinate, first halves then second halves.  split = 0: Mh = steps, C = N.
 *   mean_out (C, d)          m[c, k]  = mean_t x                                   (float64 accumulation)
 *   m2_out   (C, d)          M2[c, k] = sum_t (x_t - m)^2                          (float64 accumulation)
 *   G_out    (d, max_lag+1)  G[k, t]  = sum_c sum_{i < Mh - t} (x_i - m[c, k]) (x_{i+t} - m[c, k])
 *                            (values centred in float64; products in float32 chunks of 32 steps folded into float64)
 * These are what ranks that hold different chains all-reduce (G as it is, sum_c m, sum_c m^2, sum_c M2 and the count C).
 * `workspace`: l2hmc_chain_stats_workspace_doubles(...) doubles, required -- every block writes its partial sums there and
 * they are added in block order: no floating-point atomics, the outputs are bitwise reproducible.
 * Its size does not grow with n_chains but with d: about 1024 blocks' worth of min(d, 256) (max_lag + 1) doubles, and the block
 * count is a multiple of d / gcd(256, d) -- 7.7 MB at d = 25, 67 MB at d = 512, 536 MB at d = 511 with max_lag = 255 and split = 1.
 * L2HMC_ERR_ARG (before any launch): a NULL pointer, steps / n_chains < 1, d outside 1 .. 512, split not 0 / 1, Mh < 4,
 * C < 2, max_lag outside 0 .. Mh - 1.  A non-finite value makes the sums of its own coordinate non-finite, nothing else. */
int64_t l2hmc_chain_stats_workspace_doubles(int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split);
int l2hmc_chain_stats(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                      double* mean_out, double* m2_out, double* G_out, double* workspace, void* stream);

/* The same sums for the indicator series y = ((double) x <= thresholds[k]) ? 1 : 0 of every coordinate k, applied as the value
 * is loaded (no indicator history is written): what the effective sample size of a quantile estimate is made of (Vehtari et
 * al. 2021, `ess_quantile`; l2hmc_amd/quantiles.py).  `thresholds`: d float64 on the device.  The contract, the argument checks
 * and the workspace size are those of l2hmc_chain_stats; a NaN value or threshold gives y = 0. */
int l2hmc_chain_stats_below(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                            const double* thresholds /* (d), device */, double* mean_out, double* m2_out, double* G_out,
                            double* workspace, void* stream);

/* The same sums for the series y = (float) exp((double) x - shift[k]) of every coordinate k, formed as the value is loaded (no
 * second history is written): the likelihoods of a log-likelihood history, whose effective sample size over the number of draws
 * is the relative efficiency of PSIS-LOO (l2hmc_amd/psis.py `relative_eff_from_log_lik`).  `shift`: d float64 on the device,
 * usually the coordinate's maximum -- the effective sample size does not move with it, it only keeps e^x inside float32.  The
 * exponential is the double-precision one, rounded to float32 once.  The contract, the argument checks and the workspace size
 * are those of l2hmc_chain_stats; a NaN value or shift makes the sums of its own coordinate NaN. */
int l2hmc_chain_stats_exp(const float* X, int64_t steps, int64_t n_chains, int32_t d, int32_t max_lag, int32_t split,
                          const double* shift /* (d), device */, double* mean_out, double* m2_out, double* G_out,
                          double* workspace, void* stream);

/* Exact order statistics of every coordinate of a history kept on the device (csrc/order_stats.hip; l2hmc_amd/quantiles.py
 * builds quantiles, tail-ESS and the quantile MCSE on them).
 *   X       (n_draws, d) float32, contiguous, read in place: element (i, k) at X[i d + k] -- a recorded history (M, N, d) with
 *           n_draws = M N, or a first-axis slice of one.
 *   ranks   (n_ranks, d) int64 on the device, 0-based; every coordinate has its own.
 *   values  (n_ranks, d) float32: values[r, k] is the element a full ascending sort of coordinate k puts at position
 *           ranks[r, k] -- one of the input's own values, exact.  -0 sorts before +0, every NaN after +inf (and comes back as a
 *           NaN); a rank at or past n_draws gives the maximum, a negative one the minimum.
 *   n_nan   (d) int64: the NaNs of each coordinate.
 * Method: most-significant-digit radix select on the monotone key of a float (bits ^ 0xFFFFFFFF when negative, else
 * bits | 0x80000000) in l2hmc_order_stats_passes() passes of log2 l2hmc_order_stats_bins() bits.  A pass is a COUNT -- the
 * history is read once per coordinate / rank group (64 (coordinate, rank) pairs fit one group; pass 0 needs no rank groups) and
 * hist[r, k, :] receives the histogram of the next digit of the keys that share the prefix of (r, k) -- and an ADVANCE that
 * picks the digit in which the remaining rank falls.  Counts are integers added with integer atomics: every output is bitwise
 * reproducible, and histograms of different draws simply add (ranks that hold different draws all-reduce `hist`, and n_nan in
 * pass 0, between the two halves).  Nothing returns to the host between passes; nothing is allocated.
 *   workspace   l2hmc_order_stats_workspace_bytes(d, n_ranks) bytes, 16-byte aligned: hist | remaining | prefix.
 *   prefix      (n_ranks, d) uint32, zero before pass 0 (not read in pass 0: may be NULL there);
 *   remaining   (n_ranks, d) int64, the ranks before pass 0; both are updated by every advance.
 * l2hmc_order_stats is exactly count, advance for pass 0, 1, ... on the workspace: both routes give the same bits.
 * L2HMC_ERR_ARG (before any launch): n_draws < 1, d outside 1 .. 512, n_ranks outside 1 .. 32, n_draws > 2^40 / d, a pass
 * outside 0 .. passes - 1, a NULL pointer that the pass needs. */
int32_t l2hmc_order_stats_passes(void);
int32_t l2hmc_order_stats_bins(void);                         /* bins of the widest pass */
int64_t l2hmc_order_stats_workspace_bytes(int32_t d, int32_t n_ranks);
int l2hmc_order_stats(const float* X, int64_t n_draws, int32_t d, const int64_t* ranks, int32_t n_ranks, float* values,
                      int64_t* n_nan, void* workspace, void* stream);
int l2hmc_order_stats_count(const float* X, int64_t n_draws, int32_t d, int32_t n_ranks, int32_t pass, const uint32_t* prefix,
                            int64_t* hist /* (n_ranks, d, bins), zeroed by the call */,
                            int64_t* n_nan /* written in pass 0, else may be NULL */, void* stream);
int l2hmc_order_stats_advance(const int64_t* hist, int64_t* remaining, uint32_t* prefix, int32_t d, int32_t n_ranks,
                              int32_t pass, float* values /* written after the last pass, else may be NULL */, void* stream);

/* Bayesian logistic regression: the per-row sums behind the posterior predictive, the lppd and WAIC over every recorded draw
 * (csrc/predictive.hip; l2hmc_amd/predictive.py `finish` turns them into numbers on the host).
 *   draws   (n_draws, d) float32 row-major on the device, read in place: a first-axis slice of a recorded history (M, N, d)
 *           viewed as (M N, d) is fine -- only 4-byte alignment is needed.
 *   packed  the buffer l2hmc_pack_logistic wrote for (X, y) with the same d (its labels are used; pack zeros when there are
 *           none: the first sum does not depend on them), 16-byte aligned.
 *   sums    (4, n_data) float64, with l = x_i . w_s, z = (2 y_i - 1) l, both over the draws s:
 *             [0] sum sigmoid(l)   [1] sum lik, lik = sigmoid(z)   [2] sum ll, ll = log lik = -softplus(-z)   [3] sum ll^2
 *           The logits are float32 (f32-input MFMA, features past d contribute zero), sigmoid / softplus use the hardware
 *           exp, log and reciprocal in float32; every value is converted to float64 BEFORE it is added and ll^2 is formed in
 *           float64.  sum lik = 0 (every draw's likelihood below float32's range) is a value, not an error: the caller reports it.
 * `workspace`: l2hmc_logistic_predict_workspace_doubles(...) doubles, required -- every wave writes its partial sums there
 * and a second kernel adds them in a fixed order: no floating-point atomics, two calls give identical bits.  At most about
 * 4096 x 256 x 4 doubles whatever the shape, 4 n_data when n_data is large.
 * L2HMC_ERR_ARG (before any launch): n_draws < 2, n_data outside 1 .. 1048576, d outside 1 .. 128, n_draws > 2^40 / d, a NULL
 * or misaligned pointer. */
int64_t l2hmc_logistic_predict_workspace_doubles(int64_t n_draws, int32_t n_data, int32_t d);
int l2hmc_logistic_predict(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data,
                           double* sums /* (4, n_data) */, double* workspace, void* stream);

/* Bayesian logistic regression: the per-row raw material of PSIS-LOO (Pareto-smoothed importance-sampling leave-one-out;
 * Vehtari, Gelman, Gabry 2017) over every recorded draw (csrc/loo.hip; l2hmc_amd/predictive.py `loo_finish` turns it into
 * elpd_loo and the Pareto k-hat).  `draws` and `packed` are those of l2hmc_logistic_predict.  With t = (2 y_i - 1) x_i . w_s the
 * signed logit of row i under draw s (float32, f32-input MFMA) and M = l2hmc_logistic_loo_tail_len(n_draws) =
 * min(n_draws / 5, ceil(3 sqrt(n_draws))), per row i:
 *   cutoff  (n_data) float32: the element of rank M (0-based) of an ascending order of {t_s}; the order is that of the monotone
 *           key of l2hmc_order_stats (-0 before +0, every NaN after +inf).
 *   n_tail  (n_data) int64: L = the number of t strictly before the cutoff in that order, L <= M (ties at the cutoff shorten it).
 *   tail    (n_data, M) float32: those L values in ANY order in slots 0 .. L - 1, +inf in slots L .. M - 1 (may be NULL when M = 0).
 *   sums    (2, n_data) float64: [0] body = the sum over the draws NOT in the tail of e^m + e^(m - t), m = min(cutoff, 0) (every
 *           term in (0, 2]: log of the summed ratios 1 + e^-t is log(body) - m); [1] the sum over all draws of sigmoid(t).
 *           Every term is float32 (hardware exp and reciprocal) and is converted to float64 BEFORE it is added.
 * The cutoff is found by a radix select (4 passes of 8 bits: a fused contraction and histogram each, nothing is sorted and the
 * (n_draws, n_data) matrix is never written) and one more pass gathers; every pass forms bit-identical t.  `workspace`:
 * l2hmc_logistic_loo_workspace_bytes(...) bytes, 8-byte aligned, required: error word | histograms | ranks | prefixes | the
 * waves' partial sums, which a last kernel adds in a fixed order.  No floating-point atomics: cutoff, n_tail, the tail as a set
 * and the sums are bitwise reproducible, and the same whatever set of rows a call holds (the draws are cut into chunks by
 * n_draws alone).  The first int64 of the workspace is non-zero after the call if a tail slot at or past M was asked for (never
 * while the passes agree; the value is then not written and n_tail counts it).
 * L2HMC_ERR_ARG (before any launch): n_draws < 2, n_data outside 1 .. 1048576, d outside 1 .. 128, n_draws > 2^40 / d, a tail
 * the caller could not have sized (M n_data > 2^31: call with fewer rows), a NULL or misaligned pointer. */
int64_t l2hmc_logistic_loo_tail_len(int64_t n_draws);
int64_t l2hmc_logistic_loo_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d);
int l2hmc_logistic_loo_tails(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data,
                             float* cutoff /* (n_data) */, int64_t* n_tail /* (n_data) */, float* tail /* (n_data, M) */,
                             double* sums /* (2, n_data): body, sum_lik */, void* workspace, void* stream);

/* l2hmc_logistic_loo_tails for a run of autocorrelated draws (`predictive.loo(r_eff=...)`): every row has its own tail length
 * M_i = tail_len_row[i], 0 <= M_i <= tail_stride < n_draws (int64 on the device; an entry outside is clamped), chosen by the
 * caller from the row's relative efficiency.  cutoff[i] is the element of rank M_i, n_tail[i] = L_i <= M_i, `tail` is
 * (n_data, tail_stride) with +inf in the slots at or past L_i, and `sums` is (3, n_data): [0] body and [1] sum_lik as above,
 * [2] body_sq = the sum over the draws NOT in the tail of (e^m + e^(m - t))^2, every float32 term squared exactly in float64
 * (in (0, 4]): the sum of the squared importance ratios of the body is e^(-2 m) body_sq.  With every M_i =
 * l2hmc_logistic_loo_tail_len(n_draws) = tail_stride, then cutoff, n_tail, the tail as a set, body and sum_lik are those of
 * l2hmc_logistic_loo_tails bit for bit.  `workspace`: l2hmc_logistic_loo_mc_workspace_bytes(...) bytes (a third partial sum);
 * its first int64 is non-zero after the call if a tail slot at or past M_i was asked for.  Reproducibility and the other
 * argument errors are those of l2hmc_logistic_loo_tails; also L2HMC_ERR_ARG: tail_stride outside 0 .. n_draws - 1,
 * tail_stride n_data > 2^31, tail_len_row NULL or not 8-byte aligned. */
int64_t l2hmc_logistic_loo_mc_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d);
int l2hmc_logistic_loo_tails_mc(const float* draws, int64_t n_draws, int32_t d, const float* packed, int32_t n_data,
                                const int64_t* tail_len_row /* (n_data) */, int64_t tail_stride, float* cutoff /* (n_data) */,
                                int64_t* n_tail /* (n_data) */, float* tail /* (n_data, tail_stride) */,
                                double* sums /* (3, n_data): body, sum_lik, body_sq */, void* workspace, void* stream);

/* PSIS of ANY likelihood: the per-column raw material of Pareto-smoothed importance sampling of a pointwise log-likelihood
 * matrix (csrc/loglik_tails.hip; l2hmc_amd/psis.py `loo_from_log_lik(select="fused")` and `psis(select="fused")` finish it on
 * l2hmc_psis_smooth).  The log importance ratio of column i under draw s is -ll[s, i]: the largest ratios are the smallest ll.
 *   ll            (n_draws, n_cols) float32, row-major and contiguous on the device, read in place; n_cols in 1 .. 512.
 *   tail_len_col  (n_cols) int64 on the device: the tail length M_i of every column, 0 <= M_i <= tail_stride (an entry outside
 *                 is clamped); NULL = l2hmc_logistic_loo_tail_len(n_draws) for all (clamped to tail_stride as well).
 *   cutoff  (n_cols) float32: the element of ascending rank M_i of column i, in the total order of the monotone key of
 *           l2hmc_order_stats (-0 before +0, every NaN after +inf).
 *   top     (n_cols) float32: the element of rank n_draws - 1, the column's maximum; NaN when the column holds a NaN.
 *   n_tail  (n_cols) int64: L_i = the number of ll strictly before the cutoff in that order, L_i <= M_i (ties shorten it).
 *   tail    (n_cols, tail_stride) float32: those L_i values in ANY order in slots 0 .. L_i - 1, +inf in the other slots (may be
 *           NULL when tail_stride = 0).
 *   tail_pos  the same shape, int64, or NULL: the draw s every tail value came from, -1 in the other slots.
 *   sums    (3, n_cols) float64, with c = cutoff and every term formed in float64 from the exact float32 values (the difference,
 *           then the double-precision exp, one call per term):
 *             [0] body = the sum over the draws NOT in the tail of e^(c - ll)   (every term in (0, 1])
 *             [1] body_sq = the same sum of e^(2 (c - ll))      [2] lik = the sum over all draws of e^(ll - top)
 *           so that the summed ratios of the body are e^(-c) body, their squares e^(-2 c) body_sq, and lppd = log lik + top - log S.
 * Both ranks of every column are found by l2hmc_order_stats (one call, two ranks) and one more pass over the matrix gathers.
 * `workspace`: l2hmc_loglik_tails_workspace_bytes(...) bytes, 16-byte aligned, required: error word | ranks | values | the
 * select's workspace | one partial per (segment of draws, sum, column), which a last kernel adds in segment order.  The draws are
 * cut into segments by n_draws alone and there are no floating-point atomics: every output (the tail as a set of (value, draw)
 * pairs) is bitwise reproducible, and a column gives the same bits whichever other columns share the call.  The first int64 of the
 * workspace is non-zero after the call if a tail slot at or past M_i was asked for (never while the select and the gather agree;
 * the value is then not written and n_tail counts it).
 * A column whose cutoff is not finite: c = -inf (more than M_i draws at -inf) has an empty tail and body = body_sq = NaN;
 * c = +inf has NaN there as well; c = NaN (fewer than M_i + 1 numbers in the column) gathers every number and has three NaN
 * sums.  The finished numbers are then NaN or infinite exactly where those of the `torch.topk` route of psis.py are.
 * L2HMC_ERR_ARG (before any launch): n_draws < 2, n_cols outside 1 .. 512, n_draws > 2^40 / n_cols, tail_stride outside
 * 0 .. n_draws - 1, tail_stride n_cols > 2^31, a NULL required pointer, ll / cutoff / top / tail not 4-byte, n_tail / tail_pos /
 * tail_len_col / sums not 8-byte, workspace not 16-byte aligned. */
int64_t l2hmc_loglik_tails_workspace_bytes(int64_t n_draws, int32_t n_cols);
int l2hmc_loglik_tails(const float* ll, int64_t n_draws, int32_t n_cols,
                       const int64_t* tail_len_col /* (n_cols) device, or NULL = loo_tail_len(n_draws) for all */,
                       int64_t tail_stride, float* cutoff, float* top, int64_t* n_tail,
                       float* tail /* (n_cols, tail_stride) */, int64_t* tail_pos /* same shape, or NULL */,
                       double* sums /* (3, n_cols) */, void* workspace, void* stream);

/* Bayesian logistic regression: the raw sums behind the per-row relative efficiency of PSIS-LOO, r_eff_i = ESS(p(y_i | theta)) / S
 * (Vehtari, Gelman, Gabry 2017; csrc/lik_stats.hip; l2hmc_amd/predictive.py `relative_eff`).  `draws` is a recorded history
 * (steps, n_chains, d) float32 on the device, read in place (a first-axis slice is fine: 4-byte alignment); `packed` is that of
 * l2hmc_logistic_predict.  The series are the likelihoods lik[t, c, i] = sigmoid((2 y_i - 1) x_i . w[t, c]) -- the float32 logits
 * and likelihoods of l2hmc_logistic_loo_tails, bit for bit -- and the outputs are those of l2hmc_chain_stats for that derived
 * history, which is never written, with the data row in the place of the coordinate.  `split`, Mh and C mean what they mean there:
 *   mean  (C, n_data)            m[c, i]  = mean_t lik                                  (float64 accumulation)
 *   m2    (C, n_data)            M2[c, i] = sum_t (lik_t - m)^2                         (float64 accumulation)
 *   G     (n_data, max_lag + 1)  G[i, t]  = sum_c sum_{s < Mh - t} (lik_s - m[c, i]) (lik_{s+t} - m[c, i])
 *                                (values centred in float64 and rounded to float32 once; products in float32 chunks of 8 steps
 *                                folded into float64)
 * l2hmc_amd/diagnostics.py `reduce_sums` and `finish` take them as they take l2hmc_chain_stats' outputs.
 * `workspace`: l2hmc_logistic_lik_stats_workspace_bytes(...) bytes, 8-byte aligned, required -- the waves' partial lag sums, which
 * a last kernel adds in a fixed order: at most 2 x 16 x n_data x (max_lag + 1) doubles.  No floating-point atomics: two calls
 * give identical bits, and a row's numbers do not depend on which other rows share the call.  A non-finite draw makes the sums of
 * its own chain (mean, m2) and of the rows it meets (G) non-finite, nothing else.
 * L2HMC_ERR_ARG (before any launch): steps / n_chains < 1, split not 0 / 1, Mh < 4, C < 2, max_lag outside 0 .. Mh - 1, steps
 * n_chains < 2 or > 2^40 / d, n_data outside 1 .. 1048576, d outside 1 .. 128, a NULL or misaligned pointer. */
int64_t l2hmc_logistic_lik_stats_workspace_bytes(int64_t steps, int64_t n_chains, int32_t d, int32_t n_data, int32_t max_lag,
                                                 int32_t split);
int l2hmc_logistic_lik_stats(const float* draws, int64_t steps, int64_t n_chains, int32_t d, const float* packed, int32_t n_data,
                             int32_t max_lag, int32_t split, double* mean /* (C, n_data) */, double* m2 /* (C, n_data) */,
                             double* G /* (n_data, max_lag + 1) */, void* workspace, void* stream);

/* Generalised linear models: the pointwise log-likelihood matrix, the raw material of PSIS-LOO and the sums behind the posterior
 * predictive mean and WAIC over every recorded draw (csrc/glm.hip, the family in csrc/glm_family.hpp; l2hmc_amd/glm.py and
 * `PoissonRegression` turn them into numbers).  Additive to ABI 6.  Common arguments:
 *   draws       (n_draws, d) float32 row-major on the device, read in place (a first-axis slice of a history: 4-byte alignment).
 *   packed      the buffer l2hmc_pack_logistic wrote for (X, y) with the same d, the responses y in the label slot (counts up
 *               to 2^24 are exact in float32), 16-byte aligned.
 *   row_consts  (3, n_data) float32 on the device, contiguous: [0] the offset o_i (log exposure), [1] g_i = lgamma(y_i + 1)
 *               formed in float64 and rounded once, [2] the saturated log-likelihood sat_i = y log y - y - lgamma(y + 1) (0 at
 *               y = 0), the supremum of ll over eta.
 *   family      L2HMC_GLM_POISSON: with eta = x_i . w_s (float32, f32-input MFMA), h = eta + o_i and mu = exp(h) (hardware
 *               exp2), ll = fma(y_i, h, -mu) - g_i, four float32 roundings.
 *               L2HMC_GLM_BINOMIAL and L2HMC_GLM_NEGBINOMIAL: row_consts is (4, n_data): [0] the offset o_i, [1] the weight m_i,
 *               [2] sat_i = y log(y / m) + (m - y) log(1 - y / m) + c_i (0 log 0 = 0), [3] the constant c_i, each formed in float64
 *               and rounded once.  With t = eta + o_i, e = exp(-|t|) (hardware exp2) and softplus(t) = max(t, 0) + log(1 + e):
 *               ll = fma(y_i, t, -(m_i softplus(t))) + c_i -- the float32 operations of L2HMC_ENERGY_BINOMIAL, whose U term is
 *               c_i - ll bit for bit.  BINOMIAL: m_i trials, c_i = log C(m_i, y_i), predictive mean m_i sigmoid(t).
 *               NEGBINOMIAL (NB2, dispersion phi): m_i = y_i + phi, o_i = offset_i - log phi, c_i = lgamma(y_i + phi) -
 *               lgamma(phi) - lgamma(y_i + 1); sums[0] adds exp(t) = mu / phi (the caller multiplies by phi; +inf as IEEE
 *               gives it).  The absolute error of a float32 ll grows with m |t| (as the Poisson family's with y |h|).
 *               L2HMC_GLM_PROBIT: binomial regression with the probit link.  row_consts is the binomial's (4, n_data) [o_i, m_i,
 *               sat_i, c_i] (the supremum of ll is at Phi(t) = y / m: the same sat).  With t = eta + o_i,
 *               ll = y_i log Phi(t) + (m_i - y_i) log Phi(-t) + c_i by the float32 operations of L2HMC_ENERGY_PROBIT
 *               (ProbitLink), whose U term is c_i - ll bit for bit; the predictive mean is m_i Phi(t).
 *               Any other value (0, 2, 5, 7, ...) is L2HMC_ERR_ARG "unknown family".
 * Every kernel forms ll by the one device function of the family: the bits of ll[s, i] depend on (draws, X, y, row_consts)
 * alone -- not on the entry, the pass, the chunk or the rows that share a call.
 *
 * l2hmc_glm_log_lik writes out (n_draws, n_data) float32 row-major, out[s n_data + i] = ll[s, i]: the very values the two
 * fused entries work on.  The slow route (the caller forms it in row groups), and the feed of l2hmc_loglik_tails and
 * l2hmc_chain_stats_exp.  Also L2HMC_ERR_ARG: n_draws n_data > 2^40.
 *
 * l2hmc_glm_predict: sums (4, n_data) float64 over the draws: [0] sum mu   [1] sum exp((double) ll - sat_i), one double-precision
 * exp per term, every term in (0, 1] up to the rounding of sat_i, so that lppd_i = log(sums[1] / n_draws) + sat_i and no pass
 * looks for a shift   [2] sum ll   [3] sum ll^2 (formed and added in float64).  `workspace`:
 * l2hmc_glm_predict_workspace_doubles(...) doubles, required; the waves' partials are added in chunk order: no floating-point
 * atomics, two calls give identical bits.
 *
 * l2hmc_glm_loo_tails: the outputs of l2hmc_loglik_tails (cutoff, top, n_tail, tail with +inf pads, sums (3, n_data) = body,
 * body_sq, lik; no tail_pos) of the matrix l2hmc_glm_log_lik would write, which is never formed: four fused count passes of a
 * radix select on the keys of ll (pass 0 also takes the row's largest key with an integer atomic maximum), then one gather.
 * tail_len_row (n_data) int64 on the device or NULL (= l2hmc_logistic_loo_tail_len(n_draws) for all), clamped to
 * 0 .. tail_stride; `tail` is (n_data, tail_stride).  Every term of the sums is the double-precision exp of the exact difference
 * of two float32 values, one call per term: the per-term bound and the table of non-finite cutoffs of l2hmc_loglik_tails hold.
 * cutoff, top, n_tail, the tail as a set AND the three sums equal those of l2hmc_loglik_tails on the written matrix bit for
 * bit: the terms are added in that entry's order (segments of max(64, ceil(n_draws / 2048)) consecutive draws, each in draw
 * order, then the segments in order -- cut by n_draws alone, so a row's bits do not depend on the other rows of the call).
 * `workspace`: l2hmc_glm_loo_workspace_bytes(...) bytes, 8-byte aligned, required: error word | histograms | ranks | prefixes |
 * largest keys | partial sums; its first int64 is non-zero after the call if a tail slot at or past a row's length
 * was asked for (never while the passes agree).
 * L2HMC_ERR_ARG (before any launch): an unknown family, n_draws < 2, n_data outside 1 .. 1048576, d outside 1 .. 128,
 * n_draws > 2^40 / d, tail_stride outside 0 .. n_draws - 1, tail_stride n_data > 2^31, a NULL required pointer (tail may be
 * NULL when tail_stride = 0), draws / row_consts / cutoff / top / tail / out not 4-byte, packed not 16-byte, n_tail /
 * tail_len_row / sums / workspace not 8-byte aligned. */
enum { L2HMC_GLM_POISSON = 1, L2HMC_GLM_BINOMIAL = 3, L2HMC_GLM_NEGBINOMIAL = 4, L2HMC_GLM_PROBIT = 6 };
int l2hmc_glm_log_lik(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts /* (3 or 4, n_data) */,
                      int32_t n_data, int32_t family, float* out /* (n_draws, n_data) */, void* stream);
int64_t l2hmc_glm_predict_workspace_doubles(int64_t n_draws, int32_t n_data, int32_t d);
int l2hmc_glm_predict(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts, int32_t n_data,
                      int32_t family, double* sums /* (4, n_data) */, double* workspace, void* stream);
int64_t l2hmc_glm_loo_workspace_bytes(int64_t n_draws, int32_t n_data, int32_t d);
int l2hmc_glm_loo_tails(const float* draws, int64_t n_draws, int32_t d, const float* packed, const float* row_consts,
                        int32_t n_data, int32_t family, const int64_t* tail_len_row /* (n_data) device, or NULL */,
                        int64_t tail_stride, float* cutoff, float* top, int64_t* n_tail, float* tail /* (n_data, tail_stride) */,
                        double* sums /* (3, n_data): body, body_sq, lik */, void* workspace, void* stream);

/* Pareto-smoothed importance sampling of the tails of ANY log importance ratios, float64 throughout (csrc/psis.hip;
 * l2hmc_amd/psis.py `smooth_tails`, `psis`, `loo_from_log_lik`; `predictive.loo(finish="kernel")`).  Per row i:
 *   lam         (n_rows, tail_len) the L_i = n_tail[i] <= tail_len largest log ratios, descending, in slots 0 .. L_i - 1; a slot
 *               at or past L_i is never read
 *   n_tail      (n_rows) int64
 *   lam_cutoff  (n_rows) the log ratio of the cutoff (below every tail member)
 *   out         (3, n_rows): khat | lse_w = logsumexp_s omega_s | lse_wl = logsumexp_s (omega_s - lam_s), where omega_s is the
 *               smoothed log weight of slot s relative to the row's largest ratio.  L_i >= 5 and a finite fit (Zhang & Stephens
 *               2009 with the prior of `loo`; the formulas stand at the head of csrc/psis.hip): omega = the log of the
 *               generalised-Pareto quantile at (rank - 0.5) / L_i, capped at 0, and khat the fitted shape.  Otherwise
 *               omega_s = lam_s - lam_max and khat = +inf.  L_i = 0: -inf, -inf.  A NaN among a row's live slots makes that
 *               row's three outputs NaN and touches no other row.
 *   weights     (n_rows, tail_len) or NULL: omega in the input's slot order, -inf in the slots at or past L_i.
 * `workspace`: l2hmc_psis_workspace_bytes(n_rows, tail_len) bytes, 8-byte aligned, required: error word | x | the profile's
 * sums.  The first int64 of the workspace is non-zero after the call if an n_tail entry lay outside 0 .. tail_len (the row is
 * then computed with the entry clamped).  Every sum has a fixed order that depends on L_i alone and there are no floating-point
 * atomics: two calls give identical bits, and a row gives the same bits whichever other rows share the call.
 * l2hmc_psis_plan(n_rows, tail_len, what) reports the launch plan: what = 0 the theta blocks per row, 1 the workgroups along
 * the rows (further rows are taken in a loop), 2 the theta accumulators per thread, 3 the threads of a workgroup, 4 the
 * theta grid's length at tail_len.
 * L2HMC_ERR_ARG (before any launch): n_rows < 1, tail_len < 0, a tail the caller could not have sized (n_rows > 2^31 or
 * tail_len n_rows > 2^31: call with fewer rows), a NULL required pointer (lam may be NULL when tail_len = 0), a pointer that is
 * not 8-byte aligned.  tail_len = 0 is valid: every row has L = 0. */
int64_t l2hmc_psis_plan(int64_t n_rows, int64_t tail_len, int32_t what);
int64_t l2hmc_psis_workspace_bytes(int64_t n_rows, int64_t tail_len);
int l2hmc_psis_smooth(const double* lam, const int64_t* n_tail, const double* lam_cutoff, int64_t n_rows, int64_t tail_len,
                      double* out /* (3, n_rows) */, double* weights /* (n_rows, tail_len) or NULL */, void* workspace,
                      void* stream);

/* The raw first and second moments of a recorded history X (steps, N, d) kept on the device (csrc/moment_sums.hip): what the
 * posterior covariance and the multivariate effective sample size of Vats, Flegal & Jones (2019) are made of
 * (l2hmc_amd/multivariate.py `finish` turns them into numbers on the host, and ranks that hold different chains add them).
 *   sum_out         (d)     sum over all steps * n_chains draws of x
 *   cross_out       (d, d)  sum of x x^T; both triangles are written and carry identical bits
 *   batch_sum_out   (d)     sum over the batches of the batch MEAN ybar        -- NULL if and only if batch = 0
 *   batch_cross_out (d, d)  sum over the batches of ybar ybar^T, symmetric too -- NULL if and only if batch = 0
 * A batch is `batch` consecutive steps of ONE chain; a chain has a = steps / batch of them, over rows [steps - a batch, steps):
 * a leading remainder belongs to no batch (it still counts in sum_out and cross_out).  batch = 0 computes no batch sums, and
 * then steps x n_chains may be any factorisation of the rows of a (draws, d) array.
 * Arithmetic: every value is widened to float64 (exactly) before anything else happens to it; every product and every sum is
 * float64 on the matrix pipe (v_mfma_f64_16x16x4_f64), so the products are exact; a batch mean is a float64 sum divided once.
 * `workspace`: l2hmc_moment_sums_workspace_doubles(...) doubles, required -- every block writes its partial sums there and a
 * second kernel adds them in block order: no floating-point atomics, two calls give identical bits.  At most about
 * 256 blocks x 3 panels x 2 x 4352 doubles (53 MB, 64 < d <= 128 with batches); 1.4 MB at d = 25.
 * A non-finite entry makes the rows and columns of its own coordinate non-finite and nothing else: lanes past d or past the
 * last chain select an exact 0 and never multiply what they loaded.
 * L2HMC_ERR_ARG (before any launch): d outside 1 .. 128, steps or n_chains < 1, batch outside 0 .. steps,
 * n_chains > 2^40 / d or steps > 2^31, a required pointer NULL, batch outputs given with batch = 0 or missing with batch > 0. */
int64_t l2hmc_moment_sums_workspace_doubles(int64_t steps, int64_t n_chains, int32_t d, int64_t batch);
int l2hmc_moment_sums(const float* X, int64_t steps, int64_t n_chains, int32_t d, int64_t batch, double* sum_out,
                      double* cross_out, double* batch_sum_out, double* batch_cross_out, double* workspace, void* stream);

/* Warm-up: the step size eps = exp(*alpha) adapted on the device between launches of the sampler loop (csrc/adapt.hip;
 * l2hmc_amd/warmup.py drives it).  Every trajectory entry point reads *alpha from device memory when its kernel starts, so a
 * kernel that rewrites *alpha in place sets the step size of the next launch on the same stream: no host read, no synchronise,
 * no allocation, and no prepared copy of anything holds eps.
 *
 * `state`: L2HMC_ADAPT_STATE_DOUBLES device doubles.
 *   [0] phase (0 search, 1 averaging, 2 finished)   [1] dir (0, +1, -1)   [2] t   [3] log_eps   [4] log_eps_bar   [5] H_bar
 *   [6] mu   [7] last mean accept   [8] updates seen   [9..14] target, gamma, t0, kappa, log_eps_min, log_eps_max   [15] 0
 *
 * l2hmc_adapt_init reads *alpha on the device and writes the state: log_eps = (double) *alpha (not clamped), everything else 0;
 *   search = 0 starts in phase 1 with mu = log_eps + ln 10.
 * l2hmc_adapt_update takes p, the p_out of the window just run ((M, N) flattened: n floats), and does, in this order and in
 *   float64:
 *     a = (sum of p_i, a non-finite p_i counted as 0) / n
 *     phase 0 (Hoffman & Gelman 2014, Alg. 4, on the mean over chains):  d = a > 0.5 ? +1 : -1;  if dir == 0: dir = d;
 *       if d == dir: log_eps = clamp(log_eps + dir ln 2), and a clamp that binds starts averaging (below) at the clamped value;
 *       else start averaging: phase = 1, mu = log_eps + ln 10, t = 0, H_bar = 0, log_eps_bar = 0 (log_eps stays).
 *     phase 1 (Alg. 5):  t += 1;  w = 1 / (t + t0);  H_bar = (1 - w) H_bar + w (target - a);
 *       log_eps = clamp(mu - sqrt(t) / gamma H_bar);  e = t^-kappa;  log_eps_bar = e log_eps + (1 - e) log_eps_bar.
 *     phase 2: nothing.
 *     then *alpha = (float) log_eps, state[7] = a, state[8] += 1 and, if trace_row4 is given,
 *       trace_row4 = {a, log_eps the window ran at, log_eps now set, phase after}.
 *   mode L2HMC_ADAPT_REDUCE alone only writes sums2 = {sum of p_i, n}; L2HMC_ADAPT_APPLY alone takes a = sums2[0] / sums2[1] and
 *   ignores p and n -- what ranks run around ONE all-reduce of the two doubles; mode 3 does both in one launch (and writes sums2
 *   when it is given).  The sum has a fixed order (csrc/adapt.hip) and uses no floating-point atomics: state, alpha and trace are
 *   bitwise reproducible.  Windows of up to L2HMC_ADAPT_SINGLE_BLOCK_MAX values are one launch of one workgroup and need no
 *   workspace (l2hmc_adapt_workspace_doubles returns 0; NULL is fine); larger ones take a second small kernel and
 *   l2hmc_adapt_workspace_doubles(n) doubles (at most 1024).
 * l2hmc_adapt_finish: if t >= 1 then log_eps = log_eps_bar; phase = 2; *alpha = (float) log_eps.
 * L2HMC_ERR_ARG (before any launch): a NULL p (when reducing) / state / alpha (when applying), n < 1, a mode outside 1 .. 3,
 * one mode bit alone without sums2, n beyond the single-workgroup form without workspace; init: search not 0 / 1, target
 * outside (0, 1), gamma / t0 / kappa not positive, log_eps_min >= log_eps_max. */
#define L2HMC_ADAPT_STATE_DOUBLES 16
#define L2HMC_ADAPT_SINGLE_BLOCK_MAX 65536
enum { L2HMC_ADAPT_REDUCE = 1, L2HMC_ADAPT_APPLY = 2 };   /* mode bits; 3 = both in one launch */
int64_t l2hmc_adapt_workspace_doubles(int64_t n);
int l2hmc_adapt_init(double* state, const float* alpha, int32_t search, double target_accept, double gamma, double t0,
                     double kappa, double log_eps_min, double log_eps_max, void* stream);
int l2hmc_adapt_update(const float* p, int64_t n, int32_t mode, double* sums2, double* state, float* alpha, double* trace_row4,
                       double* workspace, void* stream);
int l2hmc_adapt_finish(double* state, float* alpha, void* stream);

/* Binding check.  The argument structs grow by trailing fields from one ABI version to the next (and
 * l2hmc_pack_nets' buffer by the lane layout: always size it with l2hmc_packed_nets_floats).  A binding built
 * against an older header would pass shorter structs, so besides comparing l2hmc_abi_version() with the
 * L2HMC_ABI_VERSION it was written for, a binding compares sizeof() of its own mirror of every struct with
 * what the library was compiled with (l2hmc_amd/_ffi.py does both when it loads the library).
 * which: one of L2HMC_STRUCT_*; returns sizeof in bytes, or L2HMC_ERR_ARG. */
enum { L2HMC_STRUCT_NET = 0, L2HMC_STRUCT_ENERGY = 1, L2HMC_STRUCT_TRAJECTORY_ARGS = 2, L2HMC_STRUCT_MLP3 = 3,
       L2HMC_STRUCT_SPLIT_ARGS = 4, L2HMC_STRUCT_TRAIN_ARGS = 5, L2HMC_STRUCT_TRAIN_SPLIT_ARGS = 6, L2HMC_STRUCT_TRAIN_STEP = 7,
       L2HMC_STRUCT_LADDER_ARGS = 8 };
int64_t l2hmc_struct_bytes(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* L2HMC_H_ */
