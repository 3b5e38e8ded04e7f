"""Shared by tests/test_probit_cpu.py, tests/test_gpu_probit_target.py, tests/test_gpu_probit_glm.py,
tests/test_gpu_probit_geometries.py and tools/probit_accuracy.py: seeded inputs of binomial regression with the probit link
(`l2hmc_amd.ProbitRegression`; L2HMC_ENERGY_PROBIT = 10, L2HMC_GLM_PROBIT = 6), a float64 restatement of the likelihood and the
energy written from the definition with scipy's log_ndtr (independent of l2hmc_amd), the float32 numpy restatement of the
device's operation sequence (ProbitLink, csrc/l2hmc_kernels.hpp), and the bounds of the device path, derived from the inputs.

A case is a dict {'kind': "probit", 'W' (S, d), 'X' (n, d), 'y' (n,), 'offset' (n,), 'trials' (n,), all float32}.  Definitions,
float64, with Phi the standard normal distribution function, phi its density and lam(t) = phi(t) / Phi(t):
    o = offset    m = trials    c = log C(m, y)    t = x_i . w + o_i
    lp = log Phi(t)    lq = log Phi(-t)    ll = y lp + (m - y) lq + c    mean = m Phi(t)
    term = -(y lp + (m - y) lq)    r = (m - y) lam(-t) - y lam(t)    U = sum_i term_i + |w|^2 / (2 s2)    g_k = sum_i x_ik r_i + w_k / s2

THE DEVICE SEQUENCE (`link32` restates it operation by operation; fl() is one float32 rounding), a = |t|:
    x = fl(a / sqrt 2)    u = rcp(x + 2)    s = (x - 2) u, one Newton step    E = fl(P(s) u)  ~ erfcx(x)    h = E / 2 (exact)
    a2 = fl((a / 2) a)    G = exp2(fl(a2 (-log2 e)))    Q = fl(h G) = Phi(-a)    w = fl(1 - Q)    rho = Q - (1 - w)    iw = rcp(w)
    log Phi(-a) = fl(fl(ln 2 log2 h) - a2)        log Phi(a) = fma(-rho, iw, fl(ln 2 log2 w))
    lam(-a) = fl(sqrt(2 / pi) rcp(E))             lam(a) = fl(fl(G / sqrt(2 pi)) iw)
    term = fma(-y, lp, fl((y - m) lq))    ll = fl(c - term)    r = fma(m - y, lam(-t), fl(-y lam(t)))    mean = fl(m Phi)
the pairs assigned to t and -t by the sign of t.

THE BOUNDS, with u = 2^-24 (glm_case.EPS) and A_si = sum_k |w_sk| |x_ik|.  y and m are integers up to 2^24 (exact, and so is
m - y); o and c are rounded once.
  t     as tests/binomial_case.py:                              dt = (d + 8) u A + u |o| + u |t|
        lam is decreasing with -1 < lam' < 0 and d log Phi / dt = lam: a moved t moves log Phi(+-t) by at most lam(+-t - dt) dt,
        lam(+-t) by at most dt and Phi by at most (phi(t) + dt / 4) dt.  What follows is the error at the device's own t.
  E     x = a / sqrt 2 is rounded and so is the constant: 2 u relative, and |x erfcx'(x) / erfcx(x)| < 1: 2 u of E.  The
        evaluation itself is within ERFCX_ULPS u of erfcx at the float32 x, MEASURED by tools/fit_erfcx.py on a dense grid with the
        reciprocal anywhere within one ulp (it enters the bounds as this one constant):   eE = (ERFCX_ULPS + 2) u
  a2    one rounding (the halving is exact):                    u a2
  G     the argument a2 (-log2 e): a2's rounding, the constant's, the product's: 3 u a2 log2 e absolute, 3 u a2 relative in G;
        the hardware exp2 within one ulp (2 u):                 eG = (3 a2 + 2) u, and an absolute 2^-126 where G underflows
  Q     one product:                                            eQ = eE + eG + u (relative), TINY = 2^-125 absolute
  log Phi(-a) = log h - a2: log h moves by eE; the hardware log2 is within one ulp of its result (2 u |log h|), ln 2 is rounded
        and so is the product (2 u |log h|), |log h| <= |lq| + a2; a2's rounding; the difference is rounded (u |lq|):
                                                                d_small = eE + 5 u (|log Phi(-a)| + a2)
  log Phi(a) = log(1 - Q): Q's error moves it by (Q / (1 - Q)) eQ.  w = fl(1 - Q) and rho = Q - (1 - w) are exact statements
        of 1 - Q = w - rho (Sterbenz twice), log(w - rho) = log w - rho / w up to (rho / w)^2, |rho| <= min(Q, u); log2, ln 2 and
        the product 4 u |log w|, the fma u |lp|; the reciprocal's 2 u acts on rho / w:
                                                                d_big = (Q / w) eQ + 5 u |log Phi(a)| + (rho / w)^2 + 2 u rho / w + TINY
  term  the product (m - y) lq is rounded, the fma once:        B_term = y D(lp) + (m - y) D(lq) + u (m - y) |lq| + u |term|
        with D(.) = the moved t's share plus d_big or d_small by the sign of t (the larger of the two where |t| <= 2 dt: the
        device may stand on the other side of 0)
  ll    c is rounded, ll = c - term is rounded:                 B = B_term + u (|c| + |ll|)
  lam(-a) = sqrt(2 / pi) / E: eE, the reciprocal's 2 u, the constant and the product:      e_small = eE + 4 u (relative)
  lam(a) = G / (sqrt(2 pi) w): eG, the constant and two products 3 u, w within (Q / w) eQ + u, the reciprocal 2 u:
                                                                e_big = eG + (Q / w) eQ + 6 u (relative), TINY absolute
  r     the product y lam(t) is rounded, the fma once:          B_r = (m - y) (dt + e lam(-t)) + y (dt + e lam(t)) + u y lam(t) + u |r|
  mean  Phi is w (within Q eQ + u w) or Q (within Q eQ), the product m Phi is rounded:
                                                                Bmean = m ((phi(t) + dt / 4) dt + Q eQ + u Phi + TINY) + u m Phi
  U     |dU|   <= sum_i B_term + n u sum_i |term_i| + (d + 8) u |w|^2 / (2 s2) + u |U|
  g     |dg_k| <= sum_i |x_ik| B_r,i + (n + 8) u sum_i |x_ik| |r_i| + 2 u |w_k| / s2 + u |g_k|
(the last two as tests/binomial_case.py states them).  Every bound is first order in u; the whole is multiplied by 1 + 2^-10 for
the products of two errors.  Temperature and the AIS bridge: `binomial_case.scaled`'s rules, restated in `scaled`.

Per row, as tests/glm_case.py: |d mean| <= mean_s Bmean, |d lppd_i| <= max_s B, |d mean ll| <= mean_s B, and p_waic_i's.

THE GATES OF THE FINISHED NUMBERS of PSIS-LOO are built as binomial_case.K_* are: K delta_i with delta_i = max_s B_si and K = 4 x
the worst sensitivity measured on the CPU between the float64 route and the float32 restatement `log_lik32` handed to the same
route (`sensitivity`; tools/probit_accuracy.py prints them, profiles/probit_accuracy.txt keeps the run).  The kernel is never the
yardstick."""
import numpy as np

from tests import binomial_case as bc
from tests import glm_case as gc

EPS = gc.EPS
TINY = 2.0 ** -125
SLOP = 1.0 + 2.0 ** -10
PRIOR_VAR = 2.0
TRIALS = (1, 1, 2, 5, 50)
# the worst relative error, in units of u = 2^-24, of the float32 erfcx sequence against scipy.special.erfcx in float64, with the
# reciprocal correctly rounded and moved one ulp either way: tools/fit_erfcx.py --degree 10 measured 5.415 at x = 29.5842 over
# np.linspace(0, 64, 4000001) (and 5.201 over 200001 logarithmic points of 64 .. 1e19); recorded with a margin for other grids
ERFCX_ULPS = 6.0
ERFCX_GRID = (0.0, 64.0, 4000001)
ERFCX_COEF = (8.274317224277183e-05, 7.457089668605477e-05, -0.0005954733933322132, -0.000864148314576596, 0.003056065645068884,
              0.006488782353699207, -0.021502695977687836, -0.036443788558244705, 0.27947142720222473, -0.6871606111526489,
              1.0215827226638794)

SHAPES = gc.SHAPES[:7]                  # (S, n, d) of the statistics tests: every geometry, ragged blocks, many chunks
GEOM_SHAPES = gc.SHAPES[7:]             # every feature-tile count 3, 5, 6, 7 of the compiled 4 / 8
LONG = bc.LONG                          # three rows beyond 131072 draws

# 4 x the worst sensitivity over SHAPES (tools/probit_accuracy.py; profiles/probit_accuracy.txt), each with the case where it occurred
# (a sensitivity is per unit of a row's own move, and this link's float32 ll is accurate RELATIVE to ll: a row whose ll hardly
# varies over the draws moves by 1e-12 and its Pareto fit, which is invariant to the scale of the ratios' spread, by 1e-7)
K_KHAT = 4 * 190200     # worst measured 190117, on (70, 33, 17)
K_ELPD = 4 * 0.73       # worst measured 0.7269, on (25, 1, 1)
K_NEFF = 4 * 1.84       # relative; worst measured 1.836, on (25, 1, 1)
K_MCSE = 4 * 28960      # relative; worst measured 28955, on (70, 33, 17)
K_REFF = 4 * 110.2      # relative, on the AR(1) history; worst measured 110.18

with_draws, rows_of, select_rows, used = bc.with_draws, bc.rows_of, bc.select_rows, bc.used
f32 = np.float32


def Phi(t):
    from scipy.special import ndtr
    return ndtr(t)


def log_Phi(t):
    from scipy.special import log_ndtr
    return log_ndtr(t)


def lam(t):
    """phi(t) / Phi(t), float64, finite in both tails."""
    t = np.asarray(t, dtype=np.float64)
    return np.exp(-0.5 * t * t - 0.5 * np.log(2.0 * np.pi) - log_Phi(t))


def case(S, n, d, seed=None):
    """The draws, rows and offsets of `glm_case.case` (max |x . w| = 3, offsets in [-1, 2]) with probit responses at the mean
    draw: trials drawn from TRIALS (1, small, 50), and from n = 3 on row 0 has y = 0 of 50, row 1 y = 1 of 1 and row 2 y = 50 of
    50 (n = 1: y = 0 of 50; n = 2: also 1 of 1)."""
    W, X, _, o = gc.case(S, n, d, seed=seed)
    rng = np.random.RandomState(177 + gc.seed_of(S, n, d) if seed is None else seed + 2)
    eta = X.astype(np.float64) @ W.astype(np.float64).mean(axis=0) + o
    m = rng.choice(TRIALS, size=n).astype(np.float64)
    for i, mi in enumerate((50.0, 1.0, 50.0)[:n]):
        m[i] = mi
    y = rng.binomial(m.astype(np.int64), Phi(eta)).astype(np.float64)
    for i, yi in enumerate((0.0, 1.0, 50.0)[:n]):
        y[i] = yi
    return {"kind": "probit", "W": W, "X": X, "offset": o, "y": y.astype(f32), "trials": m.astype(f32)}


def model(c, prior_var=1.0):
    import l2hmc_amd
    return l2hmc_amd.ProbitRegression(c["X"], c["y"], c["trials"], offset=c["offset"], prior_var=prior_var)


def terms(c):
    """(o, m, const) float64 of the definitions."""
    from scipy.special import gammaln
    y, m = c["y"].astype(np.float64), c["trials"].astype(np.float64)
    return c["offset"].astype(np.float64), m, gammaln(m + 1.0) - gammaln(y + 1.0) - gammaln(m - y + 1.0)


def saturated(c):
    """sat = y log(y / m) + (m - y) log(1 - y / m) + const, 0 log 0 = 0: the supremum of ll over t, at Phi(t) = y / m (the
    binomial's)."""
    from scipy.special import xlogy
    o, m, k = terms(c)
    y = c["y"].astype(np.float64)
    return xlogy(y, y / m) + xlogy(m - y, (m - y) / m) + k


def log_lik(c, W=None):
    """(ll, t) float64 (S, n) from the definition."""
    W = c["W"] if W is None else W
    o, m, k = terms(c)
    X, y = c["X"].astype(np.float64), c["y"].astype(np.float64)
    t = np.asarray(W, dtype=np.float64).reshape(-1, X.shape[1]) @ X.T + o
    return y * log_Phi(t) + (m - y) * log_Phi(-t) + k, t


def mean_of(c, t):
    return terms(c)[1] * Phi(t)


# ---- the device sequence in float32 numpy ---------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64 (one double rounding in about 2^-29 of the cases)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def erfcx32(x, nudge=0):
    """ProbitLink's erfcx of float32 x >= 0; `nudge` moves the reciprocal by that many ulps (tools/fit_erfcx.py's measurement)."""
    x = np.asarray(x, dtype=f32)
    u = (f32(1.0) / (x + f32(2.0))).astype(f32)
    if nudge:
        u = np.nextafter(u, f32(np.inf if nudge > 0 else -np.inf)).astype(f32)
    s = ((x - f32(2.0)) * u).astype(f32)
    e = fma32(s + f32(1.0), f32(-2.0), x)
    e = fma32(s, -x, e)
    s = fma32(u, e, s)
    p = np.full(x.shape, f32(ERFCX_COEF[0]), dtype=f32)
    for co in ERFCX_COEF[1:]:
        p = fma32(p, s, f32(co))
    return (p * u).astype(f32)


def link32(t, y, m):
    """{'lp', 'lq', 'lam_t', 'lam_nt', 'Phi', 'term', 'r'} float32 of float32 t (S, n), y and m (n,): ProbitLink, operation by
    operation."""
    with np.errstate(all="ignore"):
        t = np.asarray(t, dtype=f32)
        a = np.abs(t)
        E = erfcx32((a * f32(0.7071067811865476)).astype(f32))
        a2 = ((f32(0.5) * a) * a).astype(f32)
        G = np.exp2((a2 * f32(-1.4426950408889634)).astype(f32)).astype(f32)
        Q = ((f32(0.5) * E) * G).astype(f32)
        w = (f32(1.0) - Q).astype(f32)
        iw = (f32(1.0) / w).astype(f32)
        ln2 = f32(0.6931471805599453)
        l_small = ((ln2 * np.log2((f32(0.5) * E).astype(f32)).astype(f32)).astype(f32) - a2).astype(f32)
        rho = (Q - (f32(1.0) - w).astype(f32)).astype(f32)
        l_big = fma32(-rho, iw, (ln2 * np.log2(w).astype(f32)).astype(f32))
        lam_small = (f32(0.7978845608028654) * (f32(1.0) / E).astype(f32)).astype(f32)
        lam_big = ((G * f32(0.3989422804014327)).astype(f32) * iw).astype(f32)
        pos = t >= 0
        lp, lq = np.where(pos, l_big, l_small), np.where(pos, l_small, l_big)
        lam_t, lam_nt = np.where(pos, lam_big, lam_small), np.where(pos, lam_small, lam_big)
        y, m = np.asarray(y, dtype=f32), np.asarray(m, dtype=f32)
        term = fma32(-y, lp, ((y - m) * lq).astype(f32))
        r = fma32(m - y, lam_nt, (-y * lam_t).astype(f32))
        return {"lp": lp, "lq": lq, "lam_t": lam_t, "lam_nt": lam_nt, "Phi": np.where(pos, w, Q), "term": term, "r": r}


def log_lik32(c, W=None):
    """The float32 numpy restatement: o and const rounded once, every operation in float32, in the device's sequence."""
    W = c["W"] if W is None else W
    o, m, k = (np.asarray(a, dtype=f32) for a in terms(c))
    X = c["X"]
    t = (np.asarray(W, dtype=f32).reshape(-1, X.shape[1]) @ X.T + o).astype(f32)
    return (-link32(t, c["y"], m)["term"] + k).astype(f32)


def energy(c, W=None, s2=PRIOR_VAR, dtype=np.float64):
    """(U (N,), grad U (N, d)): from the definition in float64, or the device sequence in float32 (o rounded once)."""
    W = c["W"] if W is None else W
    o, m, _ = (np.asarray(a, dtype=dtype) for a in terms(c))
    W, X, y = (np.asarray(a, dtype=dtype) for a in (W, c["X"], c["y"]))
    t = W @ X.T + o
    if dtype == np.float64:
        term = -(y * log_Phi(t) + (m - y) * log_Phi(-t))
        r = (m - y) * lam(-t) - y * lam(t)
    else:
        L = link32(t, y, m)
        term, r = L["term"], L["r"]
    U = term.sum(axis=1) + dtype(0.5) * (W * W).sum(axis=1) / dtype(s2)
    G = r @ X + W / dtype(s2)
    return U.astype(dtype), G.astype(dtype)


def oracle_energy(c, s2=PRIOR_VAR, dtype=np.float32):
    """x -> (U, grad U) in `dtype`: the energy of `oracle.l2hmc_oracle.Dynamics`."""
    return lambda W: energy(c, W, s2, dtype)


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
def _pieces(c, W):
    W = c["W"] if W is None else W
    ll, t = log_lik(c, W)
    o, m, k = terms(c)
    X64, y = c["X"].astype(np.float64), c["y"].astype(np.float64)
    W64 = np.asarray(W, dtype=np.float64).reshape(-1, X64.shape[1])
    d = X64.shape[1]
    A = np.abs(W64) @ np.abs(X64).T
    dt = (d + 8) * EPS * A + EPS * np.abs(o) + EPS * np.abs(t)
    a = np.abs(t)
    a2 = 0.5 * a * a
    l_small, l_big = log_Phi(-a), log_Phi(a)
    Q = Phi(-a)
    w = 1.0 - Q                                                 # in [1/2, 1]
    eE = (ERFCX_ULPS + 2) * EPS
    eG = (3 * a2 + 2) * EPS
    eQ = eE + eG + EPS
    d_small = eE + 5 * EPS * (np.abs(l_small) + a2)
    rho = np.minimum(Q, EPS) / w                                # |rho| / w: rho is Q itself where w = 1, else a rounding of w
    d_big = (Q / w) * eQ + 5 * EPS * np.abs(l_big) + rho * rho + 2 * EPS * rho + TINY
    e_small = eE + 4 * EPS
    e_big = eG + (Q / w) * eQ + 6 * EPS
    pos, near = t >= 0, a <= 2 * dt
    worst = np.maximum(d_small, d_big)
    d_lp = np.where(near, worst, np.where(pos, d_big, d_small))
    d_lq = np.where(near, worst, np.where(pos, d_small, d_big))
    lam_t, lam_nt = lam(t), lam(-t)
    lam_small, lam_big = lam(-a), lam(a)
    ab_small, ab_big = e_small * lam_small, e_big * lam_big + TINY        # absolute errors of lam(-a), lam(a)
    ab_worst = np.maximum(ab_small, ab_big)
    d_lam_t = np.where(near, ab_worst, np.where(pos, ab_big, ab_small))
    d_lam_nt = np.where(near, ab_worst, np.where(pos, ab_small, ab_big))
    lp, lq = log_Phi(t), log_Phi(-t)
    D_lp = lam(t - dt) * dt + d_lp
    D_lq = lam(-t - dt) * dt + d_lq
    term, r = -(y * lp + (m - y) * lq), (m - y) * lam_nt - y * lam_t
    Bterm = SLOP * (y * D_lp + (m - y) * D_lq + EPS * (m - y) * np.abs(lq) + EPS * np.abs(term))
    Br = SLOP * ((m - y) * (dt + d_lam_nt) + y * (dt + d_lam_t) + EPS * y * lam_t + EPS * np.abs(r))
    P = Phi(t)
    phi = np.exp(-a2) / np.sqrt(2.0 * np.pi)
    Bmean = SLOP * (m * ((phi + dt / 4) * dt + Q * eQ + EPS * P + TINY) + EPS * m * P)
    return {"ll": ll, "t": t, "o": o, "m": m, "k": k, "dt": dt, "term": term, "r": r, "Bterm": Bterm, "Br": Br, "Bmean": Bmean,
            "W64": W64, "X64": X64, "y": y}


def ll_bounds(c, W=None):
    """{'B', 'Bmean' (S, n), 'delta' (n,), 'mean_mu', 'lppd_i', 'mean_ll', 'p_waic_i' (n,)} of the module docstring."""
    p = _pieces(c, W)
    ll = p["ll"]
    S = ll.shape[0]
    B = p["Bterm"] + EPS * (np.abs(p["k"]) + np.abs(ll))
    Bmax, sd = B.max(axis=0), ll.std(axis=0)
    return {"B": B, "Bmean": p["Bmean"], "delta": Bmax, "mean_mu": p["Bmean"].mean(axis=0), "lppd_i": Bmax, "mean_ll": B.mean(axis=0),
            "p_waic_i": (2 * sd * Bmax + Bmax ** 2) * S / max(S - 1, 1) + 4 * S * 2.0 ** -52 * (ll * ll).mean(axis=0)}


def restatement(c, W=None):
    """The predictive numbers per row, float64, from the definitions."""
    from scipy.special import logsumexp
    ll, t = log_lik(c, W)
    S = ll.shape[0]
    out = {"mean_mu": mean_of(c, t).mean(axis=0), "lppd_i": logsumexp(ll, axis=0) - np.log(S), "p_waic_i": ll.var(axis=0, ddof=1),
           "mean_ll": ll.mean(axis=0)}
    out["elpd_i"] = out["lppd_i"] - out["p_waic_i"]
    return out


def bounds(c, W=None, s2=PRIOR_VAR):
    """{'U' (N,), 'g' (N, d)}: the bounds of the module docstring."""
    p = _pieces(c, W)
    W64, X64 = p["W64"], p["X64"]
    n, d = X64.shape
    U, G = energy(c, W64, s2)
    w2 = (W64 * W64).sum(axis=1)
    bU = p["Bterm"].sum(axis=1) + n * EPS * np.abs(p["term"]).sum(axis=1) + (d + 8) * EPS * w2 / (2 * s2) + EPS * np.abs(U)
    aX = np.abs(X64)
    bg = p["Br"] @ aX + (n + 8) * EPS * (np.abs(p["r"]) @ aX) + 2 * EPS * np.abs(W64) / s2 + EPS * np.abs(G)
    return {"U": bU, "g": bg}


def scaled(c, W=None, s2=PRIOR_VAR, temperature=1.0, beta=1.0):
    """(U, g, bounds) float64 of the tempered / bridged energy and its bounds: `binomial_case.scaled`'s rules."""
    W = c["W"] if W is None else W
    U, G = energy(c, W, s2)
    b = bounds(c, W, s2)
    bU, bg = b["U"], b["g"]
    W64 = np.asarray(W, dtype=np.float64)
    d = W64.shape[1]
    if beta != 1.0:
        q = 0.5 * (W64 * W64).sum(axis=1)
        bU = beta * bU + (d + 8) * EPS * (1 - beta) * q + 4 * EPS * ((1 - beta) * q + beta * np.abs(U))
        bg = beta * bg + 4 * EPS * ((1 - beta) * np.abs(W64) + beta * np.abs(G))
        U, G = (1 - beta) * q + beta * U, (1 - beta) * W64 + beta * G
    if temperature != 1.0:
        U, G = U / temperature, G / temperature
        bU, bg = bU / temperature + EPS * np.abs(U), bg / temperature + EPS * np.abs(G)
    return U, G, {"U": bU, "g": bg}


# ---- the tails ------------------------------------------------------------------------------------------------------------------
EDGE_TAUS = (0.0, 5.0, -5.0, 9.0, -9.0, 15.0, -15.0, 30.0, -30.0)
EDGE_YS = (0.0, 50.0, 23.0)             # y = 0, y = m and 0 < y < m at m = 50
EDGE_N = len(EDGE_TAUS) * len(EDGE_YS)


def edge_case(S=70):
    """EDGE: 27 rows, d = 3, m = 50: the rows of `glm_case.case(S, 27, 3)` scaled to |x . w| <= 0.3 with offsets that put t near
    0, +-5, +-9, +-15 and +-30, each with y = 0, y = 50 and y = 23 -- the tails where 0.5 erfc followed by a log returns -inf
    (t = -15: Phi = 4e-51; t = -30: 5e-198, ll = -22716 at y = 50) and where 1 - Phi returns 0 (t = +9 on).  Row 3 j + k has
    tau = EDGE_TAUS[j], y = EDGE_YS[k]; two 16-row blocks, the second ragged."""
    W, X, _, _ = gc.case(S, EDGE_N, 3)
    tau = np.repeat(np.asarray(EDGE_TAUS), len(EDGE_YS))
    y = np.tile(np.asarray(EDGE_YS), len(EDGE_TAUS))
    return {"kind": "probit", "W": W, "X": (0.1 * X).astype(f32), "offset": tau.astype(f32), "y": y.astype(f32),
            "trials": np.full(EDGE_N, 50.0, dtype=f32)}


EDGE = edge_case()


# ---- sensitivities of the finished numbers (CPU) -------------------------------------------------------------------------------
def sensitivity(c):
    """(K_khat, K_elpd, K_neff, K_mcse) of one case: `binomial_case.sensitivity` with this module's two restatements."""
    from l2hmc_amd import psis
    from tests import loglik_case as lk
    ll, _ = log_lik(c)
    ll32 = log_lik32(c).astype(np.float64)
    move = np.abs(ll32 - ll).max(axis=0)
    r = lk.r_eff_for(ll.shape[1])
    ref, got = psis.loo_from_log_lik(ll, r_eff=r), psis.loo_from_log_lik(ll32, r_eff=r)
    ok = move > 0
    both = np.isfinite(ref.khat) & np.isfinite(got.khat) & ok
    with np.errstate(all="ignore"):
        return (float(np.max((np.abs(got.khat - ref.khat) / move)[both])) if both.any() else 0.0,
                float(np.max((np.abs(got.elpd_loo_i - ref.elpd_loo_i) / move)[ok])) if ok.any() else 0.0,
                float(np.max((gc.rel(got.n_eff, ref.n_eff) / move)[both])) if both.any() else 0.0,
                float(np.max((gc.rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / move)[both])) if both.any() else 0.0)


def ar1_case():
    """The AR(1) history of `glm_case.ar1_case` (steps, chains, d) with probit responses."""
    W, X, _, o = gc.ar1_case()
    rng = np.random.RandomState(9102)
    n, d = X.shape
    eta = X.astype(np.float64) @ W.reshape(-1, d).astype(np.float64).mean(axis=0) + o
    m = rng.choice(TRIALS, size=n).astype(np.float64)
    return {"kind": "probit", "W": W, "X": X, "offset": o, "y": rng.binomial(m.astype(np.int64), Phi(eta)).astype(f32),
            "trials": m.astype(f32)}


def reff_sensitivity(c):
    """The relative change of r_eff_i per unit of change of row i's ll, float32 restatement against float64, at its worst row,
    on the AR(1) history."""
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split, n = gc.AR1
    ll, _ = log_lik(c)
    ll32 = log_lik32(c).astype(np.float64)
    move = np.abs(ll32 - ll).max(axis=0)
    ref = psis.relative_eff_from_log_lik(ll.reshape(M, N, n), max_lag=max_lag, split=split)
    got = psis.relative_eff_from_log_lik(ll32.reshape(M, N, n), max_lag=max_lag, split=split)
    return float(np.max((gc.rel(got.r_eff, ref.r_eff) / move)[move > 0]))


# ---- trajectories against the oracle --------------------------------------------------------------------------------------------
TRAJ_SHAPES = [(17, 5), (200, 25), (300, 100)]
TRAJ_CASES = [(n, d, H) for (n, d) in TRAJ_SHAPES for H in (0, 10)] + [(200, 25, 24)]
_TRAJ = {}


def oracle_dynamics(g, c, hmc, eps, dtype=np.float32, temperature=1.0, T=None):
    from oracle import l2hmc_oracle as O
    xn = vn = None
    if not hmc:
        xn, vn = ({k: g[p + k] for k in O.NET_KEYS} for p in ("xnet.", "vnet."))
    return O.Dynamics(int(g["x_dim"]), oracle_energy(c, PRIOR_VAR, dtype), int(g["T"]) if T is None else T, eps, g["mask"],
                      xn, vn, temperature=temperature, dtype=dtype)


def traj_case(n, d, H):
    """`binomial_case.traj_case` for this likelihood, computed once: the synthetic nets and mask `g`, the case `c` (its draws
    are the start x), v, the step size chosen on the float32 oracle (the first of 0.1, 0.05, ... with a mean accept probability
    in (0.2, 1)), the oracle's results in float32 (`ref`) and their distance from the same oracle in float64 (`dist`)."""
    from tests import helpers
    from tests import poisson_target_case as pc
    key = (n, d, H)
    if key in _TRAJ:
        return _TRAJ[key]
    hmc = H == 0
    g = helpers.synthetic_case("gauss_diag", d, H=max(H, 1), T=pc.TRAJ_T, N=pc.TRAJ_N, seed=d, eps=0.1)
    c = case(pc.TRAJ_N, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(pc.TRAJ_N, d).astype(f32)
    eps = pc.choose_eps(lambda e: oracle_dynamics(g, c, hmc, e), x, v)

    def run(dtype):
        od = oracle_dynamics(g, c, hmc, eps, dtype)
        xx, vv = x.astype(dtype), v.astype(dtype)
        out = {}
        for s in (0, 3):
            out["fwd%d" % s] = od.forward_step(xx, vv, s)
            out["bwd%d" % s] = od.backward_step(xx, vv, s)
        X1, V1, lj = od.forward(xx, vv, log_jac=True)
        out["forward"] = (X1, V1, lj, od.forward(xx, vv)[2])
        return out
    ref, r64 = run(np.float32), run(np.float64)
    dist = {k: tuple((pc.abs_err if (k == "forward" and i == 3) else pc.rel_err)(a, b) for i, (a, b) in enumerate(zip(ref[k], r64[k])))
            for k in ref}
    _TRAJ[key] = {"g": g, "c": c, "x": x, "v": v, "eps": eps, "hmc": hmc, "ref": ref, "dist": dist}
    return _TRAJ[key]


# ---- the posterior mean ------------------------------------------------------------------------------------------------------------
def wide_is_mean(c, s2=PRIOR_VAR, n_draws=400000, seed=0, chunk=10000, widen=1.5):
    """The posterior mean by self-normalised importance sampling from a WIDE Gaussian -- the Laplace approximation at the mode
    (Newton on U; the Hessian is X^T diag(y lam(t) (t + lam(t)) + (m - y) lam(-t) (lam(-t) - t)) X + I / s2) with its standard
    deviations multiplied by `widen` -- in antithetic pairs, float64: (mean, its standard error from the weights, mode, Cholesky
    factor of the Laplace covariance)."""
    o, m, _ = terms(c)
    X, y = c["X"].astype(np.float64), c["y"].astype(np.float64)
    d = X.shape[1]
    w = np.zeros(d)
    for _ in range(200):
        t = X @ w + o
        lt, ln = lam(t), lam(-t)
        gr = X.T @ ((m - y) * ln - y * lt) + w / s2
        Hs = (X * (y * lt * (t + lt) + (m - y) * ln * (ln - t))[:, None]).T @ X + np.eye(d) / s2
        step = np.linalg.solve(Hs, gr)
        w = w - step / max(1.0, np.abs(step).max())
        if np.abs(step).max() < 1e-13:
            break
    Lc = np.linalg.cholesky(np.linalg.inv(Hs))
    Z = np.random.RandomState(seed).randn(n_draws // 2, d)
    Z = np.concatenate([Z, -Z])
    Wd = w + widen * (Z @ Lc.T)
    U = np.concatenate([energy(c, Wd[i:i + chunk], s2)[0] for i in range(0, len(Wd), chunk)])
    lw = -U + 0.5 * np.square(Z).sum(axis=1)
    wt = np.exp(lw - lw.max())
    wt /= wt.sum()
    mean = (wt[:, None] * Wd).sum(axis=0)
    se = np.sqrt((np.square(wt)[:, None] * np.square(Wd - mean)).sum(axis=0))
    return mean, se, w, Lc


# ---- the device entries, straight (need a GPU) ---------------------------------------------------------------------------------
def device_raw(c, W=None, lens=None, rows=None):
    """`binomial_case.device_raw` for this likelihood: the three entries straight through `_ffi` on the rows `rows` = (first,
    stop) of the case under the draws W, every output filled with NaN / -7 and GUARD elements longer than the entry is told."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd._history import in_place, launch, workspace
    W = c["W"] if W is None else W
    Wd = in_place(W if hasattr(W, "is_cuda") else torch.as_tensor(np.ascontiguousarray(W, dtype=f32)).cuda())
    S, d = int(Wd.shape[0]), int(Wd.shape[1])
    a, stop = (0, c["X"].shape[0]) if rows is None else rows
    m = stop - a
    dev, L = Wd.device, _ffi.lib()
    g = model(c)._glm
    packed, consts = g._device_data(dev)(a, m)
    assert tuple(consts.shape) == (4, m) and g.family == _ffi.GLM_PROBIT
    group = None if lens is None else np.ascontiguousarray(lens[a:stop], dtype=np.int64)
    stride = gc.tail_len(S) if group is None else int(group.max())
    lens_d = None if group is None else torch.as_tensor(group).to(dev)
    G = gc.GUARD

    def out(count, dtype):
        return torch.full((count + G,), -7 if dtype == torch.int64 else float("nan"), dtype=dtype, device=dev)
    buf = {"ll": out(S * m, torch.float32), "cutoff": out(m, torch.float32), "top": out(m, torch.float32),
           "n_tail": out(m, torch.int64), "tail": out(m * stride, torch.float32), "sums": out(3 * m, torch.float64),
           "psums": out(4 * m, torch.float64)}
    fam = g.family
    launch(dev, L.l2hmc_glm_log_lik, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam, buf["ll"].data_ptr())
    ws = workspace(dev, torch.uint8, L.l2hmc_glm_loo_workspace_bytes, S, m, d)
    launch(dev, L.l2hmc_glm_loo_tails, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam,
           None if lens_d is None else lens_d.data_ptr(), stride, buf["cutoff"].data_ptr(), buf["top"].data_ptr(),
           buf["n_tail"].data_ptr(), buf["tail"].data_ptr() if stride else None, buf["sums"].data_ptr(), ws.data_ptr())
    wp = workspace(dev, torch.float64, L.l2hmc_glm_predict_workspace_doubles, S, m, d)
    launch(dev, L.l2hmc_glm_predict, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam, buf["psums"].data_ptr(),
           wp.data_ptr())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    shapes = {"ll": (S, m), "cutoff": (m,), "top": (m,), "n_tail": (m,), "tail": (m, stride), "sums": (3, m), "psums": (4, m)}
    res = {k: host[k][:-G].reshape(shapes[k]) for k in host}
    res["guards"] = {k: host[k][-G:] for k in host}
    res["flag"] = np.array([int(ws[:8].view(torch.int64)[0])])
    return res
