"""Shared by tests/test_binomial_cpu.py, tests/test_gpu_binomial_target.py, tests/test_gpu_binomial_glm.py,
tests/test_gpu_binomial_geometries.py and tools/binomial_accuracy.py: seeded inputs of the binomial and negative-binomial regressions (`l2hmc_amd.BinomialRegression`,
`NegativeBinomialRegression`; L2HMC_ENERGY_BINOMIAL, L2HMC_GLM_BINOMIAL / L2HMC_GLM_NEGBINOMIAL), a float64 restatement of the
likelihood and the energy written from the definition with scipy's gammaln (independent of l2hmc_amd), the same statement in
float32 numpy, and the bounds of the device path, derived from the inputs.

A case is a dict {'kind': "binomial" | "negbinomial", 'W' (S, d), 'X' (n, d), 'y' (n,), 'offset' (n,) float32, and 'trials' (n,)
float32 or 'phi'}.  Definitions (`terms`), all float64:
    binomial      o = offset              m = trials      c = log C(m, y)
    negbinomial   o = offset - log phi    m = y + phi     c = gammaln(y + phi) - gammaln(phi) - gammaln(y + 1)
    t = x_i . w + o_i      sp = softplus(t)      s = sigmoid(t)
    ll = y t - m sp + c    mean = m s (binomial), phi exp(t) = exp(x . w + offset) (negbinomial)
    term = m sp - y t      r = m s - y           U = sum_i term_i + |w|^2 / (2 s2)      g_k = sum_i x_ik r_i + w_k / s2

THE BOUNDS, with u = 2^-24 (glm_case.EPS) and A_si = sum_k |w_sk| |x_ik|.  The device holds o, m and c as float32, each rounded
once from its float64 value, and forms every value by individually rounded float32 operations (BinomialLink, l2hmc_kernels.hpp):
  t     the float32 contraction is within (d + 8) u A of the exact eta (tests/predictive_case.py); o is rounded (u |o|), the sum
        is rounded (u |t|):                                       dt = (d + 8) u A + u |o| + u |t|
  sp    softplus is 1-Lipschitz: the moved t costs dt.  e = exp(-|t|) as exp2(-|t| log2 e): the product's rounding moves e by
        u |t| e, the hardware exp2 by 2 u e (one ulp), and (|t| + 2) e^-|t| <= 2: |de| <= 2 u.  1 + e in [1, 2] is rounded: 2 u.
        log is 1-Lipschitz on [1, 2]: 4 u so far.  The hardware log2 of a value in [1, 2] is within one ulp of a result in
        [0, 1]: 2 u, times ln 2; the product with ln 2 is rounded: u ln 2: the log term is within 4 u + 3 u ln 2 < 8 u.  The
        last sum max(t, 0) + log term is rounded: u sp:           dsp = dt + 8 u + u sp
  term  m is rounded (u m sp), the product m sp is rounded (u m sp), the fused -y t + (m sp) moves by y dt and is rounded once
        (u |term|):                                               B_term = (m + y) dt + u (8 m + 3 m sp + |term|)
  ll    c is rounded (u |c|), ll = c - term is rounded (u |ll|):   B = B_term + u (|c| + |ll|)
  s     sigmoid is 1/4-Lipschitz.  inv = rcp(1 + e): 1 + e is within 4 u (relative, as 1 + e >= 1), the hardware reciprocal
        within one ulp (2 u): 6 u; below 0, e inv adds e's (|t| + 2) u and one rounding:   ds = dt / 4 + u (|t| + 9) s
  r     m is rounded (u m s), the fma is rounded once (u |r|):     B_r = m ds + u m s + u |r|
  mean  binomial: m s, one product:                               Bmean = m ds + 2 u m s
        negbinomial: phi exp(t), glm_case's Bmu with t for h:      Bmean = mu e^dt dt + 4 u mu (2 + |t|)
  U     |dU|   <= sum_i B_term + n u sum_i |term_i| + (d + 8) u |w|^2 / (2 s2) + u |U|
  g     |dg_k| <= sum_i |x_ik| B_r,i + (n + 8) u sum_i |x_ik| |r_i| + 2 u |w_k| / s2 + u |g_k|
(the last two as tests/poisson_target_case.py derives them: the n-term sums in any order, the eight extra roundings of the
cross-wave sum, the prior's d-term sum, its quotient and product, the last addition).  Temperature and the AIS bridge:
`poisson_target_case.scaled`'s rules, restated in `scaled`.  The absolute bound on ll grows like u m |t|: what the float32
likelihood loses at many trials is in the bound, not hidden from it.

Per row, as tests/glm_case.py: |d mean| <= mean_s Bmean, |d lppd_i| <= max_s B, |d mean ll| <= mean_s B, and p_waic_i's.

THE GATES OF THE FINISHED NUMBERS of PSIS-LOO, built as glm_case.K_* are: K delta_i with delta_i = max_s B_si (order
statistics are 1-Lipschitz in the sup norm) and K = 4 x the worst sensitivity measured on the CPU.  A sensitivity is the change
of a row's finished number per unit of change of that row's ll in the sup norm.  glm_case moves the float64 matrix by +-B_si,
a move of delta_i; here the move is the one between the float64 route and the float32 numpy restatement `log_lik32` handed to
the same route, so a row's sensitivity is |finished(ll32)_i - finished(ll64)_i| / max_s |ll32_si - ll64_si| (`sensitivity`;
tools/binomial_accuracy.py prints them, profiles/binomial_accuracy.txt keeps the run).  A finished number of row i reads
column i of the matrix alone, so the ratio is a row's own.  The kernel is never the yardstick."""
import numpy as np

from tests import glm_case as gc

EPS = gc.EPS
PRIOR_VAR = 2.0
TRIALS = (1, 1, 2, 5, 50)
NB_PHIS = (0.5, 10.0)

# (S, n, d) of the statistics tests: the first seven of glm_case.SHAPES (every geometry, ragged blocks, many chunks)
SHAPES = gc.SHAPES[:7]
NB_SHAPES = [(70, 33, 17), (4099, 100, 25)]
STAT_CASES = [("binomial", None) + s for s in SHAPES] + [("negbinomial", phi) + s for s in NB_SHAPES for phi in NB_PHIS]

# 4 x the worst sensitivity over STAT_CASES (tools/binomial_accuracy.py; profiles/binomial_accuracy.txt), each with the case
# where it occurred
K_KHAT = 4 * 384        # worst measured 383.7, binomial on (4099, 100, 25)
K_ELPD = 4 * 0.52       # worst measured 0.5162, binomial on (25, 3, 2)
K_NEFF = 4 * 0.79       # relative; worst measured 0.7888, binomial on (25, 1, 1)
K_MCSE = 4 * 15.8       # relative; worst measured 15.76, negative binomial phi = 0.5 on (70, 33, 17)
K_REFF = 4 * 7.35       # relative, on the AR(1) history; worst measured 7.349, negative binomial phi = 0.5


def case(S, n, d, kind="binomial", phi=None, seed=None):
    """The draws, rows and offsets of `glm_case.case` (max |x . w| = 3, offsets in [-1, 2]) with responses of this likelihood
    at the mean draw.  binomial: trials drawn from TRIALS (1, small, 50), and from n = 3 on row 0 has y = 0 of 50, row 1 y = 1 of
    1 and row 2 y = 50 of 50 (n = 1: y = 0 of 50; n = 2: also 1 of 1).  negbinomial: y ~ NB2(mean exp(x . w + o), phi), row 0
    has y = 0 and the last row is a surprising ceil(3 mu + 5)."""
    W, X, _, o = gc.case(S, n, d, seed=seed)
    rng = np.random.RandomState(77 + gc.seed_of(S, n, d) if seed is None else seed + 1)
    eta = X.astype(np.float64) @ W.astype(np.float64).mean(axis=0) + o
    out = {"kind": kind, "W": W, "X": X, "offset": o}
    if kind == "binomial":
        m = rng.choice(TRIALS, size=n).astype(np.float64)
        for i, mi in enumerate((50.0, 1.0, 50.0)[:n]):
            m[i] = mi
        y = rng.binomial(m.astype(np.int64), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        for i, yi in enumerate((0.0, 1.0, 50.0)[:n]):
            y[i] = yi
        out.update(y=y.astype(np.float32), trials=m.astype(np.float32))
    else:
        mu = np.exp(eta)
        y = rng.negative_binomial(phi, phi / (phi + mu)).astype(np.float64)
        y[-1] = np.ceil(3.0 * mu[-1] + 5.0)
        y[0] = 0.0
        out.update(y=y.astype(np.float32), phi=float(phi))
    return out


def with_draws(c, W):
    out = dict(c)
    out["W"] = W
    return out


def rows_of(c, a, b):
    """The case restricted to the data rows [a, b)."""
    out = dict(c)
    for k in ("X", "y", "offset", "trials"):
        if k in out:
            out[k] = out[k][a:b]
    return out


def model(c, prior_var=1.0):
    import l2hmc_amd
    if c["kind"] == "binomial":
        return l2hmc_amd.BinomialRegression(c["X"], c["y"], c["trials"], offset=c["offset"], prior_var=prior_var)
    return l2hmc_amd.NegativeBinomialRegression(c["X"], c["y"], c["phi"], offset=c["offset"], prior_var=prior_var)


def terms(c):
    """(o, m, const) float64 of the definitions."""
    from scipy.special import gammaln
    y, off = c["y"].astype(np.float64), c["offset"].astype(np.float64)
    if c["kind"] == "binomial":
        m = c["trials"].astype(np.float64)
        return off, m, gammaln(m + 1.0) - gammaln(y + 1.0) - gammaln(m - y + 1.0)
    phi = c["phi"]
    return off - np.log(phi), y + phi, gammaln(y + phi) - gammaln(phi) - gammaln(y + 1.0)


def softplus(t):
    return np.logaddexp(0.0, t)


def sigmoid(t):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-t))


def saturated(c):
    """sat = y log(y / m) + (m - y) log(1 - y / m) + const, 0 log 0 = 0: the supremum of ll over t."""
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
    return y * t - m * softplus(t) + k, t


def mean_of(c, t):
    o, m, _ = terms(c)
    return m * sigmoid(t) if c["kind"] == "binomial" else c["phi"] * np.exp(t)


def log_lik32(c, W=None):
    """The float32 numpy restatement: o, m and const rounded once, every operation in float32."""
    W = c["W"] if W is None else W
    o, m, k = (np.asarray(a, dtype=np.float32) for a in terms(c))
    X, y = c["X"], c["y"]
    t = np.asarray(W, dtype=np.float32).reshape(-1, X.shape[1]) @ X.T + o
    return y * t - m * softplus(t).astype(np.float32) + k


def energy(c, W=None, s2=PRIOR_VAR, dtype=np.float64):
    """(U (N,), grad U (N, d)) from the definition, every operation in `dtype` (float32: o and m rounded once)."""
    W = c["W"] if W is None else W
    o, m, _ = (np.asarray(a, dtype=dtype) for a in terms(c))
    W, X, y = (np.asarray(a, dtype=dtype) for a in (W, c["X"], c["y"]))
    t = W @ X.T + o
    U = (m * softplus(t).astype(dtype) - y * t).sum(axis=1) + dtype(0.5) * (W * W).sum(axis=1) / dtype(s2)
    G = (m * sigmoid(t).astype(dtype) - y) @ X + W / dtype(s2)
    return U.astype(dtype), G.astype(dtype)


def oracle_energy(c, s2=PRIOR_VAR, dtype=np.float32):
    """x -> (U, grad U) in `dtype`: the energy of `oracle.l2hmc_oracle.Dynamics`."""
    return lambda W: energy(c, W, s2, dtype)


def _pieces(c, W):
    W = c["W"] if W is None else W
    ll, t = log_lik(c, W)
    o, m, k = terms(c)
    X64, y = c["X"].astype(np.float64), c["y"].astype(np.float64)
    W64 = np.asarray(W, dtype=np.float64).reshape(-1, X64.shape[1])
    d = X64.shape[1]
    A = np.abs(W64) @ np.abs(X64).T
    dt = (d + 8) * EPS * A + EPS * np.abs(o) + EPS * np.abs(t)
    sp, s = softplus(t), sigmoid(t)
    term, r = m * sp - y * t, m * s - y
    Bterm = (m + y) * dt + EPS * (8 * m + 3 * m * sp + np.abs(term))
    ds = dt / 4 + EPS * (np.abs(t) + 9) * s
    Br = m * ds + EPS * m * s + EPS * np.abs(r)
    return {"ll": ll, "t": t, "o": o, "m": m, "k": k, "dt": dt, "sp": sp, "s": s, "term": term, "r": r, "Bterm": Bterm, "ds": ds,
            "Br": Br, "W64": W64, "X64": X64, "y": y}


def ll_bounds(c, W=None):
    """{'B', 'Bmean' (S, n), 'delta' (n,), 'mean_mu', 'lppd_i', 'mean_ll', 'p_waic_i' (n,)} of the module docstring."""
    p = _pieces(c, W)
    ll, t, m, dt = p["ll"], p["t"], p["m"], p["dt"]
    S = ll.shape[0]
    B = p["Bterm"] + EPS * (np.abs(p["k"]) + np.abs(ll))
    if c["kind"] == "binomial":
        Bmean = m * p["ds"] + 2 * EPS * m * p["s"]
    else:
        mu = c["phi"] * np.exp(t)
        Bmean = mu * np.exp(dt) * dt + 4 * EPS * mu * (2 + np.abs(t))
    Bmax, sd = B.max(axis=0), ll.std(axis=0)
    return {"B": B, "Bmean": Bmean, "delta": Bmax, "mean_mu": Bmean.mean(axis=0), "lppd_i": Bmax, "mean_ll": B.mean(axis=0),
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
    """(U, g, bounds) float64 of the tempered / bridged energy and its bounds: a temperature T divides U and g (one more
    rounding each: u |.| on top of the bound divided by T); the AIS bridge (1 - b) |w|^2 / 2 + b U, (1 - b) w + b g: the bound
    times b, the d-term sum |w|^2 ((d + 8) u on its term), and the roundings of 1 - b, the two products and the sum: 4 u on
    each term's magnitude."""
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


def used(got_U, got_g, U, G, b):
    """(worst |dU| / bound, worst |dg| / bound): the share of each bound a result uses."""
    eU = np.abs(np.asarray(got_U, dtype=np.float64) - U) / b["U"]
    eg = np.abs(np.asarray(got_g, dtype=np.float64) - G) / b["g"]
    return float(eU.max()), float(eg.max())


def far_case():
    """One 16-row block, d = 2, whose rows sit at |t| = 100: x_i = (+-50, 0) against chains w = (2, z), trials 1, 5 and 50 with
    y = 0, some and all -- softplus(100) = 100 and softplus(-100) = e^-100, sigmoid 1 and 0 to the last bit."""
    rng = np.random.RandomState(5)
    n, N = 16, 40
    X = np.zeros((n, 2), dtype=np.float32)
    X[:, 0] = np.where(np.arange(n) % 2 == 0, 50.0, -50.0)
    X[:, 1] = rng.randn(n).astype(np.float32) * 0.01
    W = np.stack([np.full(N, 2.0), rng.randn(N)], axis=1).astype(np.float32)
    m = np.asarray((1, 5, 50, 50)[:4] * 4, dtype=np.float32)
    y = np.asarray([0, 5, 50, 0, 1, 0, 25, 50, 0, 2, 0, 49, 1, 5, 1, 7], dtype=np.float32)
    return {"kind": "binomial", "W": W, "X": X, "y": np.minimum(y, m), "offset": np.zeros(n, dtype=np.float32), "trials": m}


# ---- every tile count, long histories and the edges of the likelihood (tests/test_gpu_binomial_geometries.py) --------------------
# (70, 35, d) with NT / NTM = 3 / 4 (d = 33, 40), 5 / 8 (65), 6 / 8 (96), 7 / 8 (100, 112): `glm_case.SHAPES` says why.  They are
# no part of STAT_CASES: the K_* above stay "4 x the worst over STAT_CASES"
GEOM_SHAPES = gc.SHAPES[7:]
# S > 131072 with three rows: the gather's segments are no multiple of a tile (tests/test_gpu_glm_geometries.py; the
# segmentation is a function of the number of draws alone)
LONG = [(131073, 3, 40), (140001, 3, 40), (140001, 3, 100), (140003, 3, 100)]
EDGE_ROWS = {"certain": 0, "saturated": 5, "underflow": 17, "many_trials": 33, "constant": 34}      # glm_case.EDGE_ROWS' positions
EDGE_N = gc.EDGE_N
# name -> (tau, y, trials): the row is x = tau wbar / |wbar|^2, so t = tau at the mean draw, offset 0
EDGE_SPEC = {"certain": (-120.0, 0.0, 1.0), "saturated": (120.0, 50.0, 50.0), "underflow": (2.0, 0.0, 100000.0),
             "many_trials": (0.1, float(1 << 23), float(1 << 24)), "constant": (0.0, 7.0, 50.0)}
NB_EDGE_PHIS = (1e-3, 1e4)


def edge_case(S):
    """(case, ordinary): the binomial case of 37 rows under the draws of `case(S, 32, 3)`, whose 32 rows stand in their order
    at the indices `ordinary` (37,) bool; at `EDGE_ROWS` stand five rows on the edges of the float32 likelihood, each
    x = tau wbar / |wbar|^2 with wbar the float64 mean of the draws (t = tau there) and offset 0:
        certain      tau = -120, y = 0 of 1: ll = -softplus(t) is 0 or below the float32 normal range in every draw
        saturated    tau = +120, y = 50 of 50: m softplus(t) and y t cancel; the truth is between 0 and -1e-40
        underflow    tau = 2, y = 0 of 100000: ll about -2e5 and sat = 0, exp(ll - sat) = 0 in every draw
        many_trials  tau = 0.1, y = 2^23 of 2^24 (the documented limit): every term about 1e7, ll - sat about -2e4
        constant     tau = 0 (x = 0), y = 7 of 50: the same ll in every draw
    Edge rows share 16-row blocks and MFMA operands with ordinary ones; rows 32 .. 36 are a ragged third block in a second
    row group whose last row is ordinary."""
    base = case(S, 32, 3)
    wbar = base["W"].astype(np.float64).mean(axis=0)
    ordinary = np.ones(EDGE_N, dtype=bool)
    ordinary[list(EDGE_ROWS.values())] = False
    X, y = np.zeros((EDGE_N, 3), dtype=np.float32), np.zeros(EDGE_N, dtype=np.float32)
    o, m = np.zeros(EDGE_N, dtype=np.float32), np.ones(EDGE_N, dtype=np.float32)
    X[ordinary], y[ordinary], o[ordinary], m[ordinary] = base["X"], base["y"], base["offset"], base["trials"]
    for name, i in EDGE_ROWS.items():
        tau, yi, mi = EDGE_SPEC[name]
        X[i], y[i], m[i] = (tau * wbar / (wbar @ wbar)).astype(np.float32), yi, mi
    return {"kind": "binomial", "W": base["W"], "X": X, "y": y, "offset": o, "trials": m}, ordinary


def select_rows(c, mask):
    """The case restricted to the data rows `mask` (a bool or index array)."""
    out = dict(c)
    for k in ("X", "y", "offset", "trials"):
        if k in out:
            out[k] = out[k][mask]
    return out


def nb_edge_case(phi):
    """`case(70, 33, 17, "negbinomial", phi)` at a dispersion far from NB_PHIS, with a count of 100000 in row 5."""
    c = case(70, 33, 17, "negbinomial", phi)
    c["y"] = c["y"].copy()
    c["y"][5] = 100000.0
    return c


# ---- sensitivities of the finished numbers (CPU) -------------------------------------------------------------------------------
def sensitivity(c):
    """(K_khat, K_elpd, K_neff, K_mcse) of one case: |finished(ll32)_i - finished(ll64)_i| / max_s |ll32_si - ll64_si| at its
    worst row, the finished numbers by `psis.loo_from_log_lik` with `loglik_case.r_eff_for(n)` -- the float64 route against the
    float32 numpy restatement handed to the same route."""
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


def ar1_case(kind="binomial", phi=None):
    """The AR(1) history of `glm_case.ar1_case` (steps, chains, d) with responses of this likelihood."""
    W, X, _, o = gc.ar1_case()
    rng = np.random.RandomState(9101)
    n, d = X.shape
    eta = X.astype(np.float64) @ W.reshape(-1, d).astype(np.float64).mean(axis=0) + o
    out = {"kind": kind, "W": W, "X": X, "offset": o}
    if kind == "binomial":
        m = rng.choice(TRIALS, size=n).astype(np.float64)
        out.update(y=rng.binomial(m.astype(np.int64), sigmoid(eta)).astype(np.float32), trials=m.astype(np.float32))
    else:
        mu = np.exp(eta)
        out.update(y=rng.negative_binomial(phi, phi / (phi + mu)).astype(np.float32), phi=float(phi))
    return out


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
    """`poisson_target_case.traj_case` for this likelihood (binomial data), computed once: the synthetic nets and mask `g`, the
    case `c` (its draws are the start x), v, the step size chosen on the float32 oracle, the oracle's results in float32
    (`ref`) and their distance from the same oracle in float64 (`dist`)."""
    from tests import helpers
    from tests import poisson_target_case as pc
    key = (n, d, H)
    if key in _TRAJ:
        return _TRAJ[key]
    hmc = H == 0
    g = helpers.synthetic_case("gauss_diag", d, H=max(H, 1), T=pc.TRAJ_T, N=pc.TRAJ_N, seed=d, eps=0.1)
    c = case(pc.TRAJ_N, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(pc.TRAJ_N, d).astype(np.float32)
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
def laplace_is_mean(c, s2=PRIOR_VAR, n_draws=400000, seed=0, chunk=10000):
    """`poisson_target_case.laplace_is_mean` for this likelihood: the posterior mean by self-normalised importance sampling from
    the Laplace approximation (antithetic pairs), float64, with Newton on U (Hessian X^T diag(m s (1 - s)) X + I / s2):
    (mean, its standard error, mode, Cholesky factor of the Laplace covariance)."""
    o, m, _ = terms(c)
    X, y = c["X"].astype(np.float64), c["y"].astype(np.float64)
    d = X.shape[1]
    w = np.zeros(d)
    for _ in range(200):
        s = sigmoid(X @ w + o)
        gr = X.T @ (m * s - y) + w / s2
        Hs = (X * (m * s * (1 - s))[:, None]).T @ X + np.eye(d) / s2
        step = np.linalg.solve(Hs, gr)
        w = w - step / max(1.0, np.abs(step).max())
        if np.abs(step).max() < 1e-13:
            break
    Lc = np.linalg.cholesky(np.linalg.inv(Hs))
    Z = np.random.RandomState(seed).randn(n_draws // 2, d)
    Z = np.concatenate([Z, -Z])
    Wd = w + Z @ Lc.T
    U = np.concatenate([energy(c, Wd[i:i + chunk], s2)[0] for i in range(0, len(Wd), chunk)])
    lw = -U + 0.5 * np.square(Z).sum(axis=1)
    wt = np.exp(lw - lw.max())
    wt /= wt.sum()
    mean = (wt[:, None] * Wd).sum(axis=0)
    se = np.sqrt((np.square(wt)[:, None] * np.square(Wd - mean)).sum(axis=0))
    return mean, se, w, Lc


# ---- the device entries, straight (need a GPU) ---------------------------------------------------------------------------------
def device_raw(c, W=None, lens=None, rows=None):
    """`glm_case.device_raw_glm` for this likelihood: the three entries straight through `_ffi` on the rows `rows` = (first,
    stop) of the case under the draws W, every output filled with NaN / -7 and GUARD elements longer than the entry is told."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd._history import in_place, launch, workspace
    W = c["W"] if W is None else W
    Wd = in_place(W if hasattr(W, "is_cuda") else torch.as_tensor(np.ascontiguousarray(W, dtype=np.float32)).cuda())
    S, d = int(Wd.shape[0]), int(Wd.shape[1])
    a, stop = (0, c["X"].shape[0]) if rows is None else rows
    m = stop - a
    dev, L = Wd.device, _ffi.lib()
    g = model(c)._glm
    packed, consts = g._device_data(dev)(a, m)
    assert tuple(consts.shape) == (4, m)
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
