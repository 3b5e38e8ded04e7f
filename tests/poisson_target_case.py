"""Shared by tests/test_poisson_target_cpu.py, tests/test_gpu_poisson_target.py and tools/poisson_target_accuracy.py: seeded inputs
of the fused Poisson-regression target (L2HMC_ENERGY_POISSON; `PoissonRegression.get_energy_function(fused=True)`), a float64
restatement of U and grad U written from the definition (independent of l2hmc_amd/distributions.py), the same statement in
float32 numpy (the oracle's energy) and the bounds of the device path, derived from the inputs.

Definitions, for chains W (N, d), rows X (n, d), counts y, offsets o (float32 inputs, restated in float64), prior variance s2:
    h_i = x_i . w + o_i      mu_i = exp(h_i)      t_i = mu_i - y_i h_i      r_i = mu_i - y_i
    U = sum_i t_i + |w|^2 / (2 s2)                g_k = sum_i x_ik r_i + w_k / s2

The bounds reuse tests/glm_case.py (its EPS = 2^-24, its dh = (d + 8) eps A + eps |h| for the float32 contraction plus the
offset's rounding, its Bmu for mu): per chain
    |dt_i| <= (y_i + mu_i e^dh) dh_i + 4 eps (y_i |h_i| + mu_i (2 + |h_i|))
    |dU|   <= sum_i |dt_i| + n eps sum_i |t_i| + (d + 8) eps |w|^2 / (2 s2) + eps |U|
    |dg_k| <= sum_i |x_ik| (Bmu_i + eps |r_i|) + (n + 8) eps sum_i |x_ik| |r_i| + 2 eps |w_k| / s2 + eps |g_k|
(the moved h and the roundings of exp and of the fused mu - y h; the n-term sum of U in any order; the prior's d-term sum, its
1 / s2 and its product; the last addition -- and for g the residual's own rounding, the n-term contraction in any order with
the eight extra roundings of the cross-wave sum, the prior's quotient and product, the last addition).

A temperature T divides U and g: one more rounding each, `scaled` adds eps |.| to the bound divided by T.  The AIS bridge
(1 - b) |w|^2 / 2 + b U, (1 - b) w + b g: the bound times b, the d-term sum |w|^2 ((d + 8) eps on its term), and the roundings
of 1 - b, the two products and the sum: 4 eps on each term's magnitude."""
import numpy as np

from tests import glm_case as gc

EPS = gc.EPS
PRIOR_VAR = 2.0


def case(N, n, d, zero_offset=False, seed=None):
    """(W (N, d), X, y, o) of `glm_case.case` (max |x . w| = 3, offsets in [-1, 2]); zero_offset: the same with o = 0."""
    W, X, y, o = gc.case(N, n, d, seed=seed)
    return W, X, y, (np.zeros_like(o) if zero_offset else o)


def energy(W, X, y, o, s2=PRIOR_VAR, dtype=np.float64):
    """(U (N,), grad U (N, d)) from the definition, every operation in `dtype`."""
    W, X, y, o = (np.asarray(a, dtype=dtype) for a in (W, X, y, o))
    h = W @ X.T + o
    with np.errstate(over="ignore", invalid="ignore"):
        mu = np.exp(h)
        U = (mu - y * h).sum(axis=1) + dtype(0.5) * (W * W).sum(axis=1) / dtype(s2)
        G = (mu - y) @ X + W / dtype(s2)
    return U.astype(dtype), G.astype(dtype)


def oracle_energy(X, y, o, s2=PRIOR_VAR, dtype=np.float32):
    """x -> (U, grad U) in `dtype`: the energy of `oracle.l2hmc_oracle.Dynamics`."""
    return lambda W: energy(W, X, y, o, s2, dtype)


def bounds(W, X, y, o, s2=PRIOR_VAR):
    """{'U' (N,), 'g' (N, d)}: the bounds of the module docstring."""
    b = gc.bounds(W, X, y, o)
    _, h = gc.log_lik(W, X, y, o)
    W64, X64, y64 = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    n, d = X64.shape
    A = np.abs(W64) @ np.abs(X64).T
    dh = (d + 8) * EPS * A + EPS * np.abs(h)
    mu = np.exp(h)
    t, r = mu - y64 * h, mu - y64
    U, G = energy(W, X, y, o, s2)
    dt = (y64 + mu * np.exp(dh)) * dh + 4 * EPS * (y64 * np.abs(h) + mu * (2 + np.abs(h)))
    w2 = (W64 * W64).sum(axis=1)
    bU = dt.sum(axis=1) + n * EPS * np.abs(t).sum(axis=1) + (d + 8) * EPS * w2 / (2 * s2) + EPS * np.abs(U)
    aX = np.abs(X64)
    bg = (b["Bmu"] + EPS * np.abs(r)) @ aX + (n + 8) * EPS * (np.abs(r) @ aX) + 2 * EPS * np.abs(W64) / s2 + EPS * np.abs(G)
    return {"U": bU, "g": bg}


def scaled(W, X, y, o, s2=PRIOR_VAR, temperature=1.0, beta=1.0):
    """(U, g, bounds) float64 of the tempered / bridged energy and its bounds (module docstring)."""
    U, G = energy(W, X, y, o, s2)
    b = bounds(W, X, y, o, s2)
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


# ---- trajectories against the oracle --------------------------------------------------------------------------------------------
STATE_GATE, SCALAR_GATE = 3e-5, 1e-4          # this project's logistic-regression gates: states; log-Jacobian and accept probability
TRAJ_SHAPES = [(17, 5), (200, 25), (1000, 25), (300, 100)]
TRAJ_CASES = [(n, d, H) for (n, d) in TRAJ_SHAPES for H in (0, 10)] + [(200, 25, 24)]
TRAJ_N, TRAJ_T = 48, 6


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.isfinite(b)
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m])))) if m.any() else 0.0


def abs_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.isfinite(b)
    return float(np.max(np.abs(a[m] - b[m]))) if m.any() else 0.0


def oracle_dynamics(g, X, y, o, hmc, eps, dtype=np.float32, temperature=1.0, T=None):
    from oracle import l2hmc_oracle as O
    xn = vn = None
    if not hmc:
        xn, vn = ({k: g[p + k] for k in O.NET_KEYS} for p in ("xnet.", "vnet."))
    return O.Dynamics(int(g["x_dim"]), oracle_energy(X, y, o, PRIOR_VAR, dtype), int(g["T"]) if T is None else T, eps, g["mask"],
                      xn, vn, temperature=temperature, dtype=dtype)


def choose_eps(make, x, v, start=0.1, lo=0.2):
    """The first step size of start, start / 2, ... at which the float32 oracle's mean accept probability lies in (lo, 1)."""
    eps = start
    for _ in range(24):
        p = make(eps).forward(x, v)[2]
        if lo < float(p.mean()) < 1.0:
            return eps
        eps *= 0.5
    raise AssertionError("no step size with a mean accept probability in (%g, 1)" % lo)


_TRAJ = {}


def traj_case(n, d, H):
    """One case of the trajectory test, computed once: the synthetic nets and mask `g`, the data, the start (x = the draws of
    `case`, v), the step size chosen on the float32 oracle, and the oracle's results in float32 (`ref`) with their distance from
    the same oracle in float64 (`dist`): keys 'fwd0', 'fwd3', 'bwd0', 'bwd3' -> (x, v, log-Jacobian), 'forward' -> (x, v,
    log-Jacobian, accept probability)."""
    key = (n, d, H)
    if key in _TRAJ:
        return _TRAJ[key]
    from tests import helpers
    hmc = H == 0
    g = helpers.synthetic_case("gauss_diag", d, H=max(H, 1), T=TRAJ_T, N=TRAJ_N, seed=d, eps=0.1)
    x, X, y, o = case(TRAJ_N, n, d)
    v = np.random.RandomState(3).randn(TRAJ_N, d).astype(np.float32)
    eps = choose_eps(lambda e: oracle_dynamics(g, X, y, o, hmc, e), x, v)

    def run(dtype):
        od = oracle_dynamics(g, X, y, o, hmc, eps, dtype)
        xx, vv = x.astype(dtype), v.astype(dtype)
        out = {}
        for s in (0, 3):
            out["fwd%d" % s] = od.forward_step(xx, vv, s)
            out["bwd%d" % s] = od.backward_step(xx, vv, s)
        X1, V1, lj = od.forward(xx, vv, log_jac=True)
        out["forward"] = (X1, V1, lj, od.forward(xx, vv)[2])
        return out
    ref, r64 = run(np.float32), run(np.float64)
    dist = {k: tuple((abs_err if (k == "forward" and i == 3) else rel_err)(a, b) for i, (a, b) in enumerate(zip(ref[k], r64[k])))
            for k in ref}
    _TRAJ[key] = {"g": g, "X": X, "y": y, "o": o, "x": x, "v": v, "eps": eps, "hmc": hmc, "ref": ref, "dist": dist}
    return _TRAJ[key]


def gate(base, dist):
    """The tolerance of one compared quantity: the project's gate, or 4 x the float32 oracle's own distance from float64 (the
    kernel orders its sums differently and uses the hardware exp2) where that is larger."""
    return max(base, 4.0 * dist)


# ---- overflow --------------------------------------------------------------------------------------------------------------------
OVER_N = 64


def overflow_case():
    """HMC on (n, d) = (100, 5) with ONE more row whose feature vector is c u (u a unit vector, y = 0, o = 0).  All 64 chains
    start where that row's h is -20 (mu = 2e-9: the row is silent).  The first 24 chains get a momentum of 2 + |z| along u: the
    other rows' gradient (|grad U| about 100 here) turns it by eps |grad U| / 2 = 0.25 at most, so their first position update
    moves h by more than c eps 1.75 = 350, past 88.7, where float32 exp overflows.  The other 40 move away from the row (momentum
    -2 - |z| along u, which five half-kicks of 0.25 cannot reverse) and are ordinary HMC chains.  Returns the data, the start, the momenta, the accept
    uniforms, eps, T and -- from the float32 oracle alone -- `p`, `nonfinite` (the proposal's energy is not finite) and `accepted`
    (accept probability > 0), and `dist_p`, the distance of p from the float64 oracle's over the accepted chains."""
    T, eps, c, n_over = 5, 0.005, 40000.0, 24
    x, X, y, o = case(OVER_N, 100, 5)
    rng = np.random.RandomState(17)
    u = rng.randn(5)
    u /= np.linalg.norm(u)
    x64 = x.astype(np.float64)
    x = (x64 - np.outer(x64 @ u, u) - (20.0 / c) * u).astype(np.float32)
    X = np.concatenate([X, (c * u)[None, :].astype(np.float32)])
    y, o = np.concatenate([y, [0.0]]).astype(np.float32), np.concatenate([o, [0.0]]).astype(np.float32)
    v = rng.randn(OVER_N, 5)
    vu = v @ u
    want = np.where(np.arange(OVER_N) < n_over, 2.0 + np.abs(vu), -2.0 - np.abs(vu))
    v = (v + np.outer(want - vu, u)).astype(np.float32)
    uu = rng.uniform(0.01, 1.0, size=OVER_N).astype(np.float32)
    g = {"x_dim": 5, "T": T, "mask": np.zeros((T, 5), dtype=np.float32)}
    with np.errstate(all="ignore"):
        od = oracle_dynamics(g, X, y, o, True, eps)
        X1, V1, p = od.forward(x, v)
        U1 = od.energy(X1)
        p64 = oracle_dynamics(g, X, y, o, True, eps, np.float64).forward(x.astype(np.float64), v.astype(np.float64))[2]
    acc = p > 0.0
    return {"X": X, "y": y, "o": o, "x": x, "v": v, "u": uu, "eps": eps, "T": T, "p": p, "nonfinite": ~np.isfinite(U1),
            "accepted": acc, "dist_p": abs_err(p[acc], p64[acc])}


# ---- the posterior mean ------------------------------------------------------------------------------------------------------------
def laplace_is_mean(X, y, o, s2=PRIOR_VAR, n_draws=400000, seed=0, chunk=10000):
    """Posterior mean by self-normalised importance sampling from the Laplace approximation (antithetic pairs), float64, with
    Newton on the Poisson U: (mean, its standard error, mode, Cholesky factor of the Laplace covariance)."""
    X, y, o = (np.asarray(a, dtype=np.float64) for a in (X, y, o))
    d = X.shape[1]
    w = np.zeros(d)
    for _ in range(100):
        mu = np.exp(X @ w + o)
        gr = X.T @ (mu - y) + w / s2
        Hs = (X * mu[:, None]).T @ X + np.eye(d) / s2
        step = np.linalg.solve(Hs, gr)
        w = w - step / max(1.0, np.abs(step).max())             # damped while far away (exp makes the full step overshoot)
        if np.abs(step).max() < 1e-13:
            break
    Lc = np.linalg.cholesky(np.linalg.inv(Hs))
    Z = np.random.RandomState(seed).randn(n_draws // 2, d)
    Z = np.concatenate([Z, -Z])
    Wd = w + Z @ Lc.T
    U = np.concatenate([energy(Wd[i:i + chunk], X, y, o, s2)[0] for i in range(0, len(Wd), chunk)])
    lw = -U + 0.5 * np.square(Z).sum(axis=1)
    wt = np.exp(lw - lw.max())
    wt /= wt.sum()
    mean = (wt[:, None] * Wd).sum(axis=0)
    se = np.sqrt((np.square(wt)[:, None] * np.square(Wd - mean)).sum(axis=0))
    return mean, se, w, Lc
