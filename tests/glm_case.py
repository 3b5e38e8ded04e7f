"""Shared by tests/test_glm_cpu.py, tests/test_gpu_glm.py and tools/glm_accuracy.py: seeded inputs of the Poisson regression's
model criticism (`l2hmc_amd.PoissonRegression`, l2hmc_amd/glm.py, csrc/glm.hip), a float64 restatement written from the
definition with scipy's gammaln (independent of l2hmc_amd/glm.py) and the bounds of the device path, derived from the inputs.

Definitions, for draws W (S, d), rows X (n, d), counts y, offsets o (all float32 inputs, restated in float64):
    h = x_i . w_s + o_i    mu = exp(h)    ll = y_i h - mu - gammaln(y_i + 1)

The device bound, with eps = 2^-24 and A_si = sum_k |w_sk| |x_ik|: the float32 contraction is within (d + 8) eps A of the exact
eta (tests/predictive_case.py) and the sum h = eta + o adds one rounding, dh = (d + 8) eps A + eps |h|.  ll moves with h by
y dh + mu (e^dh - 1) <= (y + mu e^dh) dh, and the four float32 roundings of the device function (the product h log2 e and the
hardware exp2 inside mu: mu (|h| + 2) eps; the fused y h - mu: (y |h| + mu) eps; g rounded once: g eps; the last difference:
|ll| eps) stay inside 4 eps (y |h| + mu (2 + |h|) + g + |ll|):
    |d ll| <= (y + mu e^dh) dh + 4 eps (y |h| + mu (2 + |h|) + g + |ll|) = B_si
and the predictive mean alone: |d mu| <= mu e^dh dh + 4 eps mu (2 + |h|) = Bmu_si.  Per row, as tests/predictive_case.py
derives them with this B in the place of its own:
    |d mean mu| <= mean_s Bmu      |d lppd_i| <= max_s B      |d mean ll| <= mean_s B
    |d p_waic_i| <= (2 sd_i max_s B + (max_s B)^2) S / (S - 1) + 4 S 2^-52 mean_s ll^2

The finished numbers of PSIS-LOO are gated at K delta_i, delta_i = max_s B_si (order statistics are 1-Lipschitz in the sup
norm), with the sensitivities K below measured from the float64 route alone (`sensitivity`, run by tools/glm_accuracy.py on the
CPU, times 4: sampled sign patterns under-estimate the worst case); profiles/glm_accuracy.txt records the run."""
import numpy as np

EPS = 2.0 ** -24

# (S, n, d): all four geometries (d = 1, 2, 3 -> 1 feature tile; 17 -> 2; 50 -> 4; 128 -> 8), rows past one workgroup's 32, a
# ragged last data block, a last draw tile that is not full, one, two and many chunks (several quads at S = 4099)
SHAPES = [(25, 1, 1), (25, 3, 2), (70, 17, 3), (70, 33, 17), (70, 65, 50), (70, 50, 128), (4099, 100, 25)]
EXACT_SHAPES = [(70, 33, 3), (4099, 40, 3)]
AR1 = (200, 20, 3, 0.7, 63, False, 37)          # steps, chains, d, rho, max_lag, split, rows

# worst |change| / delta_i of the float64 route under +-B_si perturbations of ll, 8 seeded sign patterns, times 4
# (tools/glm_accuracy.py; profiles/glm_accuracy.txt)
# (the draws of `case` lie close together -- 0.1 randn about w0 -- so a row's ll spread is small against its level and the
# fitted shape moves a lot per unit of ll: the khat and mcse sensitivities are two orders above the logistic fixtures')
K_KHAT = 4 * 635        # worst measured 635, on (70, 33, 17)
K_ELPD = 4 * 2.8        # worst measured 2.78, on (25, 3, 2)
K_NEFF = 4 * 4.6        # relative; worst measured 4.53, on (25, 3, 2)
K_MCSE = 4 * 79         # relative; worst measured 78.2, on (70, 33, 17)
K_REFF = 4 * 22         # relative, on the AR(1) history; worst measured 21.2


def seed_of(S, n, d):
    return 9000 + S + n + d


def case(S, n, d, seed=None):
    """(W (S, d), X (n, d), y (n,), o (n,)) float32: X = randn, draws w0 + 0.1 randn scaled so that max |x . w| = 3, offsets
    uniform in [-1, 2], y ~ Poisson(exp(X w_mean + o)), and ONE surprising last row with y = ceil(3 mu + 5)."""
    rng = np.random.RandomState(seed_of(S, n, d) if seed is None else seed)
    X = rng.randn(n, d)
    W = rng.randn(d) + 0.1 * rng.randn(S, d)
    W *= 3.0 / np.abs(W @ X.T).max()
    o = rng.uniform(-1.0, 2.0, size=n)
    mu = np.exp(X @ W.mean(axis=0) + o)
    y = rng.poisson(mu).astype(np.float64)
    y[-1] = np.ceil(3.0 * mu[-1] + 5.0)
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32), o.astype(np.float32)


def exact_case(S, n, d, seed):
    """Small-integer W with dyadic X and offsets: eta and h are exact in float32 and take few values, so ll has many ties."""
    rng = np.random.RandomState(seed)
    W = rng.randint(-1, 2, size=(S, d)).astype(np.float32)
    X = (rng.randint(-2, 3, size=(n, d)) / 4.0).astype(np.float32)
    o = (rng.randint(-4, 9, size=n) / 4.0).astype(np.float32)
    y = rng.poisson(np.exp(o.astype(np.float64))).astype(np.float32)
    return W, X, y, o


def ar1_case():
    """(W (M, N, d), X, y, o) float32: every chain an AR(1) series about a common offset, scaled like `case`."""
    M, N, d, rho, _, _, n = AR1
    rng = np.random.RandomState(9100)
    X = rng.randn(n, d)
    eps = rng.randn(M, N, d)
    Z = np.empty((M, N, d))
    Z[0] = eps[0]
    for t in range(1, M):
        Z[t] = rho * Z[t - 1] + np.sqrt(1.0 - rho * rho) * eps[t]
    W = rng.randn(d) + 0.1 * Z
    W *= 3.0 / np.abs(W.reshape(-1, d) @ X.T).max()
    o = rng.uniform(-1.0, 2.0, size=n)
    y = rng.poisson(np.exp(X @ W.reshape(-1, d).mean(axis=0) + o)).astype(np.float64)
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32), o.astype(np.float32)


def log_lik(W, X, y, o):
    """(ll, h) float64 (S, n) from the definition."""
    from scipy.special import gammaln
    W, X, y, o = (np.asarray(a, dtype=np.float64) for a in (W, X, y, o))
    h = W.reshape(-1, X.shape[1]) @ X.T + o
    return y * h - np.exp(h) - gammaln(y + 1.0), h


def bounds(W, X, y, o):
    """{'B', 'Bmu' (S, n), 'delta' (n,), 'mean_mu', 'lppd_i', 'mean_ll', 'p_waic_i' (n,)} of the module docstring."""
    from scipy.special import gammaln
    ll, h = log_lik(W, X, y, o)
    S, d = ll.shape[0], X.shape[1]
    W64, X64, y64 = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    A = np.abs(W64.reshape(-1, d)) @ np.abs(X64).T
    dh = (d + 8) * EPS * A + EPS * np.abs(h)
    mu, g = np.exp(h), gammaln(y64 + 1.0)
    Bmu = mu * np.exp(dh) * dh + 4 * EPS * mu * (2 + np.abs(h))
    B = (y64 + mu * np.exp(dh)) * dh + 4 * EPS * (y64 * np.abs(h) + mu * (2 + np.abs(h)) + g + np.abs(ll))
    Bmax, sd = B.max(axis=0), ll.std(axis=0)
    return {"B": B, "Bmu": Bmu, "delta": Bmax, "mean_mu": Bmu.mean(axis=0), "lppd_i": Bmax, "mean_ll": B.mean(axis=0),
            "p_waic_i": (2 * sd * Bmax + Bmax ** 2) * S / (S - 1) + 4 * S * 2.0 ** -52 * (ll * ll).mean(axis=0)}


def restatement(W, X, y, o):
    """The predictive numbers per row, float64, from the definitions."""
    from scipy.special import logsumexp
    ll, h = log_lik(W, X, y, o)
    S = ll.shape[0]
    out = {"mean_mu": np.exp(h).mean(axis=0), "lppd_i": logsumexp(ll, axis=0) - np.log(S), "p_waic_i": ll.var(axis=0, ddof=1),
           "mean_ll": ll.mean(axis=0)}
    out["elpd_i"] = out["lppd_i"] - out["p_waic_i"]
    return out


def rel(a, b):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)


def sensitivity(S, n, d, patterns=8):
    """(K_khat, K_elpd, K_neff, K_mcse) of one shape: the worst |change| / delta_i of the float64 route
    (`psis.loo_from_log_lik` on the float64 matrix, with `loglik_case.r_eff_for(n)`) when ll moves by +-B_si."""
    from l2hmc_amd import psis
    from tests import loglik_case as lk
    W, X, y, o = case(S, n, d)
    ll, _ = log_lik(W, X, y, o)
    b = bounds(W, X, y, o)
    r = lk.r_eff_for(n)
    ref = psis.loo_from_log_lik(ll, r_eff=r)
    fin = np.isfinite(ref.khat)
    worst = np.zeros(4)
    rng = np.random.RandomState(77)
    for _ in range(patterns):
        got = psis.loo_from_log_lik(ll + np.where(rng.rand(*ll.shape) < 0.5, -1.0, 1.0) * b["B"], r_eff=r)
        both = fin & np.isfinite(got.khat)
        with np.errstate(all="ignore"):
            k = np.max((np.abs(got.khat - ref.khat) / b["delta"])[both]) if both.any() else 0.0
            vals = (k, np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / b["delta"]),
                    np.max((rel(got.n_eff, ref.n_eff) / b["delta"])[both]) if both.any() else 0.0,
                    np.max((rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / b["delta"])[both]) if both.any() else 0.0)
        worst = np.maximum(worst, vals)
    return tuple(float(v) for v in worst)


def reff_sensitivity(patterns=8):
    """The worst |relative change of r_eff| / delta_i of the float64 route on the AR(1) history when ll moves by +-B_si."""
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split, n = AR1
    W, X, y, o = ar1_case()
    ll, _ = log_lik(W, X, y, o)
    b = bounds(W, X, y, o)
    ref = psis.relative_eff_from_log_lik(ll.reshape(M, N, n), max_lag=max_lag, split=split)
    worst, rng = 0.0, np.random.RandomState(78)
    for _ in range(patterns):
        moved = ll + np.where(rng.rand(*ll.shape) < 0.5, -1.0, 1.0) * b["B"]
        got = psis.relative_eff_from_log_lik(moved.reshape(M, N, n), max_lag=max_lag, split=split)
        worst = max(worst, float(np.max(rel(got.r_eff, ref.r_eff) / b["delta"])))
    return worst
