"""Shared by tests/test_predictive_cpu.py and tests/test_gpu_predictive.py: seeded inputs of the posterior-predictive / WAIC
sums, a float64 restatement written from the definitions with scipy (independent of l2hmc_amd/predictive.py, whose numpy path
and HIP kernel are both held against it) and the error bounds of the device path, derived from the inputs alone.

Definitions, for draws W (S, d), rows X (n, d), labels y in {0, 1}: l = x_i . w_s, ll = log sigmoid((2 y_i - 1) l);
p_mean_i = mean_s sigmoid(l), lppd_i = logsumexp_s(ll) - log S, p_waic_i = var_s(ll) (ddof 1), elpd_i = lppd_i - p_waic_i,
totals = sums over rows, waic = -2 elpd, se = sqrt(n var_i(elpd_i)) (ddof 1).

The device bounds, with eps = 2^-24: A_si = sum_k |w_sk| |x_ik| and B_si = (d + 8) eps A_si + 8 eps (1 + |ll_si|) bound the
error of the float32 contraction (d products and sums, each within eps of the running magnitude <= A) carried through sigmoid
and log-sigmoid (|dp/dl| <= 1/4, |dll/dl| <= 1) plus a few ulps of the hardware exp / log / reciprocal on values of size
<= 1 + |ll|.  Per row:
    |d p_mean|  <= mean_s B / 4                       |d lppd_i| <= max_s B   (a weighted mean of per-draw relative errors)
    |d mean ll| <= mean_s B
    |d p_waic_i| <= (2 sd_i max_s B + (max_s B)^2) S / (S - 1) + 4 S 2^-52 mean_s ll^2
(var(ll + e) - var(ll) = 2 cov(ll, e) + var(e) with |e| <= max B, sd_i the population sd of ll; the last term is the float64
cancellation of sum ll^2 - (sum ll)^2 / S.)"""
import numpy as np

EPS = 2.0 ** -24


def case(S, n, d, seed, max_logit=10.0, labels="random", x_scale=1.0):
    """(W (S, d), X (n, d), y (n,)) float32: Gaussian draws and rows, the draws scaled so that the largest |logit| is
    `max_logit`; `x_scale` moves that magnitude into X (the saturation case).  labels: 'random', 'ones' or 'zeros'."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    W = rng.randn(S, d) + 0.5 * rng.randn(d)
    W *= max_logit / np.abs(W @ X.T).max()
    y = {"random": (rng.rand(n) < 0.5).astype(np.float64), "ones": np.ones(n), "zeros": np.zeros(n)}[labels]
    return (W / x_scale).astype(np.float32), (X * x_scale).astype(np.float32), y.astype(np.float32)


def log_lik(W, X, y):
    """(S, n) float64 log-likelihoods and logits, from scipy's log_expit."""
    from scipy.special import log_expit
    L = np.asarray(W, dtype=np.float64).reshape(-1, X.shape[1]) @ np.asarray(X, dtype=np.float64).T
    return log_expit((2.0 * np.asarray(y, dtype=np.float64) - 1.0) * L), L


def restatement(W, X, y):
    """Every per-row array and total, in float64, from the definitions."""
    from scipy.special import expit, logsumexp
    ll, L = log_lik(W, X, y)
    S, n = ll.shape
    out = {"p_mean": expit(L).mean(axis=0), "lppd_i": logsumexp(ll, axis=0) - np.log(S), "p_waic_i": ll.var(axis=0, ddof=1)}
    out["elpd_i"] = out["lppd_i"] - out["p_waic_i"]
    out["lppd"], out["p_waic"], out["elpd_waic"] = out["lppd_i"].sum(), out["p_waic_i"].sum(), out["elpd_i"].sum()
    out["waic"] = -2.0 * out["elpd_waic"]
    out["se"] = np.sqrt(n * out["elpd_i"].var(ddof=1)) if n > 1 else np.nan
    out["n_draws"], out["mean_ll"] = S, ll.mean(axis=0)
    return out


def device_bounds(W, X, y):
    """Per-row bounds of the device path's error (module docstring) and B itself: {'p_mean', 'lppd_i', 'mean_ll', 'p_waic_i'}
    (n,) each, 'B' (S, n), 'll' (S, n)."""
    ll, _ = log_lik(W, X, y)
    S, d = ll.shape[0], X.shape[1]
    A = np.abs(np.asarray(W, dtype=np.float64).reshape(-1, d)) @ np.abs(np.asarray(X, dtype=np.float64)).T
    B = (d + 8) * EPS * A + 8 * EPS * (1.0 + np.abs(ll))
    Bmax, sd = B.max(axis=0), ll.std(axis=0)
    return {"p_mean": B.mean(axis=0) / 4, "lppd_i": Bmax, "mean_ll": B.mean(axis=0),
            "p_waic_i": (2 * sd * Bmax + Bmax ** 2) * S / (S - 1) + 4 * S * 2.0 ** -52 * (ll * ll).mean(axis=0),
            "B": B, "ll": ll}


def ratios(got, ref, bounds):
    """Worst |error| / bound of each gated quantity; `got` is a finished Summary plus 'mean_ll'."""
    return {k: float(np.max(np.abs(np.asarray(got[k]) - ref[k]) / bounds[k])) for k in ("p_mean", "lppd_i", "mean_ll", "p_waic_i")}


def laplace_recipe(n=2000, d=10, n_draws=2000):
    """The deterministic sanity recipe: RandomState(0); X = randn(n, d) as float32; w_true = randn(d) 2 / sqrt(d);
    y ~ Bernoulli(sigmoid(X w_true)); Newton to the posterior mode under the unit prior; draws = mode + randn @ chol(H^-1)^T."""
    from scipy.special import expit
    rng = np.random.RandomState(0)
    X = rng.randn(n, d).astype(np.float32)
    w_true = rng.randn(d) * 2.0 / np.sqrt(d)
    X64 = X.astype(np.float64)
    y = (rng.rand(n) < expit(X64 @ w_true)).astype(np.float32)
    w = np.zeros(d)
    for _ in range(50):
        p = expit(X64 @ w)
        H = (X64 * (p * (1 - p))[:, None]).T @ X64 + np.eye(d)
        step = np.linalg.solve(H, X64.T @ (p - y) + w)
        w -= step
        if np.abs(step).max() < 1e-13:
            break
    C = np.linalg.cholesky(np.linalg.inv(H))
    return w + rng.randn(n_draws, d) @ C.T, X, y
