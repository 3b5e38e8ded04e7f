"""Shared by tests/test_loo_cpu.py and tests/test_gpu_loo.py (and tools/loo_accuracy.py): seeded inputs of PSIS-LOO, a float64
restatement written from the definition (independent of l2hmc_amd/predictive.py: one row at a time, a full sort, the rule
`lw > cutoff` of the `loo` package, smoothed weights written back into the vector of all S log weights, two logaddexp
reductions -- no tail / body decomposition), and the bounds of the device path, derived from the inputs alone.

Definitions, for draws W (S, d), rows X (n, d), labels y: t_si = (2 y_i - 1) x_i . w_s, ll = -softplus(-t), the log importance
ratio lw = -ll.  Per row: M = min(S // 5, ceil(3 sqrt S)), cutoff = the (M + 1)-th largest lw, tail = {lw > cutoff}; with at
least 5 tail members a generalised Pareto is fitted to exp(lw - max) - exp(cutoff - max) (Zhang & Stephens 2009 with the prior
of `loo`), its quantiles replace the tail's weights (capped at the largest raw weight), khat is the fitted shape, otherwise
khat = inf and the raw weights stay; elpd_loo_i = logsumexp(lw' + ll) - logsumexp(lw').

The device bound.  With eps = 2^-24 and A_si = sum_k |w_sk| |x_ik| the float32 logit is within (d + 8) eps A_si of the exact
one (tests/predictive_case.py), so delta_i = max_s (d + 8) eps A_si bounds every logit of row i; order statistics are
1-Lipschitz in the sup norm, so the cutoff and every sorted tail element are within delta_i of the reference's.  The finished
numbers are gated at K delta_i with the sensitivities K_KHAT and K_ELPD below, measured from the float64 route alone."""
import math

import numpy as np

EPS = 2.0 ** -24
KHAT_BAD = 0.7

# The worst |change| / delta_i of khat and elpd_loo_i of the float64 route under +-delta_si perturbations of the logits, over
# FIXTURES and 8 seeded sign patterns, times 4 (sampled sign patterns under-estimate the worst case): tools/loo_accuracy.py
# measures them on the CPU and profiles/loo_accuracy.txt records the run.
K_KHAT = 4 * 4.7        # worst measured 4.664, on (37, 17, 3)
K_ELPD = 4 * 2.2        # worst measured 2.19, on (300, 50, 128)
# the device `loo_finish` against the numpy one on the same tails: 100 x the worst difference measured on the MI355X
# (profiles/loo_accuracy.txt), never looser than 1e-6
FINISH_KHAT = 3.6e-12    # worst measured 3.54e-14, on (4099, 100, 25)
FINISH_ELPD = 8e-13      # worst measured 7.99e-15

FIXTURES = [(25, 1, 1), (24, 3, 2), (37, 17, 3), (16, 16, 16), (523, 33, 17), (300, 50, 128), (4099, 100, 25)]


def tail_len(S):
    return min(S // 5, math.isqrt(9 * S - 1) + 1)


def seed_of(S, n, d):
    return 2000 + S + n + d


def case(S, n, d, seed=None, max_logit=10.0):
    """(W (S, d), X (n, d), y (n,)) float32 as predictive_case.case makes them (Gaussian draws about a common offset, scaled so
    that the largest |logit| is `max_logit`), plus ONE surprising row: the last row lies 3 prior standard deviations along the
    generating weight vector (the draws' mean) and carries the wrong label, so a few draws dominate its importance weights."""
    rng = np.random.RandomState(seed_of(S, n, d) if seed is None else seed)
    X = rng.randn(n, d)
    W = rng.randn(S, d) + 0.5 * rng.randn(d)
    W *= max_logit / np.abs(W @ X.T).max()
    y = (rng.rand(n) < 0.5).astype(np.float64)
    w = W.mean(axis=0)
    X[-1] = 3.0 * w / np.linalg.norm(w)
    y[-1] = 0.0                                              # x . w > 0 predicts 1
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32)


def exact_case(S, n, d, seed):
    """Small-integer W and dyadic X: every product and partial sum is exact in float32 (|t| < 2^12 in steps of 1/4), so the
    device's logits equal the float64 ones bit for bit, with many ties."""
    rng = np.random.RandomState(seed)
    W = rng.randint(-4, 5, size=(S, d)).astype(np.float32)
    X = (rng.randint(-8, 9, size=(n, d)) / 4.0).astype(np.float32)
    y = (rng.rand(n) < 0.5).astype(np.float32)
    return W, X, y


def degenerate(kind, W):
    """'twice': every draw twice; 'half': the second half of the draws one repeated vector; 'constant': all draws identical."""
    W = np.array(W)
    if kind == "twice":
        return np.concatenate([W, W])
    if kind == "half":
        W[W.shape[0] // 2:] = W[0]
        return W
    if kind == "constant":
        W[:] = W[0]
        return W
    raise ValueError(kind)


def signed_logits(W, X, y):
    W, X, y = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    return (W.reshape(-1, X.shape[1]) @ X.T) * (2.0 * y - 1.0)


def delta(W, X):
    """(delta_i (n,), delta_si (S, n)): the bound of the float32 logit error."""
    W, X = np.asarray(W, dtype=np.float64), np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    D = (d + 8) * EPS * (np.abs(W.reshape(-1, d)) @ np.abs(X).T)
    return D.max(axis=0), D


def _gpdfit(x):
    """(k, sigma) of the generalised Pareto fitted to the ascending sample x > 0 (Zhang & Stephens 2009; `loo::gpdfit`)."""
    N = len(x)
    m = 30 + int(math.floor(math.sqrt(N)))
    jj = np.arange(1, m + 1, dtype=np.float64)
    x_star = x[int(math.floor(N / 4.0 + 0.5)) - 1]
    theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (jj - 0.5))) / (3.0 * x_star)
    k = np.array([np.mean(np.log1p(-th * x)) for th in theta])
    ell = N * (np.log(-theta / k) - k - 1.0)
    w = np.array([1.0 / np.sum(np.exp(ell - e)) for e in ell])
    theta_hat = float(np.sum(theta * w))
    k = float(np.mean(np.log1p(-theta_hat * x)))
    sigma = -k / theta_hat
    return (k * N + 5.0) / (N + 10.0), sigma


def restate_row(t):
    """(elpd_loo_i, khat, n_tail) of one row from its S signed logits, the direct form."""
    S = len(t)
    ll = -np.logaddexp(0.0, -t)
    lw = -ll
    M = tail_len(S)
    cutoff = np.sort(lw)[S - M - 1]
    idx = np.nonzero(lw > cutoff)[0]
    L = len(idx)
    mx = lw.max()
    lw = lw - mx
    khat = np.inf
    if L >= 5:
        order = idx[np.argsort(lw[idx], kind="stable")]
        ec = np.exp(cutoff - mx)
        with np.errstate(all="ignore"):
            k, sigma = _gpdfit(np.exp(lw[order]) - ec)
            if np.isfinite(k) and np.isfinite(sigma):
                p = (np.arange(1, L + 1) - 0.5) / L
                q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
                lw[order] = np.minimum(np.log(q + ec), 0.0)
                khat = k
    return np.logaddexp.reduce(lw + ll) - np.logaddexp.reduce(lw), khat, L


def restatement(W, X, y, t=None):
    """{'elpd_loo_i', 'khat', 'n_tail', 'lppd_i'} (n,) each, one row at a time; `t` replaces the logits (the sensitivity runs)."""
    t = signed_logits(W, X, y) if t is None else t
    rows = [restate_row(t[:, i]) for i in range(t.shape[1])]
    S = t.shape[0]
    return {"elpd_loo_i": np.array([r[0] for r in rows]), "khat": np.array([r[1] for r in rows]),
            "n_tail": np.array([r[2] for r in rows], dtype=np.int64),
            "lppd_i": np.logaddexp.reduce(-np.logaddexp(0.0, -t), axis=0) - math.log(S)}


def khat_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), KHAT_BAD)
