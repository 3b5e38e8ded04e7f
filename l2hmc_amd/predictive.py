"""Posterior predictive, log pointwise predictive density and WAIC of Bayesian logistic regression over every recorded draw
(Watanabe 2010; Gelman, Hwang, Vehtari 2014; Vehtari, Gelman, Gabry 2017 -- WAIC with the variance form of the penalty).

    s = waic(x_hist[burn_in:], X, y)                 # x_hist of sample_chain(record=True): (M, N, d), or a matrix (S, d)
    s.elpd_waic, s.waic, s.p_waic, s.lppd, s.se, s.n_high_variance, s.n_underflow, s.elpd_i, ...
    p = predict_proba(x_hist[burn_in:], X_new)       # (n,) posterior predictive P(y = 1)
    h = log_predictive_density(x_hist[burn_in:], X_test, y_test)       # held-out lppd: h.lppd, h.lppd_i, h.se

Both are expectations over every draw s of a function of every data row i.  With l = x_i . w_s and z = (2 y_i - 1) l:

    p1 = sigmoid(l)      lik = sigmoid(z)      ll = log lik = -softplus(-z)
    pointwise_sums:  sum_p = sum_s p1,  sum_lik = sum_s lik,  sum_ll = sum_s ll,  sum_ll2 = sum_s ll^2         (each (n,))
    finish:          p_mean = sum_p / S,  lppd_i = log(sum_lik / S),  p_waic_i = (sum_ll2 - sum_ll^2 / S) / (S - 1),
                     elpd_i = lppd_i - p_waic_i;  lppd, p_waic, elpd_waic = their sums over rows,  waic = -2 elpd_waic,
                     se = sqrt(n var_i(elpd_i))  (sample variance over the rows; NaN for one row)

A ROCm tensor of draws goes to the HIP kernel behind `l2hmc_logistic_predict` (csrc/predictive.hip) where it lies -- a first-axis
slice of a history is contiguous -- the (S, n) log-likelihood matrix is never formed and only the (4, n) sums come back; the
logits are float32 there and the sums float64, bitwise reproducible.  numpy or a CPU tensor is computed in float64 numpy
(`_history` has that rule and the host side of the launches), with a two-pass variance and `logaddexp`; the host sums carry
these as `m2_ll` and `log_sum_lik`, which `finish` prefers when they are there.  The four plain sums are what ranks that hold different draws add up (`sharding.predictive`).

Summing lik itself needs no running maximum and is exact as long as one draw gives lik above the smallest float32; a row where
every draw underflows has sum_lik = 0, lppd_i = -inf, and is counted in `n_underflow` -- reported, not hidden.
`n_high_variance` counts the rows with p_waic_i > 0.4, the usual warning threshold: WAIC is unreliable there.
"""
import numpy as np

from . import _ffi
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace
from .diagnostics import Summary

MAX_DEVICE_ROWS = 1 << 20     # l2hmc_pack_logistic
MAX_DEVICE_DIM = 128
HIGH_VARIANCE = 0.4
_HOST_CHUNK_ELEMS = 1 << 22   # (draws x rows) logits formed at a time on the host


def _check(draws, X, y):
    """(S, d, n) of valid arguments, or ValueError (shapes only: the labels' values are checked where they lie)."""
    shape = history_shape(draws, flat_ok=True, says="draws are a history (steps, chains, dim) or a matrix (n_draws, dim)")
    d = shape[-1]
    S = shape[0] * shape[1] if len(shape) == 3 else shape[0]
    if d < 1:
        raise ValueError("draws need dim >= 1")
    if S < 2:
        raise ValueError("the predictive sums need >= 2 draws (got %d)" % S)
    xs = tuple(int(v) for v in X.shape)
    if len(xs) != 2 or xs[0] < 1:
        raise ValueError("X must be (n_rows, d) with n_rows >= 1; got shape %s" % (xs,))
    if xs[1] != d:
        raise ValueError("X has %d features but the draws have dim %d" % (xs[1], d))
    if y is not None and tuple(int(v) for v in y.shape) != (xs[0],):
        raise ValueError("y must be (n_rows,) = (%d,), got shape %s" % (xs[0], tuple(y.shape)))
    return S, d, xs[0]


def _device_sums(draws, X, y, S, d, n):
    import torch
    if n > MAX_DEVICE_ROWS or d > MAX_DEVICE_DIM:
        raise ValueError("the predictive kernel holds n_rows <= %d and dim <= %d (got %d, %d)"
                         % (MAX_DEVICE_ROWS, MAX_DEVICE_DIM, n, d))
    dev = draws.device
    W = in_place(draws)
    Xd = torch.as_tensor(X).detach().to(device=dev, dtype=torch.float32).contiguous()
    if y is None:
        yd = torch.zeros(n, dtype=torch.float32, device=dev)
    else:
        yd = torch.as_tensor(y).detach().to(device=dev, dtype=torch.float32).contiguous()
        if not bool(((yd == 0) | (yd == 1)).all()):
            raise ValueError("labels y must be 0 or 1")
    L = _ffi.lib()
    packed = workspace(dev, torch.float32, L.l2hmc_packed_logistic_floats, n, d)
    launch(dev, L.l2hmc_pack_logistic, Xd.data_ptr(), yd.data_ptr(), n, d, packed.data_ptr())
    ws = workspace(dev, torch.float64, L.l2hmc_logistic_predict_workspace_doubles, S, n, d)
    sums = torch.empty((4, n), dtype=torch.float64, device=dev)
    launch(dev, L.l2hmc_logistic_predict, W.data_ptr(), S, d, packed.data_ptr(), n, sums.data_ptr(), ws.data_ptr())
    return sums.cpu().numpy()


def _host_sums(draws, X, y, S, d, n):
    W = as_numpy(draws, np.float64).reshape(S, d)
    X = as_numpy(X, np.float64)
    if y is None:
        y = np.zeros(n)
    else:
        y = as_numpy(y, np.float64)
        if not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("labels y must be 0 or 1")
    sign = 2.0 * y - 1.0
    step = max(1, _HOST_CHUNK_ELEMS // n)
    out = {k: np.zeros(n) for k in ("sum_p", "sum_lik", "sum_ll", "sum_ll2", "m2_ll")}
    log_sum = np.full(n, -np.inf)
    with np.errstate(over="ignore", under="ignore"):
        for a in range(0, S, step):                          # pass 1
            Lg = W[a:a + step] @ X.T
            ll = -np.logaddexp(0.0, -sign * Lg)
            out["sum_p"] += np.exp(-np.logaddexp(0.0, -Lg)).sum(axis=0)
            out["sum_lik"] += np.exp(ll).sum(axis=0)
            out["sum_ll"] += ll.sum(axis=0)
            out["sum_ll2"] += (ll * ll).sum(axis=0)
            log_sum = np.logaddexp(log_sum, np.logaddexp.reduce(ll, axis=0))
        mean = out["sum_ll"] / S
        for a in range(0, S, step):                          # pass 2: the variance about the mean
            z = -np.logaddexp(0.0, -sign * (W[a:a + step] @ X.T)) - mean
            out["m2_ll"] += (z * z).sum(axis=0)
    out["log_sum_lik"] = log_sum
    return out


def pointwise_sums(draws, X, y=None):
    """{'sum_p', 'sum_lik', 'sum_ll', 'sum_ll2': (n,) float64 numpy, 'n_draws': S} of draws (M, N, d) or (S, d) against the
    rows of X (n, d) with labels y in {0, 1} (None: zeros -- `sum_p` does not depend on them).  A ROCm tensor of draws -> the
    HIP kernel, read in place (bitwise reproducible); numpy or a CPU tensor -> float64 numpy, which adds 'm2_ll' (two-pass
    sum of squares about the mean) and 'log_sum_lik' (by logaddexp)."""
    S, d, n = _check(draws, X, y)
    if is_device_tensor(draws):
        s = _device_sums(draws, X, y, S, d, n)
        out = {"sum_p": s[0], "sum_lik": s[1], "sum_ll": s[2], "sum_ll2": s[3]}
    else:
        out = _host_sums(draws, X, y, S, d, n)
    out["n_draws"] = S
    return out


def finish(sums):
    """The `Summary` of `pointwise_sums`' result (or of the four sums ranks have added up): per-row `p_mean`, `lppd_i`,
    `p_waic_i`, `elpd_i` and the totals `lppd`, `p_waic`, `elpd_waic`, `waic`, `se`, with `n_draws`, `n_high_variance` and
    `n_underflow`.  A row whose likelihood underflowed in every draw has lppd_i = -inf, quietly."""
    S = int(sums["n_draws"])
    if S < 2:
        raise ValueError("the predictive sums need >= 2 draws (got %d)" % S)
    get = lambda k: np.asarray(sums[k], dtype=np.float64)  # noqa: E731
    sum_p, sum_lik, sum_ll, sum_ll2 = get("sum_p"), get("sum_lik"), get("sum_ll"), get("sum_ll2")
    n = sum_p.shape[0]
    with np.errstate(all="ignore"):
        p_mean = sum_p / S
        lppd_i = get("log_sum_lik") - np.log(S) if "log_sum_lik" in sums else np.log(sum_lik / S)
        m2 = get("m2_ll") if "m2_ll" in sums else sum_ll2 - sum_ll * sum_ll / S
        p_waic_i = m2 / (S - 1)
        elpd_i = lppd_i - p_waic_i
        lppd, p_waic, elpd = float(lppd_i.sum()), float(p_waic_i.sum()), float(elpd_i.sum())
        se = float(np.sqrt(n * elpd_i.var(ddof=1))) if n > 1 else float("nan")
    return Summary(p_mean=p_mean, lppd_i=lppd_i, p_waic_i=p_waic_i, elpd_i=elpd_i, lppd=lppd, p_waic=p_waic, elpd_waic=elpd,
                   waic=-2.0 * elpd, se=se, n_draws=S, n_rows=n, n_high_variance=int(np.sum(p_waic_i > HIGH_VARIANCE)),
                   n_underflow=int(np.sum(np.isneginf(lppd_i))))


def waic(draws, X, y):
    """WAIC of the logistic regression (X, y) under the posterior draws: `finish(pointwise_sums(draws, X, y))`.  Compare two
    models on the same rows by `elpd_waic` (higher is better) against `se`."""
    if y is None:
        raise ValueError("waic needs the labels y")
    return finish(pointwise_sums(draws, X, y))


def predict_proba(draws, X_new):
    """The posterior predictive P(y = 1 | x) of every row of X_new: (n,) float64, the mean of sigmoid(x . w) over the draws."""
    s = pointwise_sums(draws, X_new)
    return np.asarray(s["sum_p"], dtype=np.float64) / s["n_draws"]


def log_predictive_density(draws, X_new, y_new):
    """The held-out log pointwise predictive density: `Summary(lppd, lppd_i, se, n_draws, n_rows, n_underflow)` with
    lppd_i = log mean_s P(y_i | x_i, w_s) and se = sqrt(n var_i(lppd_i))."""
    if y_new is None:
        raise ValueError("log_predictive_density needs the labels y_new")
    f = finish(pointwise_sums(draws, X_new, y_new))
    n = f.n_rows
    with np.errstate(all="ignore"):
        se = float(np.sqrt(n * f.lppd_i.var(ddof=1))) if n > 1 else float("nan")
    return Summary(lppd=f.lppd, lppd_i=f.lppd_i, se=se, n_draws=f.n_draws, n_rows=n, n_underflow=f.n_underflow)
