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

The standard answer to those rows is PSIS-LOO (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024) with its
per-row diagnostic, the Pareto k-hat:

    s = loo(x_hist[burn_in:], X, y)                  # = loo_finish(loo_tails(...))
    s.elpd_loo, s.p_loo, s.looic, s.se, s.khat, s.n_bad, s.khat_threshold, s.n_above_threshold, s.elpd_loo_i, ...

The log importance ratio of row i under draw s is softplus(-t) with t = (2 y_i - 1) x_i . w_s the signed logit, and it decreases
in t.  PSIS needs per row only the M = min(S // 5, ceil(3 sqrt S)) smallest t -- the tail, cut strictly before the element of
rank M so that ties shorten it, the rule of the `loo` package -- and one sum over the other draws: `loo_tails` returns
{'cutoff', 'n_tail', 'tail' (n, M; +inf past n_tail), 'body', 'sum_lik', 'tail_len', 'n_draws'}, where body = the sum over the
draws outside the tail of e^m + e^(m - t), m = min(cutoff, 0).  A ROCm tensor of draws goes to the kernels behind
`l2hmc_logistic_loo_tails` (csrc/loo.hip: a fused contraction and per-row radix select, nothing is sorted, float32 t, bitwise
reproducible) and the dict holds device tensors; numpy or a CPU tensor is float64 numpy.  `loo_finish` fits the generalised
Pareto distribution to every tail (Zhang & Stephens 2009 with the prior of `loo`), smooths the tail weights and forms elpd_loo_i
in float64 where the tails lie: torch on the device in row chunks of bounded memory, numpy on the host.
`finish="kernel"` (opt-in, device tails only) fits and smooths on the fused float64 kernels of csrc/psis.hip instead (`psis.py`).

The recorded draws are Markov chains, not independent: `relative_eff(x_hist, X, y)` gives per row r_eff_i = ESS(lik_i) / S, the
relative efficiency of `loo::relative_eff`, with the effective sample size of `diagnostics` on the series of likelihoods
lik[t, c, i] = sigmoid(t) of every chain.  On the device the (steps, chains, rows) array is never formed: csrc/lik_stats.hip
fuses the logit contraction with the moment and lag sums of csrc/chain_stats.hip.
"""
import numpy as np

from . import _ffi, diagnostics
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace
from .diagnostics import Summary

MAX_DEVICE_ROWS = 1 << 20     # l2hmc_pack_logistic
MAX_DEVICE_DIM = 128
HIGH_VARIANCE = 0.4
_HOST_CHUNK_ELEMS = 1 << 22   # (draws x rows) logits formed at a time on the host
KHAT_BAD = 0.7                # PSIS is unreliable above it whatever S is
MIN_TAIL_FIT = 5              # a shorter tail is not fitted: khat = +inf
_FINISH_CHUNK_BYTES = 1 << 26  # the (rows, theta grid, tail) block of the Pareto profile formed at a time by `loo_finish`
_REFF_BYTES = 256 << 20       # the (chains, rows) moments and the lag-sum workspace of one `relative_eff` launch
_NEG_ZERO_KEY = -5e-324       # stands for -0.0 on the host so that a float64 sort puts it before +0.0, as the device order does


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


def _device_packer(dev, X, y, n, d, who):
    """`pack(a, m)`: rows [a, a + m) of (X, y) on `dev` as `l2hmc_pack_logistic` packs them.  The limits are checked, the data
    moved and the labels validated once, here (y=None: zeros, which need no look and so no device synchronisation)."""
    import torch
    if n > MAX_DEVICE_ROWS or d > MAX_DEVICE_DIM:
        raise ValueError("%s n_rows <= %d and dim <= %d (got %d, %d)" % (who, MAX_DEVICE_ROWS, MAX_DEVICE_DIM, n, d))
    Xd = torch.as_tensor(X).detach().to(device=dev, dtype=torch.float32).contiguous()
    if y is None:
        yd = torch.zeros(n, dtype=torch.float32, device=dev)
    else:
        yd = torch.as_tensor(y).detach().to(device=dev, dtype=torch.float32).contiguous()
        if not bool(((yd == 0) | (yd == 1)).all()):
            raise ValueError("labels y must be 0 or 1")
    L = _ffi.lib()

    def pack(a, m):
        packed = workspace(dev, torch.float32, L.l2hmc_packed_logistic_floats, m, d)
        launch(dev, L.l2hmc_pack_logistic, Xd[a:a + m].data_ptr(), yd[a:a + m].data_ptr(), m, d, packed.data_ptr())
        return packed
    return pack


def _device_sums(draws, X, y, S, d, n):
    import torch
    dev = draws.device
    packed = _device_packer(dev, X, y, n, d, "the predictive kernel holds")(0, n)
    W = in_place(draws)
    L = _ffi.lib()
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


def loo_tail_len(S):
    """M = min(S // 5, ceil(3 sqrt S)): how many of the largest importance ratios PSIS may fit and smooth."""
    import math
    S = int(S)
    return min(S // 5, math.isqrt(9 * S - 1) + 1) if S >= 1 else 0


def tail_len_rows(r_eff, S):
    """M_i = min(S // 5, ceil(3 sqrt(S / r_eff_i))) (n,) int64, in float64 on the host: the tail length `loo` prescribes for a
    row whose draws have relative efficiency r_eff_i; a NaN or non-positive r_eff_i counts as 1."""
    r = np.asarray(r_eff, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(np.isfinite(r) & (r > 0), r, 1.0)
        return np.minimum(float(int(S) // 5), np.ceil(3.0 * np.sqrt(int(S) / r))).astype(np.int64)


def _check_lengths(tail_len_row, n, S):
    lens = np.ascontiguousarray(as_numpy(tail_len_row), dtype=np.int64)
    if lens.shape != (n,) or np.any(lens < 0) or np.any(lens >= S):
        raise ValueError("tail_len_row must be (n_rows,) = (%d,) integers in 0 .. n_draws - 1" % n)
    return lens


def _device_tail_groups(draws, X, y, S, d, n, max_tail_bytes, tail_len_row=None):
    """The raw dict of one group of consecutive rows at a time, on the device; a group's tail stays under `max_tail_bytes`.
    `tail_len_row` (n,) int64: a tail length per row (`l2hmc_logistic_loo_tails_mc`); the dict gains 'body_sq' and
    'tail_len_row', and 'tail_len' is the largest length."""
    import torch
    dev = draws.device
    pack = _device_packer(dev, X, y, n, d, "the LOO kernels hold")
    W = in_place(draws)
    L = _ffi.lib()
    if tail_len_row is not None:
        yield from _device_tail_groups_mc(dev, pack, W, L, S, d, n, max_tail_bytes, tail_len_row)
        return
    M = _ffi.check(L.l2hmc_logistic_loo_tail_len(S))
    rows = max(1, min(n, int(max_tail_bytes) // max(1, 4 * M), (1 << 31) // max(1, M)))
    flags = []                                               # every group's error word, read once after the last group
    for a in range(0, n, rows):
        m = min(rows, n - a)
        packed = pack(a, m)
        ws = workspace(dev, torch.uint8, L.l2hmc_logistic_loo_workspace_bytes, S, m, d)
        cutoff = torch.empty(m, dtype=torch.float32, device=dev)
        n_tail = torch.empty(m, dtype=torch.int64, device=dev)
        tail = torch.empty((m, M), dtype=torch.float32, device=dev)
        sums = torch.empty((2, m), dtype=torch.float64, device=dev)
        launch(dev, L.l2hmc_logistic_loo_tails, W.data_ptr(), S, d, packed.data_ptr(), m, cutoff.data_ptr(), n_tail.data_ptr(),
               tail.data_ptr() if M else None, sums.data_ptr(), ws.data_ptr())
        flags.append(ws[:8].view(torch.int64).clone())
        yield {"cutoff": cutoff, "n_tail": n_tail, "tail": tail, "body": sums[0], "sum_lik": sums[1], "tail_len": M, "n_draws": S}
    if bool(torch.cat(flags).any()):
        raise RuntimeError("l2hmc_logistic_loo_tails: a tail outgrew its %d slots: the passes disagree" % M)


def _device_tail_groups_mc(dev, pack, W, L, S, d, n, max_tail_bytes, lens):
    import torch
    M = int(lens.max()) if n else 0
    lens_d = torch.as_tensor(lens).to(dev)
    rows = max(1, min(n, int(max_tail_bytes) // max(1, 4 * M), (1 << 31) // max(1, M)))
    flags = []
    for a in range(0, n, rows):
        m = min(rows, n - a)
        packed = pack(a, m)
        ws = workspace(dev, torch.uint8, L.l2hmc_logistic_loo_mc_workspace_bytes, S, m, d)
        cutoff = torch.empty(m, dtype=torch.float32, device=dev)
        n_tail = torch.empty(m, dtype=torch.int64, device=dev)
        tail = torch.empty((m, M), dtype=torch.float32, device=dev)
        sums = torch.empty((3, m), dtype=torch.float64, device=dev)
        group = lens_d[a:a + m].contiguous()
        launch(dev, L.l2hmc_logistic_loo_tails_mc, W.data_ptr(), S, d, packed.data_ptr(), m, group.data_ptr(), M, cutoff.data_ptr(),
               n_tail.data_ptr(), tail.data_ptr() if M else None, sums.data_ptr(), ws.data_ptr())
        flags.append(ws[:8].view(torch.int64).clone())
        yield {"cutoff": cutoff, "n_tail": n_tail, "tail": tail, "body": sums[0], "sum_lik": sums[1], "body_sq": sums[2],
               "tail_len_row": group, "tail_len": M, "n_draws": S}
    if bool(torch.cat(flags).any()):
        raise RuntimeError("l2hmc_logistic_loo_tails_mc: a tail outgrew its slots: the passes disagree")


def _host_tails(draws, X, y, S, d, n, tail_len_row=None):
    """The same raw dict in float64 numpy: per row the M + 1 smallest signed logits are kept while the draws pass in chunks
    (a partition, not a sort), then one more pass over the draws adds the body and the likelihoods.  `tail_len_row` (n,): row i
    is cut at its own rank M_i (M is then the largest), and the dict gains 'body_sq' and 'tail_len_row'."""
    W = as_numpy(draws, np.float64).reshape(S, d)
    X = as_numpy(X, np.float64)
    y = as_numpy(y, np.float64)
    if not np.all((y == 0.0) | (y == 1.0)):
        raise ValueError("labels y must be 0 or 1")
    sign = 2.0 * y - 1.0
    M = loo_tail_len(S) if tail_len_row is None else (int(tail_len_row.max()) if n else 0)
    Mi = np.full(n, M, dtype=np.int64) if tail_len_row is None else tail_len_row
    step = max(1, _HOST_CHUNK_ELEMS // n)

    def logits(a):
        t = (W[a:a + step] @ X.T) * sign
        return np.where((t == 0.0) & np.signbit(t), _NEG_ZERO_KEY, t)             # the device order: -0 before +0

    with np.errstate(all="ignore"):
        low = np.empty((0, n))
        for a in range(0, S, step):
            low = np.concatenate([low, logits(a)])
            if low.shape[0] > M + 1:
                low = np.partition(low, M, axis=0)[:M + 1]                         # NaN sorts last, as on the device
        low = np.sort(low, axis=0)
        c = low[Mi, np.arange(n)]                                                  # the element of rank M_i of row i
        keep = (low[:M] < c) & (np.arange(M)[:, None] < Mi)                        # strictly before the cutoff
        n_tail = keep.sum(axis=0).astype(np.int64)
        tail = np.where(keep, low[:M], np.inf).T.copy()                            # (n, M): sorted, +inf past n_tail
        m = np.minimum(np.where(c != c, 0.0, c), 0.0)
        body, sum_lik, body_sq = np.zeros(n), np.zeros(n), np.zeros(n)
        for a in range(0, S, step):
            t = logits(a)
            rho = np.where(t < c, 0.0, np.exp(m) + np.exp(m - t))
            body += rho.sum(axis=0)
            if tail_len_row is not None:
                body_sq += (rho * rho).sum(axis=0)
            sum_lik += np.exp(-np.logaddexp(0.0, -t)).sum(axis=0)
    unkey = lambda v: np.where(v == _NEG_ZERO_KEY, -0.0, v)  # noqa: E731
    out = {"cutoff": unkey(c), "n_tail": n_tail, "tail": unkey(tail), "body": body, "sum_lik": sum_lik, "tail_len": M, "n_draws": S}
    if tail_len_row is not None:
        out.update(body_sq=body_sq, tail_len_row=tail_len_row)
    return out


def _check_loo(draws, X, y):
    if y is None:
        raise ValueError("loo needs the labels y")
    return _check(draws, X, y)


def loo_tails(draws, X, y, max_tail_bytes=256 << 20, tail_len_row=None):
    """The raw material of PSIS-LOO per row of X (module docstring): {'cutoff' (n,), 'n_tail' (n,) int64, 'tail' (n, M) with
    +inf past n_tail, 'body' (n,), 'sum_lik' (n,), 'tail_len': M, 'n_draws': S}.  A ROCm tensor of draws -> the HIP kernels,
    read in place, device tensors back (float32 cutoff and tail in any order, float64 sums; bitwise reproducible); the rows go
    in groups whose tail buffer stays under `max_tail_bytes`, and the bits do not depend on the grouping.  numpy or a CPU
    tensor -> float64 numpy arrays, the tail sorted.  `tail_len_row` (n,) integers (`tail_len_rows(r_eff, S)`): row i is cut at
    its own rank M_i instead of the single M; 'tail' is (n, max M_i), 'tail_len' that maximum, and the dict gains 'tail_len_row'
    and 'body_sq', the sum over the body of (e^m + e^(m - t))^2 (`l2hmc_logistic_loo_tails_mc` on the device)."""
    S, d, n = _check_loo(draws, X, y)
    if tail_len_row is not None:
        tail_len_row = _check_lengths(tail_len_row, n, S)
    if not is_device_tensor(draws):
        return _host_tails(draws, X, y, S, d, n, tail_len_row)
    import torch
    groups = list(_device_tail_groups(draws, X, y, S, d, n, max_tail_bytes, tail_len_row))
    keys = ("cutoff", "n_tail", "tail", "body", "sum_lik") + (("body_sq", "tail_len_row") if tail_len_row is not None else ())
    out = {k: torch.cat([g[k] for g in groups]) for k in keys}
    out["tail_len"], out["n_draws"] = groups[0]["tail_len"], S
    return out


class _Numpy:
    """The few array operations `_loo_rows` needs, over numpy ..."""
    def __init__(self):
        for k in ("exp", "log", "log1p", "expm1", "sqrt", "floor", "where", "isfinite", "minimum", "maximum", "isnan"):
            setattr(self, k, getattr(np, k))

    def f64(self, a):
        return np.asarray(a, dtype=np.float64)

    def arange(self, n, like):
        return np.arange(n, dtype=np.float64)

    def sort(self, a):
        return np.sort(a, axis=-1)

    def sum(self, a):
        return a.sum(axis=-1)

    def max(self, a):
        return a.max(axis=-1) if a.shape[-1] else np.full(a.shape[:-1], -np.inf)

    def take(self, a, idx):
        return np.take_along_axis(a, idx.astype(np.int64)[..., None], axis=-1)[..., 0]

    def host(self, a):
        return np.asarray(a)


class _Torch:
    """... and over torch, on the device of the tails."""
    def __init__(self):
        import torch
        self.t = torch
        for k in ("exp", "log", "log1p", "expm1", "sqrt", "floor", "where", "isfinite", "minimum", "maximum", "isnan"):
            setattr(self, k, getattr(torch, k))

    def f64(self, a):
        return a.to(self.t.float64)

    def arange(self, n, like):
        return self.t.arange(n, dtype=self.t.float64, device=like.device)

    def sort(self, a):
        return self.t.sort(a, dim=-1).values

    def sum(self, a):
        return a.sum(dim=-1)

    def max(self, a):
        return a.amax(dim=-1) if a.shape[-1] else self.t.full(a.shape[:-1], -float("inf"), dtype=a.dtype, device=a.device)

    def take(self, a, idx):
        return self.t.gather(a, -1, idx.to(self.t.int64).unsqueeze(-1)).squeeze(-1)

    def host(self, a):
        return a.cpu().numpy()


def _softplus_neg(xp, v):
    """softplus(-v) = log(1 + e^-v)"""
    return xp.maximum(-v, v * 0.0) + xp.log1p(xp.exp(-xp.maximum(v, -v)))


def _lse(xp, a, zero):
    """logsumexp over the last axis; -inf when empty"""
    mx = xp.max(a)
    mx = xp.where(xp.isfinite(mx), mx, xp.where(xp.isnan(mx), mx, zero))              # centre: 0 for an empty (-inf) row
    return mx + xp.log(xp.sum(xp.exp(a - mx[..., None])))


def _logaddexp(xp, a, b, zero):
    """logaddexp of two (rows,) arrays"""
    mx = xp.maximum(a, b)
    mx = xp.where(xp.isfinite(mx), mx, xp.where(xp.isnan(mx), mx, zero))
    return mx + xp.log(xp.exp(a - mx) + xp.exp(b - mx))


def _loo_prepare(xp, cutoff, n_tail, tail):
    """The first seam of `_loo_rows`: (c, L, lam_c, lam) float64 of a chunk of rows -- the tail sorted so that t ascends (the
    +inf pads last), lam = softplus(-t) descending with 0 in the pads."""
    c, Lf = xp.f64(cutoff), xp.f64(n_tail)
    t = xp.sort(xp.f64(tail))                                                      # the +inf pads last
    return c, Lf, _softplus_neg(xp, c), _softplus_neg(xp, t)


def _psis_rows(xp, lam, Lf, lam_c, M):
    """The middle of `_loo_rows`, and the host form of `psis.smooth_tails` (csrc/psis.hip restates it formula for formula):
    (khat, lam_max, lse_w, lse_wl, omega, live) of a chunk of rows whose (rows, M) log ratios `lam` descend over the L live
    slots; slot s < L holds the ratio of ascending rank j = L - s.  khat is the fitted shape or +inf where nothing was
    smoothed; omega (rows, M) is meaningful in the live slots only."""
    zero = Lf * 0.0
    slot = xp.arange(M, Lf)
    zeros = zero[:, None] + slot[None, :] * 0.0                                    # (rows, M)
    minus_inf = zeros - float("inf")
    live = slot[None, :] < Lf[:, None]
    j = Lf[:, None] - slot[None, :]                                                # ascending rank of the ratio, 1 .. L
    lam_max = xp.where(Lf > 0, lam[:, 0], lam_c) if M else lam_c
    floor_c = xp.exp(lam_c - lam_max)                                              # the cutoff's ratio over the largest one
    x = xp.where(live, xp.exp(lam - lam_max[:, None]) - floor_c[:, None], zeros)
    fit = Lf >= MIN_TAIL_FIT
    Ls = xp.where(fit, Lf, zero + MIN_TAIL_FIT)                                    # (a placeholder length where nothing is fitted)
    # Zhang & Stephens (2009) with the prior of `loo`: the profile likelihood on a grid of theta, theta's posterior mean
    jt = xp.arange(30 + int(np.floor(np.sqrt(max(M, 1)))), Lf) + 1.0
    m_theta = 30.0 + xp.floor(xp.sqrt(Ls))
    on_grid = jt[None, :] <= m_theta[:, None]
    if M:
        x_star = xp.take(x, xp.minimum(xp.maximum(Ls - xp.floor(Ls / 4.0 + 0.5), zero), zero + (M - 1)))   # rank floor(L/4 + 0.5)
        x_top = x[:, 0]
    else:
        x_star = x_top = zero
    theta = 1.0 / x_top[:, None] + (1.0 - xp.sqrt(m_theta[:, None] / (jt[None, :] - 0.5))) / (3.0 * x_star[:, None])
    kj = xp.sum(xp.where(live[:, None, :], xp.log1p(-theta[:, :, None] * x[:, None, :]), zeros[:, None, :])) / Ls[:, None]
    ell = xp.where(on_grid, Ls[:, None] * (xp.log(-theta / kj) - kj - 1.0), theta * 0.0 - float("inf"))
    wj = xp.exp(ell - _lse(xp, ell, zero)[:, None])                                # = 1 / sum_j' exp(ell_j' - ell_j)
    theta_hat = xp.sum(xp.where(on_grid, theta * wj, theta * 0.0))
    k = xp.sum(xp.where(live, xp.log1p(-theta_hat[:, None] * x), zeros)) / Ls
    sigma = -k / theta_hat
    k = (k * Ls + 5.0) / (Ls + 10.0)
    smooth = fit & xp.isfinite(k) & xp.isfinite(sigma)
    lp = xp.log1p(-xp.where(live, (j - 0.5) / Ls[:, None], zeros))                 # log(1 - p_j)
    ks = xp.where(smooth & (k != 0.0), k, zero + 1.0)[:, None]
    qj = xp.where((k == 0.0)[:, None], -sigma[:, None] * lp, sigma[:, None] * xp.expm1(-ks * lp) / ks)
    omega = xp.where(smooth[:, None], xp.minimum(xp.log(qj + floor_c[:, None]), zeros), lam - lam_max[:, None])
    lse_wl = _lse(xp, xp.where(live, omega - lam, minus_inf), zero)
    lse_w = _lse(xp, xp.where(live, omega, minus_inf), zero)
    khat = xp.where(smooth, k, zero + float("inf"))
    return khat, lam_max, lse_w, lse_wl, omega, live


def _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S):
    """The last seam of `_loo_rows`: the O(rows) numbers into (khat, elpd_loo_i, lppd_i)."""
    zero = Lf * 0.0
    m = xp.minimum(xp.where(xp.isnan(c), zero, c), zero)
    num = _logaddexp(xp, xp.log(S - Lf) - lam_max, lse_wl, zero)
    den = _logaddexp(xp, xp.log(xp.f64(body)) - m - lam_max, lse_w, zero)
    elpd = num - den
    khat = xp.where(xp.isnan(elpd), elpd, khat)                                    # a NaN draw makes the row NaN, quietly
    return khat, elpd, xp.log(xp.f64(sum_lik) / S)


def _loo_rows(xp, cutoff, n_tail, tail, body, sum_lik, S, M):
    """(khat, elpd_loo_i, lppd_i) of a chunk of rows, float64, over the operations of `xp` alone: prepare lam / fit and smooth
    / combine.  The tail is sorted so that t ascends: slot s < L holds the ratio of ascending rank j = L - s, and slot 0 the
    largest."""
    c, Lf, lam_c, lam = _loo_prepare(xp, cutoff, n_tail, tail)
    khat, lam_max, lse_w, lse_wl, _, _ = _psis_rows(xp, lam, Lf, lam_c, M)
    return _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S)


def _loo_summary(khat, elpd_i, lppd_i, n_tail, S, M):
    n = elpd_i.shape[0]
    with np.errstate(all="ignore"):
        p_loo_i = lppd_i - elpd_i
        elpd, p_loo, lppd = float(elpd_i.sum()), float(p_loo_i.sum()), float(lppd_i.sum())
        se = float(np.sqrt(n * elpd_i.var(ddof=1))) if n > 1 else float("nan")
        threshold = min(1.0 - 1.0 / np.log10(S), KHAT_BAD)
    return Summary(elpd_loo_i=elpd_i, p_loo_i=p_loo_i, lppd_i=lppd_i, khat=khat, n_tail=n_tail, elpd_loo=elpd, p_loo=p_loo,
                   lppd=lppd, looic=-2.0 * elpd, se=se, khat_threshold=threshold, n_bad=int(np.sum(khat > KHAT_BAD)),
                   n_above_threshold=int(np.sum(khat > threshold)), tail_len=M, n_draws=S, n_rows=n,
                   n_underflow=int(np.sum(np.isneginf(lppd_i))))


def _row_chunks(tails, rows_for, middle, extra=()):
    """(khat, elpd_loo_i, lppd_i, n_tail) as float64 / int64 numpy of one raw dict: `middle(xp, cutoff, n_tail, tail, body,
    sum_lik, S, M)` on chunks of `rows_for(M)` rows, computed where the tails lie; only these O(n) numbers come to the host.
    `extra`: further per-row entries of the dict handed to `middle` after sum_lik; every array `middle` returns comes back,
    n_tail last."""
    S, M = int(tails["n_draws"]), int(tails["tail_len"])
    if S < 2:
        raise ValueError("PSIS-LOO needs >= 2 draws (got %d)" % S)
    xp = _Torch() if is_device_tensor(tails["tail"]) else _Numpy()
    keys = ("cutoff", "n_tail", "tail", "body", "sum_lik") + tuple(extra)
    arrays = [tails[k] if isinstance(xp, _Torch) else np.asarray(tails[k]) for k in keys]
    n, rows = int(arrays[0].shape[0]), max(1, rows_for(M))
    out = [[] for _ in range(3 + len(extra))]
    with np.errstate(all="ignore"):
        for a in range(0, n, rows):
            for o, r in zip(out, middle(xp, *(v[a:a + rows] for v in arrays), S, M)):
                o.append(xp.host(r))
    return tuple(np.concatenate(o) for o in out) + (np.asarray(xp.host(arrays[1]), dtype=np.int64),)


def _finish_rows(tails):
    """`_loo_rows` in row chunks of bounded memory: the (rows, theta grid, tail) block of the Pareto profile."""
    n_theta = lambda M: 30 + int(np.floor(np.sqrt(max(M, 1))))  # noqa: E731
    return _row_chunks(tails, lambda M: _FINISH_CHUNK_BYTES // (8 * n_theta(M) * max(M, 1)), _loo_rows)


def _check_finish(finish, on_device):
    if finish not in ("torch", "kernel"):
        raise ValueError('finish is "torch" or "kernel" (got %r)' % (finish,))
    if finish == "kernel" and not on_device:
        raise ValueError('finish="kernel" runs the Pareto fit of csrc/psis.hip where the tails lie, on a ROCm device; these are '
                         'host data (numpy or a CPU tensor), which float64 numpy finishes: leave finish="torch"')


_KERNEL_FINISH_BYTES = 1 << 28  # the float64 (rows, M) log ratios formed at a time by the kernel finish


def _loo_rows_kernel(xp, cutoff, n_tail, tail, body, sum_lik, S, M):
    """`_loo_rows` with the middle on csrc/psis.hip: `torch.sort` of the float32 tail, lam = softplus(-t) in float64 torch,
    `psis.smooth_tails`, and the O(n) combine."""
    from .psis import smooth_tails
    c, Lf, lam_c, lam = _loo_prepare(xp, cutoff, n_tail, tail)
    khat, lse_w, lse_wl = smooth_tails(lam, n_tail, lam_c)
    lam_max = xp.where(Lf > 0, lam[:, 0], lam_c) if M else lam_c
    return _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S)


def _finish_rows_kernel(tails):
    """`_finish_rows` of device tails by `_loo_rows_kernel`, in row chunks of bounded memory (the float64 (rows, M) log ratios),
    whose bits do not depend on the chunking."""
    return _row_chunks(tails, lambda M: _KERNEL_FINISH_BYTES // (8 * max(M, 1)), _loo_rows_kernel)


def _mc_extras(xp, elpd, lam_max, lse_w, omega, live, lam, c, Lf, body, body_sq, r_eff, S):
    """(n_eff_i, mcse_elpd_loo_i) of a chunk of rows (module docstring, "Monte Carlo error"), relative to the row's largest
    ratio e^lam_max as `_loo_combine` works: every weight is then <= 1 and their sum Z lies in [1, S]."""
    zero = Lf * 0.0
    m = xp.minimum(xp.where(xp.isnan(c), zero, c), zero)
    body, body_sq, r_eff = xp.f64(body), xp.f64(body_sq), xp.f64(r_eff)
    Z2 = xp.exp(2.0 * _logaddexp(xp, xp.log(body) - m - lam_max, lse_w, zero))
    E = xp.exp(elpd)
    zeros = zero[:, None] + xp.arange(lam.shape[-1], Lf)[None, :] * 0.0       # (omega and lam are not finite in the dead slots)
    w2 = xp.where(live, xp.exp(2.0 * omega), zeros)
    n_eff = r_eff * Z2 / (xp.exp(-2.0 * (m + lam_max)) * body_sq + xp.sum(w2))
    v_body = xp.exp(-2.0 * lam_max) * ((S - Lf) - 2.0 * E * xp.exp(-m) * body + E * E * xp.exp(-2.0 * m) * body_sq)
    v_tail = xp.sum(xp.where(live, w2 * (xp.exp(-lam) - E[:, None]) ** 2, zeros))
    mcse = xp.sqrt((xp.maximum(v_body, zero) + v_tail) / Z2 / r_eff) / E
    return n_eff, mcse


def _loo_rows_mc(xp, cutoff, n_tail, tail, body, sum_lik, body_sq, r_eff, S, M):
    """`_loo_rows` plus (n_eff_i, mcse_elpd_loo_i): the rows' tails have their own lengths, which `_psis_rows` takes per row."""
    c, Lf, lam_c, lam = _loo_prepare(xp, cutoff, n_tail, tail)
    khat, lam_max, lse_w, lse_wl, omega, live = _psis_rows(xp, lam, Lf, lam_c, M)
    khat, elpd, lppd = _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S)
    return (khat, elpd, lppd) + _mc_extras(xp, elpd, lam_max, lse_w, omega, live, lam, c, Lf, body, body_sq, r_eff, S)


def _loo_rows_mc_kernel(xp, cutoff, n_tail, tail, body, sum_lik, body_sq, r_eff, S, M):
    """`_loo_rows_mc` with the middle on csrc/psis.hip (`psis.smooth_tails(weights=True)` returns omega from the kernel)."""
    from .psis import smooth_tails
    c, Lf, lam_c, lam = _loo_prepare(xp, cutoff, n_tail, tail)
    khat, lse_w, lse_wl, omega = smooth_tails(lam, n_tail, lam_c, weights=True)
    lam_max = xp.where(Lf > 0, lam[:, 0], lam_c) if M else lam_c
    live = xp.arange(M, Lf)[None, :] < Lf[:, None]
    khat, elpd, lppd = _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S)
    return (khat, elpd, lppd) + _mc_extras(xp, elpd, lam_max, lse_w, omega, live, lam, c, Lf, body, body_sq, r_eff, S)


def _finish_rows_mc(tails, r_eff, finish):
    """(khat, elpd_loo_i, lppd_i, n_eff_i, mcse_i, n_tail) of a raw dict with per-row tails and 'body_sq'."""
    if "body_sq" not in tails:
        raise ValueError("r_eff needs tails with per-row lengths: loo_tails(..., tail_len_row=tail_len_rows(r_eff, S))")
    r = np.asarray(r_eff, dtype=np.float64)
    if is_device_tensor(tails["tail"]):
        import torch
        r = torch.as_tensor(r).to(tails["tail"].device)
    n_theta = lambda M: 30 + int(np.floor(np.sqrt(max(M, 1))))  # noqa: E731
    if finish == "kernel":
        return _row_chunks(dict(tails, r_eff=r), lambda M: _KERNEL_FINISH_BYTES // (8 * max(M, 1)), _loo_rows_mc_kernel,
                           extra=("body_sq", "r_eff"))
    return _row_chunks(dict(tails, r_eff=r), lambda M: _FINISH_CHUNK_BYTES // (8 * n_theta(M) * max(M, 1)), _loo_rows_mc,
                       extra=("body_sq", "r_eff"))


def _mc_fields(s, r_eff, n_eff, mcse, lens):
    """The fields `r_eff` adds to the Summary of `_loo_summary`."""
    r = np.asarray(r_eff, dtype=np.float64)
    with np.errstate(all="ignore"):
        total = float(np.sqrt(np.sum(mcse * mcse))) if not np.any(s.khat > KHAT_BAD) else float("nan")
        low = float(np.nanmin(n_eff)) if np.any(~np.isnan(n_eff)) else float("nan")
    s.update(r_eff=r, n_eff=n_eff, min_n_eff=low, mcse_elpd_loo_i=mcse, mcse_elpd_loo=total, n_reff_nan=int(np.isnan(r).sum()),
             tail_len_row=np.asarray(lens, dtype=np.int64))
    return s


def _check_r_eff(r_eff, n):
    r = as_numpy(r_eff, np.float64)
    if r.shape != (n,):
        raise ValueError("r_eff is None, \"auto\" or an array (n_rows,) = (%d,); got shape %s" % (n, r.shape))
    with np.errstate(invalid="ignore"):
        return np.where(r > 0, r, np.nan)                    # an entry that is not a positive number is no efficiency: NaN


def loo_finish(tails, finish="torch", r_eff=None):
    """The `Summary` of `loo_tails`' result: per row `elpd_loo_i`, `p_loo_i`, `lppd_i`, `khat`, `n_tail`; the totals `elpd_loo`,
    `p_loo`, `lppd`, `looic` = -2 elpd_loo, `se` = sqrt(n var_i elpd_loo_i) (NaN for one row); `khat_threshold` =
    min(1 - 1 / log10 S, 0.7), `n_bad` = #{khat > 0.7}, `n_above_threshold`; `tail_len`, `n_draws`, `n_rows`, `n_underflow`.
    A tail shorter than 5 (or a fit that is not finite) is not smoothed and has khat = +inf.  `finish="kernel"` (device tails
    only; opt-in) fits and smooths on the fused float64 kernels of csrc/psis.hip instead of chunked torch: the same formulas,
    another summation order.  `r_eff` (n,): the tails were cut at `tail_len_rows(r_eff, S)` (`loo_tails(tail_len_row=)`), and the
    Summary gains the Monte Carlo fields of `loo`."""
    _check_finish(finish, is_device_tensor(tails["tail"]))
    if r_eff is not None:
        r = _check_r_eff(r_eff, int(tails["cutoff"].shape[0]))
        khat, elpd_i, lppd_i, n_eff, mcse, n_tail = _finish_rows_mc(tails, r, finish)
        s = _loo_summary(khat, elpd_i, lppd_i, n_tail, int(tails["n_draws"]), int(tails["tail_len"]))
        return _mc_fields(s, r, n_eff, mcse, as_numpy(tails["tail_len_row"]))
    khat, elpd_i, lppd_i, n_tail = (_finish_rows_kernel if finish == "kernel" else _finish_rows)(tails)
    return _loo_summary(khat, elpd_i, lppd_i, n_tail, int(tails["n_draws"]), int(tails["tail_len"]))


def loo(draws, X, y, max_tail_bytes=256 << 20, finish="torch", r_eff=None):
    """PSIS-LOO of the logistic regression (X, y) under the posterior draws: `loo_finish(loo_tails(draws, X, y))`, except that
    on the device every group of rows is finished before the next one's tails are formed, so that no more than
    `max_tail_bytes` of tails exist at a time.  Compare two models on the same rows by `elpd_loo` (higher is better) against
    `se`; rows with khat > 0.7 (`n_bad`) are where the estimate cannot be trusted.  `finish`: see `loo_finish`.

    `r_eff`: None treats the draws as independent (one tail length M, the fields above).  "auto" (a history (steps, chains,
    dim) only) takes `relative_eff(draws, X, y).r_eff`; an array (n,) is used as given.  Row i's tail is then M_i =
    min(S // 5, ceil(3 sqrt(S / r_eff_i))) long (`tail_len_row`; `tail_len` is the largest; a NaN or non-positive r_eff_i
    counts as 1 there, is reported as NaN in `r_eff` and counted in `n_reff_nan`) and the Summary gains, with w the normalised smoothed weights and E_i = sum_s w_s lik_s:
    `n_eff` = r_eff_i / sum_s w_s^2, `min_n_eff`, `mcse_elpd_loo_i` = sqrt(sum_s w_s^2 (lik_s - E_i)^2 / r_eff_i) / E_i -- the
    first-order (delta-method) Monte Carlo standard error of elpd_loo_i; `loo` pushes a normal approximation through the log
    instead, which agrees to first order and is not built -- `mcse_elpd_loo` = sqrt(sum_i mcse_i^2), NaN when any khat > 0.7 as
    `loo` reports NA there, `r_eff` and `n_reff_nan`; rows with NaN r_eff have NaN in both per-row fields.  The body's part of
    both sums comes from `body` and `body_sq` in the three-term form N_b - 2 E e^-m body + E^2 e^-2m body_sq (N_b draws
    outside the tail), the tail's from the smoothed weights the finish holds."""
    S, d, n = _check_loo(draws, X, y)
    _check_finish(finish, is_device_tensor(draws))
    if r_eff is not None:
        if isinstance(r_eff, str):
            if r_eff != "auto":
                raise ValueError('r_eff is None, "auto" or an array (n_rows,) (got %r)' % (r_eff,))
            r = _check_r_eff(relative_eff(draws, X, y).r_eff, n)
        else:
            r = _check_r_eff(r_eff, n)
        lens = tail_len_rows(r, S)
        if not is_device_tensor(draws):
            return loo_finish(_host_tails(draws, X, y, S, d, n, lens), r_eff=r)
        parts, a = [], 0
        for g in _device_tail_groups(draws, X, y, S, d, n, max_tail_bytes, lens):
            m = int(g["cutoff"].shape[0])
            parts.append(_finish_rows_mc(g, r[a:a + m], finish))
            a += m
        khat, elpd_i, lppd_i, n_eff, mcse, n_tail = (np.concatenate([p[k] for p in parts]) for k in range(6))
        return _mc_fields(_loo_summary(khat, elpd_i, lppd_i, n_tail, S, int(lens.max())), r, n_eff, mcse, lens)
    if not is_device_tensor(draws):
        return loo_finish(_host_tails(draws, X, y, S, d, n))
    rows_of = _finish_rows_kernel if finish == "kernel" else _finish_rows
    parts = [rows_of(g) for g in _device_tail_groups(draws, X, y, S, d, n, max_tail_bytes)]
    khat, elpd_i, lppd_i, n_tail = (np.concatenate([p[k] for p in parts]) for k in range(4))
    return _loo_summary(khat, elpd_i, lppd_i, n_tail, S, loo_tail_len(S))


def _reff_device(draws, X, y, M, N, d, n, Mh, C, max_lag, split, max_bytes):
    """`diagnostics.finish` of every group of consecutive rows, on the sums of `l2hmc_logistic_lik_stats`; a group's moments
    and workspace stay under `max_bytes`."""
    import torch
    dev = draws.device
    pack = _device_packer(dev, X, y, n, d, "the likelihood-statistics kernels hold")
    W = in_place(draws)
    L = _ffi.lib()
    shape = (M, N, d)
    per_row = 16 * C + _ffi.check(L.l2hmc_logistic_lik_stats_workspace_bytes(*shape, 1, max_lag, int(split)))
    rows = max(1, min(n, int(max_bytes) // per_row))
    for a in range(0, n, rows):
        m = min(rows, n - a)
        packed = pack(a, m)
        ws = workspace(dev, torch.uint8, L.l2hmc_logistic_lik_stats_workspace_bytes, *shape, m, max_lag, int(split))
        mean = torch.empty((C, m), dtype=torch.float64, device=dev)
        m2 = torch.empty((C, m), dtype=torch.float64, device=dev)
        G = torch.empty((m, max_lag + 1), dtype=torch.float64, device=dev)
        launch(dev, L.l2hmc_logistic_lik_stats, W.data_ptr(), *shape, packed.data_ptr(), m, max_lag, int(split), mean.data_ptr(),
               m2.data_ptr(), G.data_ptr(), ws.data_ptr())
        yield diagnostics.finish({"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C})


def _reff_host(draws, X, y, M, N, d, n, Mh, C, max_lag, split):
    """The same in float64 numpy, a chunk of rows at a time: the likelihoods of the chunk as a history (steps, chains, rows)
    through `diagnostics`' host sums."""
    W = as_numpy(draws, np.float64).reshape(M * N, d)
    X = as_numpy(X, np.float64)
    y = as_numpy(y, np.float64)
    if not np.all((y == 0.0) | (y == 1.0)):
        raise ValueError("labels y must be 0 or 1")
    sign = 2.0 * y - 1.0
    rows = max(1, _HOST_CHUNK_ELEMS // (M * N))
    for a in range(0, n, rows):
        with np.errstate(all="ignore"):
            lik = np.exp(-np.logaddexp(0.0, -(W @ X[a:a + rows].T) * sign[a:a + rows])).reshape(M, N, -1)
        mean, m2, G = diagnostics._host_sums(lik, Mh, max_lag, split)
        series = np.concatenate([lik[:Mh], lik[M - Mh:]], axis=1) if split else lik
        with np.errstate(invalid="ignore"):                  # a constant series has M2 = 0 exactly, whatever its mean rounds to
            m2 = np.where(series.max(axis=0) == series.min(axis=0), 0.0, m2)
        yield diagnostics.finish({"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C})


def relative_eff(draws, X, y, max_lag=None, split=False, max_bytes=_REFF_BYTES):
    """The per-row relative efficiency of the likelihoods under a recorded history `draws` (steps, chains, dim):
    r_eff_i = ess_i / S with S = steps x chains and ess_i the effective sample size of `diagnostics` (its `finish`, on the chain
    sums of the series lik[t, c, i] = P(y_i | x_i, w[t, c])) -- what `loo::relative_eff` computes from whole chains, hence
    `split=False` by default; `max_lag=None` is min(steps per chain - 1, `diagnostics.DEFAULT_MAX_LAG`).  A `Summary` of
    `r_eff`, `ess` (n,), `truncated` (n,) bool -- no non-positive pair of autocorrelations within `max_lag`: ask for more lags
    -- `n_truncated`, `n_nan` (rows whose series is constant or not finite: r_eff = NaN), `n_draws`, `n_steps`, `n_chains`,
    `max_lag`.  A ROCm history goes to the kernels behind `l2hmc_logistic_lik_stats` (csrc/lik_stats.hip), read in place, the
    rows in groups whose moments and workspace stay under `max_bytes` (the bits do not depend on the grouping); numpy or a CPU
    tensor is float64 numpy, a chunk of rows at a time.  A matrix (draws, dim) is refused: its chains are not known.
    A series whose values are all equal has M2 = 0 exactly on both routes, so a row whose every series is constant is NaN;
    `diagnostics.summarize` of the same likelihoods on the host keeps whatever its rounded mean leaves (see its docstring)."""
    if y is None:
        raise ValueError("relative_eff needs the labels y")
    M, N, _ = history_shape(draws, says="relative_eff needs a history (steps, chains, dim): the chains of a matrix of draws are "
                                        "not known")
    S, d, n = _check(draws, X, y)
    Mh, C, max_lag = diagnostics._shape(M, N, split, max_lag)
    if is_device_tensor(draws):
        parts = list(_reff_device(draws, X, y, M, N, d, n, Mh, C, max_lag, split, max_bytes))
    else:
        parts = list(_reff_host(draws, X, y, M, N, d, n, Mh, C, max_lag, split))
    ess = np.concatenate([p.ess for p in parts])
    truncated = np.concatenate([p.truncated for p in parts])
    return Summary(r_eff=ess / S, ess=ess, truncated=truncated, n_truncated=int(truncated.sum()), n_nan=int(np.isnan(ess).sum()),
                   n_draws=S, n_steps=Mh, n_chains=C, max_lag=max_lag)
