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

from . import _ffi, diagnostics, psis
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace
from ._pareto import (KHAT_BAD, MIN_TAIL_FIT, _Numpy, _Torch, _logaddexp, _loo_summary, _psis_rows, _se_rows,  # noqa: F401
                      _softplus_neg, lam_max, loo_tail_len, theta_grid_len)
from .diagnostics import Summary

MAX_DEVICE_ROWS = 1 << 20     # l2hmc_pack_logistic
MAX_DEVICE_DIM = 128
HIGH_VARIANCE = 0.4
_HOST_CHUNK_ELEMS = 1 << 22   # (draws x rows) logits formed at a time on the host
_FINISH_CHUNK_BYTES = 1 << 26  # the (rows, theta grid, tail) block of the Pareto profile formed at a time by `loo_finish`
_KERNEL_FINISH_BYTES = 1 << 28  # the float64 (rows, M) log ratios formed at a time by the kernel finish
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


def _row_groups(pack, n, rows):
    """(a, m, packed) of every group of at most `rows` consecutive rows [a, a + m), packed by `_device_packer`'s `pack`."""
    for a in range(0, n, rows):
        m = min(rows, n - a)
        yield a, m, pack(a, m)


def _device_sums(draws, X, y, S, d, n):
    import torch
    dev = draws.device
    (_, _, packed), = _row_groups(_device_packer(dev, X, y, n, d, "the predictive kernel holds"), n, n)
    W = in_place(draws)
    L = _ffi.lib()
    ws = workspace(dev, torch.float64, L.l2hmc_logistic_predict_workspace_doubles, S, n, d)
    sums = torch.empty((4, n), dtype=torch.float64, device=dev)
    launch(dev, L.l2hmc_logistic_predict, W.data_ptr(), S, d, packed.data_ptr(), n, sums.data_ptr(), ws.data_ptr())
    return sums.cpu().numpy()


def _host_inputs(draws, X, y, S, d, n):
    """(W (S, d), X (n, d), sign (n,) = 2 y - 1) in float64 numpy of host data; the labels are checked here (y=None: zeros)."""
    W = as_numpy(draws, np.float64).reshape(S, d)
    X = as_numpy(X, np.float64)
    y = np.zeros(n) if y is None else as_numpy(y, np.float64)
    if not np.all((y == 0.0) | (y == 1.0)):
        raise ValueError("labels y must be 0 or 1")
    return W, X, 2.0 * y - 1.0


def _host_sums(draws, X, y, S, d, n):
    W, X, sign = _host_inputs(draws, X, y, S, d, n)
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
        se = _se_rows(elpd_i)
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
        se = _se_rows(f.lppd_i)
    return Summary(lppd=f.lppd, lppd_i=f.lppd_i, se=se, n_draws=f.n_draws, n_rows=n, n_underflow=f.n_underflow)


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


def _device_tail_groups(draws, X, y, S, d, n, max_tail_bytes, lens=None):
    """The raw dict of one group of consecutive rows at a time, on the device; a group's tail stays under `max_tail_bytes`.
    `lens` (n,) int64: a tail length per row (`l2hmc_logistic_loo_tails_mc`, which has one more sum row); the dict gains
    'body_sq' and 'tail_len_row', and 'tail_len' is the largest length."""
    import torch
    dev = draws.device
    pack = _device_packer(dev, X, y, n, d, "the LOO kernels hold")
    W = in_place(draws)
    L = _ffi.lib()
    mc = lens is not None
    if mc:
        M = int(lens.max()) if n else 0
        lens_d = torch.as_tensor(lens).to(dev)
        entry, query = L.l2hmc_logistic_loo_tails_mc, L.l2hmc_logistic_loo_mc_workspace_bytes
        outgrew = "l2hmc_logistic_loo_tails_mc: a tail outgrew its slots: the passes disagree"
    else:
        M = _ffi.check(L.l2hmc_logistic_loo_tail_len(S))
        entry, query = L.l2hmc_logistic_loo_tails, L.l2hmc_logistic_loo_workspace_bytes
        outgrew = "l2hmc_logistic_loo_tails: a tail outgrew its %d slots: the passes disagree" % M
    rows = max(1, min(n, int(max_tail_bytes) // max(1, 4 * M), (1 << 31) // max(1, M)))
    flags = []                                               # every group's error word, read once after the last group
    for a, m, packed in _row_groups(pack, n, rows):
        ws = workspace(dev, torch.uint8, query, S, m, d)
        cutoff = torch.empty(m, dtype=torch.float32, device=dev)
        n_tail = torch.empty(m, dtype=torch.int64, device=dev)
        tail = torch.empty((m, M), dtype=torch.float32, device=dev)
        sums = torch.empty((3 if mc else 2, m), dtype=torch.float64, device=dev)
        group = lens_d[a:a + m].contiguous() if mc else None
        launch(dev, entry, W.data_ptr(), S, d, packed.data_ptr(), m, *((group.data_ptr(), M) if mc else ()), cutoff.data_ptr(),
               n_tail.data_ptr(), tail.data_ptr() if M else None, sums.data_ptr(), ws.data_ptr())
        flags.append(ws[:8].view(torch.int64).clone())
        out = {"cutoff": cutoff, "n_tail": n_tail, "tail": tail, "body": sums[0], "sum_lik": sums[1], "tail_len": M, "n_draws": S}
        if mc:
            out.update(body_sq=sums[2], tail_len_row=group)
        yield out
    if bool(torch.cat(flags).any()):
        raise RuntimeError(outgrew)


def _host_tails(draws, X, y, S, d, n, tail_len_row=None):
    """The same raw dict in float64 numpy: per row the M + 1 smallest signed logits are kept while the draws pass in chunks
    (a partition, not a sort), then one more pass over the draws adds the body and the likelihoods.  `tail_len_row` (n,): row i
    is cut at its own rank M_i (M is then the largest), and the dict gains 'body_sq' and 'tail_len_row'."""
    W, X, sign = _host_inputs(draws, X, y, S, d, n)
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


def _loo_prepare(xp, cutoff, n_tail, tail):
    """The first seam of `_loo_rows`: (c, L, lam_c, lam) float64 of a chunk of rows -- the tail sorted so that t ascends (the
    +inf pads last), lam = softplus(-t) descending with 0 in the pads."""
    c, Lf = xp.f64(cutoff), xp.f64(n_tail)
    t = xp.sort(xp.f64(tail))                                                      # the +inf pads last
    return c, Lf, _softplus_neg(xp, c), _softplus_neg(xp, t)


def _loo_combine(xp, khat, lam_max, lse_w, lse_wl, c, Lf, body, sum_lik, S):
    """The last seam of `_loo_rows`: the O(rows) numbers into (khat, elpd_loo_i, lppd_i)."""
    zero = Lf * 0.0
    m = xp.minimum(xp.where(xp.isnan(c), zero, c), zero)
    num = _logaddexp(xp, xp.log(S - Lf) - lam_max, lse_wl, zero)
    den = _logaddexp(xp, xp.log(xp.f64(body)) - m - lam_max, lse_w, zero)
    elpd = num - den
    khat = xp.where(xp.isnan(elpd), elpd, khat)                                    # a NaN draw makes the row NaN, quietly
    return khat, elpd, xp.log(xp.f64(sum_lik) / S)


def _mc_extras(xp, elpd, lam_max, lse_w, omega, live, lam, c, Lf, body, body_sq, r_eff, S):
    """(n_eff_i, mcse_elpd_loo_i) of a chunk of rows (`loo`'s docstring has the formulas), relative to the row's largest
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


def _middle_torch(xp, lam, n_tail, Lf, lam_c, M, mc):
    return _psis_rows(xp, lam, Lf, lam_c, M)


def _middle_kernel(xp, lam, n_tail, Lf, lam_c, M, mc):
    """The fit on csrc/psis.hip (`psis.smooth_tails`, which returns omega from the kernel only when the extras need it)."""
    res = psis.smooth_tails(lam, n_tail, lam_c, weights=mc)
    top = lam_max(xp, lam, Lf, lam_c, M)
    live = xp.arange(M, Lf)[None, :] < Lf[:, None] if mc else None
    return res[0], top, res[1], res[2], res[3] if mc else None, live


_MIDDLES = {"torch": _middle_torch, "kernel": _middle_kernel}


def _loo_rows(xp, middle, S, M, cutoff, n_tail, tail, body, sum_lik, body_sq=None, r_eff=None):
    """(khat, elpd_loo_i, lppd_i) of a chunk of rows, float64, over the operations of `xp` alone: prepare lam / fit and smooth
    (`middle`: a `_MIDDLES` entry, which returns (khat, lam_max, lse_w, lse_wl, omega, live)) / combine.  The tail is sorted so
    that t ascends: slot s < L holds the ratio of ascending rank j = L - s, and slot 0 the largest; the rows' tails may have
    their own lengths, which the fit takes per row.  With `body_sq` and `r_eff`: plus (n_eff_i, mcse_elpd_loo_i)."""
    mc = r_eff is not None
    c, Lf, lam_c, lam = _loo_prepare(xp, cutoff, n_tail, tail)
    khat, top, lse_w, lse_wl, omega, live = middle(xp, lam, n_tail, Lf, lam_c, M, mc)
    out = _loo_combine(xp, khat, top, lse_w, lse_wl, c, Lf, body, sum_lik, S)
    if mc:
        out += _mc_extras(xp, out[1], top, lse_w, omega, live, lam, c, Lf, body, body_sq, r_eff, S)
    return out


def _row_chunks(tails, rows_for, middle, extra=()):
    """(khat, elpd_loo_i, lppd_i, n_tail) as float64 / int64 numpy of one raw dict: `_loo_rows` with `middle` on chunks of
    `rows_for(M)` rows, computed where the tails lie; only these O(n) numbers come to the host.  `extra`: further per-row
    entries of the dict handed to `_loo_rows` after sum_lik; every array it returns comes back, n_tail last."""
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
            for o, r in zip(out, _loo_rows(xp, middle, S, M, *(v[a:a + rows] for v in arrays))):
                o.append(xp.host(r))
    return tuple(np.concatenate(o) for o in out) + (np.asarray(xp.host(arrays[1]), dtype=np.int64),)


def _finish_chunk_rows(finish, M):
    """The rows of one chunk, of bounded memory: the float64 (rows, M) log ratios of the kernel finish (whose bits do not depend
    on the chunking), the (rows, theta grid, tail) block of the Pareto profile of the torch and numpy one."""
    if finish == "kernel":
        return _KERNEL_FINISH_BYTES // (8 * max(M, 1))
    return _FINISH_CHUNK_BYTES // (8 * theta_grid_len(M) * max(M, 1))


def _finish_rows(tails, finish, r_eff=None):
    """(khat, elpd_loo_i, lppd_i, n_tail) of a raw dict by `finish`; with `r_eff` (per-row tails and 'body_sq' in the dict)
    (khat, elpd_loo_i, lppd_i, n_eff_i, mcse_i, n_tail)."""
    extra = ()
    if r_eff is not None:
        if "body_sq" not in tails:
            raise ValueError("r_eff needs tails with per-row lengths: loo_tails(..., tail_len_row=tail_len_rows(r_eff, S))")
        r = np.asarray(r_eff, dtype=np.float64)
        if is_device_tensor(tails["tail"]):
            import torch
            r = torch.as_tensor(r).to(tails["tail"].device)
        tails, extra = dict(tails, r_eff=r), ("body_sq", "r_eff")
    return _row_chunks(tails, lambda M: _finish_chunk_rows(finish, M), _MIDDLES[finish], extra)


def _check_finish(finish, on_device):
    if finish not in ("torch", "kernel"):
        raise ValueError('finish is "torch" or "kernel" (got %r)' % (finish,))
    if finish == "kernel" and not on_device:
        raise ValueError('finish="kernel" runs the Pareto fit of csrc/psis.hip where the tails lie, on a ROCm device; these are '
                         'host data (numpy or a CPU tensor), which float64 numpy finishes: leave finish="torch"')


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


def _loo_of(raws, finish, r, lens=None):
    """The `Summary` of the raw dicts `raws` of consecutive rows, each finished before the next is taken; `r` (n,) or None."""
    parts, a = [], 0
    for g in raws:
        m = int(g["cutoff"].shape[0])
        parts.append(_finish_rows(g, finish, None if r is None else r[a:a + m]))
        a += m
    cols = [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]
    s = _loo_summary(cols[0], cols[1], cols[2], cols[-1], int(g["n_draws"]), int(g["tail_len"]))
    return s if r is None else _mc_fields(s, r, cols[3], cols[4], as_numpy(g["tail_len_row"]) if lens is None else lens)


def loo_finish(tails, finish="torch", r_eff=None):
    """The `Summary` of `loo_tails`' result: per row `elpd_loo_i`, `p_loo_i`, `lppd_i`, `khat`, `n_tail`; the totals `elpd_loo`,
    `p_loo`, `lppd`, `looic` = -2 elpd_loo, `se` = sqrt(n var_i elpd_loo_i) (NaN for one row); `khat_threshold` =
    min(1 - 1 / log10 S, 0.7), `n_bad` = #{khat > 0.7}, `n_above_threshold`; `tail_len`, `n_draws`, `n_rows`, `n_underflow`.
    A tail shorter than 5 (or a fit that is not finite) is not smoothed and has khat = +inf.  `finish="kernel"` (device tails
    only; opt-in) fits and smooths on the fused float64 kernels of csrc/psis.hip instead of chunked torch: the same formulas,
    another summation order.  `r_eff` (n,): the tails were cut at `tail_len_rows(r_eff, S)` (`loo_tails(tail_len_row=)`), and the
    Summary gains the Monte Carlo fields of `loo`."""
    _check_finish(finish, is_device_tensor(tails["tail"]))
    r = None if r_eff is None else _check_r_eff(r_eff, int(tails["cutoff"].shape[0]))
    return _loo_of([tails], finish, r)


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
    r = lens = None
    if r_eff is not None:
        if isinstance(r_eff, str):
            if r_eff != "auto":
                raise ValueError('r_eff is None, "auto" or an array (n_rows,) (got %r)' % (r_eff,))
            r_eff = relative_eff(draws, X, y).r_eff
        r = _check_r_eff(r_eff, n)
        lens = tail_len_rows(r, S)
    if is_device_tensor(draws):
        return _loo_of(_device_tail_groups(draws, X, y, S, d, n, max_tail_bytes, lens), finish, r, lens)
    return _loo_of([_host_tails(draws, X, y, S, d, n, lens)], finish, r, lens)


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
    for a, m, packed in _row_groups(pack, n, rows):
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
    W, X, sign = _host_inputs(draws, X, y, M * N, d, n)
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
