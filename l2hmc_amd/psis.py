"""Pareto-smoothed importance sampling (PSIS; Vehtari, Simpson, Gelman, Yao, Gabry 2024) of ANY log importance ratios, and
PSIS-LOO of any model from its pointwise log-likelihood matrix -- the model-comparison counterpart of "any energy drops in as a
torch callable":

    s = psis(log_ratios)                  # (S, n) or (S,): draws first; float32 / float64, numpy or a ROCm tensor
    s.khat, s.n_tail, s.log_weights, s.log_sum, s.n_eff, s.n_bad, s.khat_threshold, s.n_above_threshold, s.tail_len, s.n_draws
    s = loo_from_log_lik(log_lik)         # (S, n): log p(y_i | theta_s); the fields of `predictive.loo`
    khat, lse_w, lse_wl = smooth_tails(lam, n_tail, lam_cutoff)        # the kernel itself, on prepared tails

Per column: M = `predictive.loo_tail_len(S)`, the cutoff is the (M + 1)-th largest ratio, the tail the ratios strictly above it
(ties at the cutoff shorten it, the rule of the `loo` package).  A tail of at least 5 is fitted with a generalised Pareto
distribution (Zhang & Stephens 2009 with the prior of `loo`) and its weights are replaced by the fitted quantiles, capped at the
largest raw weight; the fitted shape is the diagnostic khat (above 0.7: do not trust the estimate).  A shorter tail, or a fit
that is not finite, keeps its raw weights and has khat = +inf.

A ROCm tensor goes to the float64 HIP kernels behind `l2hmc_psis_smooth` (csrc/psis.hip): `torch.topk` finds the M + 1 largest
ratios of every column in order with their positions, the kernels fit and smooth, and every smoothed weight goes back to the
draw it belongs to; all else is torch on the same device.  numpy or a CPU tensor is float64 numpy, whose fit is
`_pareto._psis_rows` -- the very operations `predictive.loo` finishes with; the kernel restates them formula for formula.

Sums over the draws (`log_sum`, `n_eff`, elpd and lppd of `loo_from_log_lik`) are added by a fixed pairwise tree of elementwise
additions, which depends on S alone: a column gives the same bits whichever other columns share the call, so the results of
row groups concatenate to the result of one call bit for bit.  `loo_from_log_lik` is the SLOW path: it needs the (S, n) matrix,
which the caller forms (in row groups when it is large).  The fused `predictive.loo` of the logistic regression never forms it.

Not here: r_eff and the Monte-Carlo standard error of elpd_loo, moment matching, a fused selection for the generic matrix, ranks
that hold different draws (`sharding`)."""
import numpy as np

from . import _ffi
from ._history import as_numpy, is_device_tensor, launch, workspace
from ._pareto import _Numpy, _centre, _khat_fields, _loo_summary, _psis_rows, lam_max, loo_tail_len, ops_of, theta_grid_len
from .diagnostics import Summary

_HOST_CHUNK_BYTES = 1 << 26  # the (rows, theta grid, tail) block of the Pareto profile formed at a time on the host


def _host_smooth(lam, n_tail, lam_c, want_weights):
    xp = _Numpy()
    n, M = lam.shape
    rows = max(1, _HOST_CHUNK_BYTES // (8 * theta_grid_len(M) * max(M, 1)))
    out = [[], [], [], []]
    with np.errstate(all="ignore"):
        for a in range(0, n, rows):
            khat, _, lse_w, lse_wl, omega, live = _psis_rows(xp, lam[a:a + rows], xp.f64(n_tail[a:a + rows]), lam_c[a:a + rows], M)
            bad = np.isnan(lse_w) | np.isnan(lse_wl)
            res = (np.where(bad, np.nan, khat), lse_w, lse_wl, np.where(live, omega, -np.inf) if want_weights else omega[:, :0])
            for o, r in zip(out, res):
                o.append(r)
    return tuple(np.concatenate(o) for o in out)


def smooth_tails(lam, n_tail, lam_cutoff, weights=False):
    """The Pareto fit and tail smoothing of prepared tails: `lam` (n_rows, M) holds the L_i = n_tail[i] largest log ratios of
    row i, descending, in slots 0 .. L_i - 1 (the other slots are never read), `lam_cutoff` (n_rows,) the log ratio of the
    cutoff.  Returns (khat, lse_w, lse_wl) -- and omega (n_rows, M) with `weights=True` -- float64: omega_s is the smoothed log
    weight of slot s relative to the row's largest ratio (-inf in the dead slots), lse_w = logsumexp_s omega_s and
    lse_wl = logsumexp_s (omega_s - lam_s); both are -inf when L_i = 0.  A NaN among a row's live slots makes that row's
    outputs NaN.  ROCm tensors -> `l2hmc_psis_smooth` (bitwise reproducible; device tensors back); anything else -> float64
    numpy (`_pareto._psis_rows`)."""
    shape = tuple(int(v) for v in lam.shape)
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError("lam must be (n_rows, tail_len) with n_rows >= 1; got shape %s" % (shape,))
    n, M = shape
    for name, v in (("n_tail", n_tail), ("lam_cutoff", lam_cutoff)):
        if tuple(int(k) for k in v.shape) != (n,):
            raise ValueError("%s must be (n_rows,) = (%d,), got shape %s" % (name, n, tuple(v.shape)))
    if not is_device_tensor(lam):
        L = as_numpy(n_tail, np.int64)
        if np.any(L < 0) or np.any(L > M):
            raise ValueError("n_tail must lie in 0 .. tail_len = %d" % M)
        res = _host_smooth(as_numpy(lam, np.float64), L, as_numpy(lam_cutoff, np.float64), weights)
        return res if weights else res[:3]
    import torch
    dev = lam.device
    lam = lam.detach().to(torch.float64).contiguous()
    L = torch.as_tensor(n_tail).detach().to(device=dev, dtype=torch.int64).contiguous()
    lam_c = torch.as_tensor(lam_cutoff).detach().to(device=dev, dtype=torch.float64).contiguous()
    lib = _ffi.lib()
    ws = workspace(dev, torch.uint8, lib.l2hmc_psis_workspace_bytes, n, M)
    out = torch.empty((3, n), dtype=torch.float64, device=dev)
    omega = torch.empty((n, M), dtype=torch.float64, device=dev) if weights else None
    launch(dev, lib.l2hmc_psis_smooth, lam.data_ptr() if M else None, L.data_ptr(), lam_c.data_ptr(), n, M, out.data_ptr(),
           omega.data_ptr() if weights and M else None, ws.data_ptr())
    if bool(ws[:8].view(torch.int64).any()):
        raise RuntimeError("l2hmc_psis_smooth: an n_tail entry lies outside 0 .. tail_len = %d" % M)
    return (out[0], out[1], out[2], omega) if weights else (out[0], out[1], out[2])


def _tree_sum(a):
    """The sum over axis 0 by a fixed pairwise tree of elementwise additions: rows h .. onto rows 0 .., h = ceil(rows / 2),
    until one row is left.  The order depends on the number of rows alone, not on the other axes.  (0,) rows give 0."""
    if a.shape[0] == 0:
        return a.sum(0)
    a = a.clone() if hasattr(a, "clone") else a.copy()
    while a.shape[0] > 1:
        h = (a.shape[0] + 1) // 2
        a[:a.shape[0] - h] += a[h:]
        a = a[:h]
    return a[0]


def _lse0(a):
    """logsumexp over axis 0 (the draws) of float64 (S, n): `_pareto._lse`'s centring, `_tree_sum`'s order."""
    xp = ops_of(a)
    with np.errstate(all="ignore"):
        mx = _centre(xp, xp.max(a.T), 0.0)
        return mx + xp.log(_tree_sum(xp.exp(a - mx[None, :])))


def _select(r):
    """(lam (n, M) descending, n_tail (n,) int64, cutoff (n,), idx (M, n) positions of the M largest, M) of float (S, n) ratios."""
    S = int(r.shape[0])
    M = loo_tail_len(S)
    if hasattr(r, "topk"):
        import torch
        vals, idx = torch.topk(r, M + 1, dim=0, largest=True, sorted=True)
        vals = vals.to(torch.float64)
        cutoff, top, idx = vals[M], vals[:M], idx[:M]
        n_tail = (top > cutoff[None, :]).sum(0).to(torch.int64)
        return top.t().contiguous(), n_tail, cutoff.contiguous(), idx, M
    order = np.argsort(r, axis=0, kind="stable")[::-1][:M + 1]                     # NaN first, as torch.topk has it
    vals = np.take_along_axis(r, order, axis=0).astype(np.float64)
    cutoff, top, idx = vals[M], vals[:M], order[:M]
    with np.errstate(invalid="ignore"):
        n_tail = (top > cutoff[None, :]).sum(axis=0).astype(np.int64)
    return np.ascontiguousarray(top.T), n_tail, cutoff, idx, M


def _as_ratios(a, name):
    """(float (S, n) on the device or in numpy, was_1d)"""
    shape = tuple(int(v) for v in a.shape)
    if len(shape) not in (1, 2) or shape[0] < 1 or (len(shape) == 2 and shape[1] < 1):
        raise ValueError("%s must be (n_draws, n) or (n_draws,) with n_draws >= 1 and n >= 1; got shape %s" % (name, shape))
    if is_device_tensor(a):
        import torch
        a = a.detach()
        if a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float64)
    else:
        a = as_numpy(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
    return (a.reshape(shape[0], 1), True) if len(shape) == 1 else (a, False)


def _psis(r, want_weights):
    """khat, n_tail, lam_max (all (n,)), the (S, n) float64 smoothed log weights (or None), M -- where `r` lies."""
    lam, n_tail, cutoff, idx, M = _select(r)
    res = smooth_tails(lam, n_tail, cutoff, weights=want_weights)
    khat = res[0]
    xp = ops_of(r)
    top = lam_max(xp, lam, n_tail, cutoff, M)
    if not want_weights:
        return khat, n_tail, top, None, M
    omega = res[3]                                           # (n, M), slot s = the draw idx[s]
    with np.errstate(all="ignore"):
        lw = xp.f64(r) - top[None, :]
    if M and hasattr(r, "topk"):
        import torch
        live = torch.arange(M, device=r.device)[:, None] < n_tail[None, :]
        lw.scatter_(0, idx, torch.where(live, omega.t(), lw.gather(0, idx)))
    elif M:
        live = np.arange(M)[:, None] < n_tail[None, :]
        np.put_along_axis(lw, idx, np.where(live, omega.T, np.take_along_axis(lw, idx, axis=0)), axis=0)
    return khat, n_tail, top, lw, M


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def psis(log_ratios, weights=True):
    """PSIS of log importance ratios (S, n) -- or (S,) for one set of weights -- float32 or float64, numpy or a ROCm tensor.
    A `Summary`: `khat` (n,), `n_tail` (n,), `tail_len`, `n_draws`, `n_bad` = #{khat > 0.7}, `khat_threshold` =
    min(1 - 1 / log10 S, 0.7), `n_above_threshold`; `log_weights` (S, n) float64, the smoothed log weights shifted so that the
    largest RAW ratio of a column is 0 (not normalised: a smoothed tail weight never exceeds it), `log_sum` (n,) =
    logsumexp over the draws of `log_weights` (so `log_weights - log_sum` are the normalised ones) and `n_eff` (n,) =
    exp(2 lse(w) - lse(2 w)), the importance-sampling effective sample size.  A 1-d input gives `log_weights` (S,) and the
    other arrays of length 1.  Device input: `log_weights` stays a device tensor, everything else comes to the host.
    `weights=False` skips the matrix (and `log_sum`, `n_eff`): khat alone."""
    r, flat = _as_ratios(log_ratios, "log_ratios")
    S = int(r.shape[0])
    khat, n_tail, _, lw, M = _psis(r, weights)
    khat, n_tail = _host(khat), _host(n_tail).astype(np.int64)
    out = dict(khat=khat, n_tail=n_tail, tail_len=M, n_draws=S, **_khat_fields(khat, S))
    if weights:
        log_sum = _lse0(lw)
        log_ess = _host(2.0 * log_sum - _lse0(2.0 * lw))
        with np.errstate(all="ignore"):
            out.update(log_weights=lw[:, 0] if flat else lw, log_sum=_host(log_sum), n_eff=np.exp(log_ess))
    return Summary(**out)


def loo_from_log_lik(log_lik):
    """PSIS-LOO of any model from its pointwise log-likelihood matrix (S, n), log p(y_i | theta_s), draws first; float32 or
    float64, numpy or a ROCm tensor.  The ratios are -log_lik; with w the smoothed log weights of `psis`,
    elpd_loo_i = lse(w + ll) - lse(w) and lppd_i = lse(ll) - log S.  The `Summary` has the fields of `predictive.loo`.

    This is the SLOW path: the caller forms the (S, n) matrix (in row groups -- column blocks -- when it is large; the per-row
    results of the groups concatenate to those of one call bit for bit), and every column's top M + 1 is found by a
    `torch.topk`.  The fused `predictive.loo` of the logistic regression never forms the matrix."""
    ll, flat = _as_ratios(log_lik, "log_lik")
    if flat:
        raise ValueError("log_lik must be (n_draws, n): one column per data row")
    S, n = int(ll.shape[0]), int(ll.shape[1])
    if S < 2:
        raise ValueError("PSIS-LOO needs >= 2 draws (got %d)" % S)
    khat, n_tail, _, lw, M = _psis(-ll, True)
    xp = ops_of(ll)
    import math
    with np.errstate(all="ignore"):
        l64 = xp.f64(ll)
        elpd = _lse0(lw + l64) - _lse0(lw)
        lppd = _lse0(l64) - math.log(S)
        khat = xp.where(xp.isnan(elpd), elpd, khat)
    return _loo_summary(_host(khat), _host(elpd), _host(lppd), _host(n_tail).astype(np.int64), S, M)
