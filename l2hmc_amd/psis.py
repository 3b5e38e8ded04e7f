"""Pareto-smoothed importance sampling (PSIS; Vehtari, Simpson, Gelman, Yao, Gabry 2024) of ANY log importance ratios, and
PSIS-LOO of any model from its pointwise log-likelihood matrix -- the model-comparison counterpart of "any energy drops in as a
torch callable":

    s = psis(log_ratios)                  # (S, n) or (S,): draws first; float32 / float64, numpy or a ROCm tensor
    s.khat, s.n_tail, s.log_weights, s.log_sum, s.n_eff, s.n_bad, s.khat_threshold, s.n_above_threshold, s.tail_len, s.n_draws
    s = loo_from_log_lik(log_lik)         # (S, n): log p(y_i | theta_s); the fields of `predictive.loo`
    s = loo_from_log_lik(log_lik3, r_eff="auto", select="fused")       # (steps, chains, n): + n_eff, mcse_elpd_loo, ...
    e = relative_eff_from_log_lik(log_lik3)                            # e.r_eff, e.ess, e.truncated, e.n_truncated, e.n_nan
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

The draws of a sampler are Markov chains, not independent.  `relative_eff_from_log_lik(log_lik)` of a history (steps, chains, n)
gives per column r_eff_i = ESS(lik_i) / S on the series exp(ll - column maximum) (`diagnostics`' effective sample size;
`l2hmc_chain_stats_exp` on the device), and `loo_from_log_lik(log_lik, r_eff=...)` / `psis(log_ratios, r_eff=...)` then cut
column i at M_i = `predictive.tail_len_rows(r_eff, S)[i]` and report `n_eff`, `mcse_elpd_loo_i` and `mcse_elpd_loo` -- the
fields of `predictive.loo(r_eff=...)`.

`select="fused"` (opt-in, float32 ROCm matrices): `l2hmc_loglik_tails` (csrc/loglik_tails.hip) finds every column's cutoff and
maximum with the radix select of csrc/order_stats.hip and gathers the tail, the positions of its draws and three float64 sums
over the other draws in one more read of the matrix, in column groups of at most 512; the Pareto kernels finish where the
tails lie and no (S, n) float64 array is formed.  With c the cutoff's log-likelihood, `body` = sum over the draws outside the
tail of e^(c - ll), `body_sq` the same of e^(2 (c - ll)), `lik` = sum over all draws of e^(ll - top), and w the smoothed weights
relative to the largest ratio e^lam_max: sum_body w = e^(-c - lam_max) body, sum_body w^2 = e^(-2 (c + lam_max)) body_sq,
sum_body w lik = (S - L) e^-lam_max, lppd_i = log lik + top - log S, and the body's part of the variance behind the Monte Carlo
standard error is the three-term form N_b - 2 E sum_body w + E^2 sum_body w^2 of `predictive.loo`, divided through by E^2 so
that no e^-c is formed alone: e^(-2 (c + lam_max)) [N_b q^2 - 2 q body + body_sq] with q = e^(c - elpd_loo_i).  On the device
`r_eff` is served by the fused route only; the numpy route builds the same raw numbers in float64 and finishes them alike.

Not here: moment matching, float64 keys, an in-place strided read of more than 512 columns, forming the log-likelihood inside
a kernel, ranks that hold different draws (`sharding`)."""
import numpy as np

from . import _ffi
from . import diagnostics
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace
from ._pareto import (_Numpy, _Torch, _centre, _khat_fields, _logaddexp, _loo_summary, _psis_rows, lam_max, loo_tail_len, ops_of,
                      theta_grid_len)
from .diagnostics import Summary

_HOST_CHUNK_BYTES = 1 << 26  # the (rows, theta grid, tail) block of the Pareto profile formed at a time on the host
MAX_DEVICE_COLS = 512         # l2hmc_loglik_tails, l2hmc_chain_stats_exp, l2hmc_order_stats: columns of one launch
_NEG_ZERO_KEY = -5e-324       # stands for -0.0 on the host so that a float64 sort puts it before +0.0, as the device order does
SELECTS = ("topk", "fused")


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


def _slot_sum(a):
    """The sum over the last axis of (rows, M) whose dead slots -- every slot at or past a row's live ones -- hold exact zeros,
    by a pairwise tree over the next power of two P >= M (slots h .. onto slots 0 .., h = P / 2, P / 4, ...), padded with
    zeros.  Adding a zero changes nothing, so a row's sum depends on its live values alone, not on M: a column finished with
    another stride -- in another group of columns -- gives the same bits."""
    rows, M = int(a.shape[0]), int(a.shape[1])
    if M == 0:
        return a.sum(-1)
    P = 1 << (M - 1).bit_length()
    if P > M:
        if hasattr(a, "new_zeros"):
            a = ops_of(a).t.cat([a, a.new_zeros((rows, P - M))], dim=1)
        else:
            a = np.concatenate([a, np.zeros((rows, P - M))], axis=1)
    while P > 1:
        P //= 2
        a = a[:, :P] + a[:, P:2 * P]
    return a[:, 0]


def _smooth_cols(lam, n_tail, lam_c, lens, weights):
    """`smooth_tails` whose bits do not depend on the stride M of `lam`.  The kernel's sums have an order that depends on L_i
    alone; the numpy fit adds over all M slots, so on the host the columns of every distinct tail length m are fitted on their
    own (rows, m) block: what a column gets depends on its own length and values, not on its neighbours'."""
    if lens is None or is_device_tensor(lam):
        return smooth_tails(lam, n_tail, lam_c, weights=weights)
    n, M = lam.shape
    out = [np.empty(n), np.empty(n), np.empty(n)] + ([np.full((n, M), -np.inf)] if weights else [])
    for m in np.unique(lens):
        sel = np.nonzero(lens == m)[0]
        res = smooth_tails(lam[sel][:, :m], n_tail[sel], lam_c[sel], weights=weights)
        for o, v in zip(out[:3], res[:3]):
            o[sel] = v
        if weights:
            out[3][sel, :m] = res[3]
    return tuple(out)


def _lse0(a):
    """logsumexp over axis 0 (the draws) of float64 (S, n): `_pareto._lse`'s centring, `_tree_sum`'s order."""
    xp = ops_of(a)
    with np.errstate(all="ignore"):
        mx = _centre(xp, xp.max(a.T), 0.0)
        return mx + xp.log(_tree_sum(xp.exp(a - mx[None, :])))


def _select(r, lens=None):
    """(lam (n, M) descending, n_tail (n,) int64, cutoff (n,), idx (M, n) positions of the M largest, M) of float (S, n) ratios.
    `lens` (n,) int64 (numpy ratios only): column i is cut at its own rank lens[i], and M is the largest."""
    S = int(r.shape[0])
    M = loo_tail_len(S)
    if lens is not None:
        M = int(lens.max())
        k = np.asarray(r, dtype=np.float64)
        k = np.where((k == 0.0) & np.signbit(k), _NEG_ZERO_KEY, k)                 # -0 below +0, the order of the device and `_host_raw`
        order = np.argsort(k, axis=0, kind="stable")[::-1][:M + 1]
        vals = np.take_along_axis(k, order, axis=0)
        cutoff, top, idx = vals[lens, np.arange(r.shape[1])], vals[:M], order[:M]
        with np.errstate(invalid="ignore"):
            n_tail = ((top > cutoff[None, :]) & (np.arange(M)[:, None] < lens[None, :])).sum(axis=0).astype(np.int64)
        unkey = lambda v: np.where(v == _NEG_ZERO_KEY, -0.0, v)  # noqa: E731
        return np.ascontiguousarray(unkey(top).T), n_tail, unkey(cutoff), idx, M
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


def _psis(r, want_weights, lens=None):
    """khat, n_tail, lam_max (all (n,)), the (S, n) float64 smoothed log weights (or None), M -- where `r` lies."""
    lam, n_tail, cutoff, idx, M = _select(r, lens)
    res = _smooth_cols(lam, n_tail, cutoff, lens, want_weights)
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


def _check_select(select, on_device, dtype_is_f32, r_eff):
    """The routes a call may take, refused before anything is computed."""
    if select not in SELECTS:
        raise ValueError('select is "topk" or "fused" (got %r)' % (select,))
    if select == "fused":
        if not on_device:
            raise ValueError('select="fused" runs l2hmc_loglik_tails on a ROCm device; these are host data (numpy or a CPU tensor), '
                             'which float64 numpy serves: leave select="topk"')
        if not dtype_is_f32:
            raise ValueError('select="fused" takes float32 matrices (the radix select has float32 keys); this one is not: '
                             'use select="topk"')
    elif on_device and r_eff is not None:
        raise ValueError('on the device r_eff (per-column tail lengths, n_eff and the Monte Carlo SE) is served by the fused '
                         'selection only: pass select="fused"')


def _is_f32(a):
    return str(a.dtype).endswith("float32")


def _lens_of(r_eff, n, S):
    """(r_eff (n,) float64 with NaN where an entry is no positive number, M_i (n,) int64) -- the rules of `predictive.loo`."""
    from .predictive import _check_r_eff, tail_len_rows
    r = _check_r_eff(r_eff, n)
    return r, tail_len_rows(r, S)


def _col_groups(a, n):
    """(first column, float32 contiguous (S, m) block) of every group of at most MAX_DEVICE_COLS consecutive columns of a device
    matrix: a matrix of at most that many contiguous columns is read in place, a wider one a group's copy at a time."""
    if n <= MAX_DEVICE_COLS:
        yield 0, in_place(a)
        return
    for k in range(0, n, MAX_DEVICE_COLS):
        yield k, in_place(a[..., k:k + MAX_DEVICE_COLS])


def _device_raw(block, lens, want_pos):
    """`l2hmc_loglik_tails` of one float32 contiguous (S, m <= 512) block: {'cutoff', 'top' (m,) float32, 'n_tail' (m,) int64,
    'tail' (m, stride) float32 with +inf pads, 'tail_pos' (or None), 'body', 'body_sq', 'lik' (m,) float64, 'flag'}.  `lens`
    (m,) int64 numpy or None (one length `loo_tail_len(S)`)."""
    import torch
    S, m = (int(v) for v in block.shape)
    dev, L = block.device, _ffi.lib()
    stride = loo_tail_len(S) if lens is None else int(lens.max())
    lens_d = None if lens is None else torch.as_tensor(np.ascontiguousarray(lens, dtype=np.int64)).to(dev)
    ws = workspace(dev, torch.uint8, L.l2hmc_loglik_tails_workspace_bytes, S, m)
    cutoff = torch.empty(m, dtype=torch.float32, device=dev)
    top = torch.empty(m, dtype=torch.float32, device=dev)
    n_tail = torch.empty(m, dtype=torch.int64, device=dev)
    tail = torch.empty((m, stride), dtype=torch.float32, device=dev)
    pos = torch.empty((m, stride), dtype=torch.int64, device=dev) if want_pos else None
    sums = torch.empty((3, m), dtype=torch.float64, device=dev)
    launch(dev, L.l2hmc_loglik_tails, block.data_ptr(), S, m, None if lens_d is None else lens_d.data_ptr(), stride,
           cutoff.data_ptr(), top.data_ptr(), n_tail.data_ptr(), tail.data_ptr() if stride else None,
           pos.data_ptr() if want_pos and stride else None, sums.data_ptr(), ws.data_ptr())
    return {"cutoff": cutoff, "top": top, "n_tail": n_tail, "tail": tail, "tail_pos": pos, "body": sums[0], "body_sq": sums[1],
            "lik": sums[2], "flag": ws[:8].view(torch.int64).clone()}


def _check_flags(flags):
    import torch
    if flags and bool(torch.cat(flags).any()):
        raise RuntimeError("l2hmc_loglik_tails: a tail outgrew its slots: the select and the gather disagree")


def _host_raw(ll, lens):
    """The raw dict of `_device_raw` in float64 numpy (the tail sorted): a full sort per column, then the three sums by
    `_tree_sum`.  -0 sorts before +0 and every NaN last, as on the device; a column whose cutoff is a NaN (fewer than M_i + 1
    numbers) has every number in its tail, as the kernel gathers it."""
    S, n = ll.shape
    M = int(lens.max()) if n else 0
    with np.errstate(all="ignore"):
        k = np.asarray(ll, dtype=np.float64)
        k = np.where((k == 0.0) & np.signbit(k), _NEG_ZERO_KEY, k)
        low = np.sort(k, axis=0)
        c, top = low[lens, np.arange(n)], low[S - 1]
        no_c = np.isnan(c)[None, :]
        keep = np.where(no_c, ~np.isnan(low[:M]), low[:M] < c[None, :]) & (np.arange(M)[:, None] < lens[None, :])
        in_tail = np.where(no_c, ~np.isnan(k), k < c[None, :])
        a = c[None, :] - k
        body = _tree_sum(np.where(in_tail, 0.0, np.exp(a)))
        body_sq = _tree_sum(np.where(in_tail, 0.0, np.exp(2.0 * a)))
        lik = _tree_sum(np.exp(k - top[None, :]))
    unkey = lambda v: np.where(v == _NEG_ZERO_KEY, -0.0, v)  # noqa: E731
    return {"cutoff": unkey(c), "top": unkey(top), "n_tail": keep.sum(axis=0).astype(np.int64),
            "tail": unkey(np.where(keep, low[:M], np.inf).T.copy()), "tail_pos": None, "body": body, "body_sq": body_sq, "lik": lik,
            "lens": lens}


def _finish_raw(raw, S, r_eff=None):
    """(khat, elpd_loo_i, lppd_i, n_tail) -- with `r_eff` (m,) also (n_eff, mcse_elpd_loo_i) before n_tail -- float64 / int64
    numpy of one raw dict, computed where its tails lie (the module docstring has the formulas)."""
    import math
    tail = raw["tail"]
    xp = ops_of(tail)
    M = int(tail.shape[1])
    mc = r_eff is not None
    with np.errstate(all="ignore"):
        c, top_ll, Lf = xp.f64(raw["cutoff"]), xp.f64(raw["top"]), xp.f64(raw["n_tail"])
        lam = -xp.sort(xp.f64(tail))                         # ll ascending, the +inf pads last = ratios descending, -inf pads
        res = _smooth_cols(lam, raw["n_tail"], -c, raw.get("lens"), mc)
        zero = Lf * 0.0
        lmax = lam_max(xp, lam, Lf, -c, M)
        body = xp.f64(raw["body"])
        den = _logaddexp(xp, xp.log(body) - c - lmax, res[1], zero)
        elpd = _logaddexp(xp, xp.log(S - Lf) - lmax, res[2], zero) - den
        khat = xp.where(xp.isnan(elpd), elpd, res[0])        # a NaN draw makes the column NaN, quietly
        out = [khat, elpd, xp.log(xp.f64(raw["lik"])) + top_ll - math.log(S)]
        if mc:
            r = r_eff if isinstance(xp, _Numpy) else xp.t.as_tensor(r_eff).to(tail.device)
            omega, body_sq = res[3], xp.f64(raw["body_sq"])
            slot = xp.arange(M, Lf)
            live = slot[None, :] < Lf[:, None]
            zeros = zero[:, None] + slot[None, :] * 0.0      # (omega and lam are not finite in the dead slots)
            w2 = xp.where(live, xp.exp(2.0 * omega), zeros)
            Z2, scale, q = xp.exp(2.0 * den), xp.exp(-2.0 * (c + lmax)), xp.exp(c - elpd)
            n_eff = r * Z2 / (scale * body_sq + _slot_sum(w2))         # (the bits do not depend on the group's stride)
            v_body = scale * xp.maximum((S - Lf) * q * q - 2.0 * q * body + body_sq, zero)
            v_tail = _slot_sum(xp.where(live, w2 * (xp.exp(-lam - elpd[:, None]) - 1.0) ** 2, zeros))
            out += [n_eff, xp.sqrt((v_body + v_tail) / Z2 / r)]
    return tuple(xp.host(v) for v in out) + (np.asarray(xp.host(raw["n_tail"]), dtype=np.int64),)


def _psis_fused(r, want_weights, lens):
    """`_psis` on `l2hmc_loglik_tails`: the kernel selects the smallest values, so it is handed -r, one float32 (S, n) copy
    (`loo_from_log_lik` needs none: its ratios are the negated input already); the smoothed tail weights return
    to their draws through `tail_pos`.  (khat, n_tail, the (S, n) float64 log weights or None, M)"""
    import torch
    S, n = int(r.shape[0]), int(r.shape[1])
    neg = -r
    parts, flags = [], []
    for k, block in _col_groups(neg, n):
        m = int(block.shape[1])
        raw = _device_raw(block, None if lens is None else lens[k:k + m], want_weights)
        flags.append(raw["flag"])
        M = int(raw["tail"].shape[1])
        if want_weights:
            # equal ratios share the quantiles of their ranks: the later draw takes the larger one, as the stable sorts of the
            # `topk` and numpy routes have it -- and whatever slots the gather's atomics handed out, the weights are the same
            by_pos = torch.argsort(raw["tail_pos"], dim=-1, descending=True)
            asc, order = torch.sort(raw["tail"].gather(1, by_pos).to(torch.float64), dim=-1, stable=True)
            order = by_pos.gather(1, order)
        else:
            asc = torch.sort(raw["tail"].to(torch.float64), dim=-1).values
        lam, lam_c, Lf = -asc, -raw["cutoff"].to(torch.float64), raw["n_tail"].to(torch.float64)
        res = smooth_tails(lam, raw["n_tail"], lam_c, weights=want_weights)
        khat = torch.where(torch.isnan(raw["top"]), raw["top"].to(torch.float64), res[0])
        part = [khat, raw["n_tail"], lam_max(_Torch(), lam, Lf, lam_c, M)]
        if want_weights:
            part += [raw["tail_pos"].gather(1, order), res[3]]
        parts.append(part)
    _check_flags(flags)
    khat, n_tail, top = (torch.cat([p[j] for p in parts]) for j in range(3))
    M = loo_tail_len(S) if lens is None else int(lens.max())
    if not want_weights:
        return khat, n_tail, None, M
    lw = r.to(torch.float64) - top[None, :]
    k = 0
    for p in parts:
        pos, omega = p[3], p[4]
        m, Mg = int(pos.shape[0]), int(pos.shape[1])
        live = torch.arange(Mg, device=r.device)[None, :] < p[1][:, None]
        cols = (k + torch.arange(m, device=r.device))[:, None].expand(m, Mg)
        lw[pos[live], cols[live]] = omega[live]
        k += m
    return khat, n_tail, lw, M


def psis(log_ratios, weights=True, r_eff=None, select="topk"):
    """PSIS of log importance ratios (S, n) -- or (S,) for one set of weights -- float32 or float64, numpy or a ROCm tensor.
    A `Summary`: `khat` (n,), `n_tail` (n,), `tail_len`, `n_draws`, `n_bad` = #{khat > 0.7}, `khat_threshold` =
    min(1 - 1 / log10 S, 0.7), `n_above_threshold`; `log_weights` (S, n) float64, the smoothed log weights shifted so that the
    largest RAW ratio of a column is 0 (not normalised: a smoothed tail weight never exceeds it), `log_sum` (n,) =
    logsumexp over the draws of `log_weights` (so `log_weights - log_sum` are the normalised ones) and `n_eff` (n,) =
    exp(2 lse(w) - lse(2 w)), the importance-sampling effective sample size.  A 1-d input gives `log_weights` (S,) and the
    other arrays of length 1.  Device input: `log_weights` stays a device tensor, everything else comes to the host.
    `weights=False` skips the matrix (and `log_sum`, `n_eff`): khat alone.

    `r_eff` (n,): the relative efficiency of every column's draws (`relative_eff_from_log_lik`); column i is then cut at
    `predictive.tail_len_rows(r_eff, S)[i]` (`tail_len_row`; `tail_len` is the largest), `n_eff` is r_eff (sum w)^2 / sum w^2, and
    `r_eff` comes back with NaN where an entry was no positive number.  `select="fused"` (float32 ROCm tensors; module docstring)
    selects and gathers on `l2hmc_loglik_tails`; on the device `r_eff` needs it.  It costs one negated float32 copy of the
    matrix (the kernel selects the smallest values) besides the float64 `log_weights`, which `weights=False` spares.  With
    `r_eff` -0 counts as below +0 on every route, as the device orders them; the default route keeps its plain comparison."""
    on_device = is_device_tensor(log_ratios)
    _check_select(select, on_device, _is_f32(log_ratios), r_eff)
    r, flat = _as_ratios(log_ratios, "log_ratios")
    S, n = int(r.shape[0]), int(r.shape[1])
    rr = lens = None
    if r_eff is not None:
        if S < 2:
            raise ValueError("r_eff needs >= 2 draws (got %d)" % S)
        rr, lens = _lens_of(r_eff, n, S)
    if select == "fused":
        if S < 2:
            raise ValueError('select="fused" needs >= 2 draws (got %d)' % S)
        khat, n_tail, lw, M = _psis_fused(r, weights, lens)
    else:
        khat, n_tail, _, lw, M = _psis(r, weights, lens)
    khat, n_tail = _host(khat), _host(n_tail).astype(np.int64)
    out = dict(khat=khat, n_tail=n_tail, tail_len=M, n_draws=S, **_khat_fields(khat, S))
    if weights:
        log_sum = _lse0(lw)
        log_ess = _host(2.0 * log_sum - _lse0(2.0 * lw))
        with np.errstate(all="ignore"):
            n_eff = np.exp(log_ess) if rr is None else rr * np.exp(log_ess)
            out.update(log_weights=lw[:, 0] if flat else lw, log_sum=_host(log_sum), n_eff=n_eff)
    if rr is not None:
        out.update(r_eff=rr, tail_len_row=lens)
    return Summary(**out)


def _reff_device(X, M, N, n, Mh, C, max_lag, split):
    """`diagnostics.finish` of every column group, on the sums of `l2hmc_chain_stats_exp` shifted by the column maxima that one
    `l2hmc_order_stats` call finds."""
    import torch
    dev, L = X.device, _ffi.lib()
    for _, block in _col_groups(X, n):
        m = int(block.shape[2])
        rank = torch.full((1, m), M * N - 1, dtype=torch.int64, device=dev)
        top = torch.empty((1, m), dtype=torch.float32, device=dev)
        n_nan = torch.empty(m, dtype=torch.int64, device=dev)
        ws = workspace(dev, torch.uint8, L.l2hmc_order_stats_workspace_bytes, m, 1)
        launch(dev, L.l2hmc_order_stats, block.data_ptr(), M * N, m, rank.data_ptr(), 1, top.data_ptr(), n_nan.data_ptr(),
               ws.data_ptr())
        shift = top[0].to(torch.float64).contiguous()
        ws = workspace(dev, torch.float64, L.l2hmc_chain_stats_workspace_doubles, M, N, m, max_lag, int(split))
        mean = torch.empty((C, m), dtype=torch.float64, device=dev)
        m2 = torch.empty((C, m), dtype=torch.float64, device=dev)
        G = torch.empty((m, max_lag + 1), dtype=torch.float64, device=dev)
        launch(dev, L.l2hmc_chain_stats_exp, block.data_ptr(), M, N, m, max_lag, int(split), shift.data_ptr(), mean.data_ptr(),
               m2.data_ptr(), G.data_ptr(), ws.data_ptr())
        yield diagnostics.finish(diagnostics.reduce_sums({"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C}))


def _reff_host(X, M, Mh, C, max_lag, split):
    ll = as_numpy(X, np.float64)
    with np.errstate(all="ignore"):
        lik = np.exp(ll - ll.max(axis=(0, 1)))
    mean, m2, G = diagnostics._host_sums(lik, Mh, max_lag, split)
    series = np.concatenate([lik[:Mh], lik[M - Mh:]], axis=1) if split else lik
    with np.errstate(invalid="ignore"):                      # a constant series has M2 = 0 exactly, as on the device
        m2 = np.where(series.max(axis=0) == series.min(axis=0), 0.0, m2)
    yield diagnostics.finish(diagnostics.reduce_sums({"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C}))


def relative_eff_from_log_lik(log_lik, max_lag=None, split=False):
    """The per-column relative efficiency of the likelihoods of a recorded history of pointwise log-likelihoods `log_lik`
    (steps, chains, n): r_eff_i = ess_i / S with S = steps x chains and ess_i the effective sample size of `diagnostics` on the
    series exp(ll[t, c, i] - max ll[:, :, i]) of every chain (the shift only keeps the likelihoods inside float32: the
    effective sample size does not move with it) -- `predictive.relative_eff` for any model.  A `Summary` of `r_eff`, `ess`
    (n,), `truncated` (n,) bool, `n_truncated`, `n_nan` (columns whose series is constant or not finite: r_eff = NaN),
    `n_draws`, `n_steps`, `n_chains`, `max_lag`; `max_lag=None` is min(steps per chain - 1, `diagnostics.DEFAULT_MAX_LAG`).
    A ROCm tensor (read as float32) -> one `l2hmc_order_stats` call for the maxima, then `l2hmc_chain_stats_exp`, in column groups of at most
    512: a history of at most 512 contiguous columns is read in place, a wider one a group's copy at a time.  numpy or a CPU
    tensor -> float64 numpy.  A matrix (draws, n) is refused: its chains are not known."""
    M, N, n = history_shape(log_lik, says="relative_eff_from_log_lik needs a history (steps, chains, n): the chains of a matrix "
                                          "of draws are not known")
    if n < 1:
        raise ValueError("log_lik needs n >= 1 columns")
    Mh, C, max_lag = diagnostics._shape(M, N, split, max_lag)
    if is_device_tensor(log_lik):
        parts = list(_reff_device(log_lik.detach(), M, N, n, Mh, C, max_lag, split))
    else:
        parts = list(_reff_host(log_lik, M, Mh, C, max_lag, split))
    ess = np.concatenate([p.ess for p in parts])
    truncated = np.concatenate([p.truncated for p in parts])
    S = M * N
    return Summary(r_eff=ess / S, ess=ess, truncated=truncated, n_truncated=int(truncated.sum()), n_nan=int(np.isnan(ess).sum()),
                   n_draws=S, n_steps=Mh, n_chains=C, max_lag=max_lag)


def _loo_of_parts(parts, S, r, lens):
    """The `Summary` of the `_finish_raw` results `parts` of consecutive column groups (`loo_from_log_lik`, `glm.Glm.loo`);
    `r` (n,) and `lens` (n,), or None for independent draws."""
    cols = [np.concatenate([p[j] for p in parts]) for j in range(len(parts[0]))]
    s = _loo_summary(cols[0], cols[1], cols[2], cols[-1], S, loo_tail_len(S) if lens is None else int(lens.max()))
    if r is None:
        return s
    from .predictive import _mc_fields
    return _mc_fields(s, r, cols[3], cols[4], lens)


def loo_from_log_lik(log_lik, r_eff=None, select="topk", max_lag=None, split=False):
    """PSIS-LOO of any model from its pointwise log-likelihood matrix (S, n), log p(y_i | theta_s), draws first -- or the history
    form (steps, chains, n), which is read as (steps x chains, n); float32 or float64, numpy or a ROCm tensor.  The ratios are
    -log_lik; with w the smoothed log weights of `psis`, elpd_loo_i = lse(w + ll) - lse(w) and lppd_i = lse(ll) - log S.  The
    `Summary` has the fields of `predictive.loo`.

    `r_eff`: None treats the draws as independent (one tail length).  "auto" (the history form only) takes
    `relative_eff_from_log_lik(log_lik, max_lag, split).r_eff`; an array (n,) is used as given.  Column i is then cut at
    `predictive.tail_len_rows(r_eff, S)[i]` and the Summary gains the fields of `predictive.loo(r_eff=...)`: `r_eff`, `n_eff`,
    `min_n_eff`, `mcse_elpd_loo_i`, `mcse_elpd_loo` (NaN when a khat exceeds 0.7), `n_reff_nan`, `tail_len_row`.

    `select="topk"` (the default) is the SLOW path on the device: every column's top M + 1 is found by a `torch.topk` and the
    smoothed weights go into a float64 copy of the matrix; it serves no `r_eff` there.  `select="fused"` (float32 ROCm tensors)
    runs `l2hmc_loglik_tails` per group of at most 512 columns and finishes on the Pareto kernels where the tails lie: the
    matrix is read in place when it has at most 512 contiguous columns and no (S, n) float64 array is formed.  numpy or a CPU
    tensor is float64 numpy by either tail rule.  The caller forms the matrix (in column blocks when it is large; the
    per-column results of the blocks concatenate to those of one call bit for bit, with `r_eff` too: a column's sums over
    its tail slots depend on its own length and values, not on the longest tail of its block -- `_slot_sum`, `_smooth_cols`);
    the fused `predictive.loo` of the logistic
    regression never forms it."""
    shape = tuple(int(v) for v in log_lik.shape)
    on_device = is_device_tensor(log_lik)
    if isinstance(r_eff, str) and r_eff != "auto":
        raise ValueError('r_eff is None, "auto" or an array (n,) (got %r)' % (r_eff,))
    _check_select(select, on_device, _is_f32(log_lik), r_eff)
    if isinstance(r_eff, str):
        if len(shape) != 3:
            raise ValueError('r_eff="auto" needs the history form (steps, chains, n): the chains of a matrix of draws are not '
                             'known; got shape %s' % (shape,))
        r_eff = relative_eff_from_log_lik(log_lik, max_lag=max_lag, split=split).r_eff
    if len(shape) == 3:
        if shape[0] < 2 or shape[1] < 1:
            raise ValueError("the history form of log_lik is (steps, chains, n) with steps >= 2 and chains >= 1 (one step is a "
                             "matrix: pass (n_draws, n)); got shape %s" % (shape,))
        log_lik = log_lik.reshape(shape[0] * shape[1], shape[2])
    ll, flat = _as_ratios(log_lik, "log_lik")
    if flat:
        raise ValueError("log_lik must be (n_draws, n): one column per data row")
    S, n = int(ll.shape[0]), int(ll.shape[1])
    if S < 2:
        raise ValueError("PSIS-LOO needs >= 2 draws (got %d)" % S)
    if r_eff is None and select == "topk":
        khat, n_tail, _, lw, M = _psis(-ll, True)
        xp = ops_of(ll)
        import math
        with np.errstate(all="ignore"):
            l64 = xp.f64(ll)
            elpd = _lse0(lw + l64) - _lse0(lw)
            lppd = _lse0(l64) - math.log(S)
            khat = xp.where(xp.isnan(elpd), elpd, khat)
        return _loo_summary(_host(khat), _host(elpd), _host(lppd), _host(n_tail).astype(np.int64), S, M)
    r = lens = None
    if r_eff is not None:
        r, lens = _lens_of(r_eff, n, S)
    parts, flags = [], []
    if on_device:
        for k, block in _col_groups(ll, n):                  # every group is finished before the next one's tails are formed
            m = int(block.shape[1])
            raw = _device_raw(block, None if lens is None else lens[k:k + m], False)
            flags.append(raw["flag"])
            parts.append(_finish_raw(raw, S, None if r is None else r[k:k + m]))
        _check_flags(flags)
    else:
        parts.append(_finish_raw(_host_raw(ll, lens), S, r))
    return _loo_of_parts(parts, S, r, lens)
