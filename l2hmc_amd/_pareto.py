"""The array-operation layer and the generalised Pareto fit that `predictive` (the finish of PSIS-LOO) and `psis` (PSIS of any
log ratios) share: the same lines run over numpy on the host and over torch where the tails lie, and csrc/psis.hip restates
`_psis_rows` formula for formula."""
import numpy as np

from .diagnostics import Summary

KHAT_BAD = 0.7                # PSIS is unreliable above it whatever S is
MIN_TAIL_FIT = 5              # a shorter tail is not fitted: khat = +inf
_OPS = ("exp", "log", "log1p", "expm1", "sqrt", "floor", "where", "isfinite", "minimum", "maximum", "isnan")


class _Numpy:
    """The few array operations the fit and the finish need, over numpy ..."""
    def __init__(self):
        for k in _OPS:
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
        for k in _OPS:
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


def ops_of(a):
    """The operations of the library `a` belongs to."""
    return _Torch() if hasattr(a, "amax") else _Numpy()


def _softplus_neg(xp, v):
    """softplus(-v) = log(1 + e^-v)"""
    return xp.maximum(-v, v * 0.0) + xp.log1p(xp.exp(-xp.maximum(v, -v)))


def _centre(xp, mx, zero):
    """The centre of a logsumexp whose largest term is `mx`: 0 for an empty (-inf) row, NaN kept."""
    return xp.where(xp.isfinite(mx), mx, xp.where(xp.isnan(mx), mx, zero))


def _lse(xp, a, zero):
    """logsumexp over the last axis; -inf when empty"""
    mx = _centre(xp, xp.max(a), zero)
    return mx + xp.log(xp.sum(xp.exp(a - mx[..., None])))


def _logaddexp(xp, a, b, zero):
    """logaddexp of two (rows,) arrays"""
    mx = _centre(xp, xp.maximum(a, b), zero)
    return mx + xp.log(xp.exp(a - mx) + xp.exp(b - mx))


def loo_tail_len(S):
    """M = min(S // 5, ceil(3 sqrt S)): how many of the largest importance ratios PSIS may fit and smooth."""
    import math
    S = int(S)
    return min(S // 5, math.isqrt(9 * S - 1) + 1) if S >= 1 else 0


def theta_grid_len(M):
    """30 + floor(sqrt M): the length of the theta grid of a tail of M slots (Zhang & Stephens 2009 with the prior of `loo`)."""
    return 30 + int(np.floor(np.sqrt(max(M, 1))))


def lam_max(xp, lam, Lf, lam_c, M):
    """The largest log ratio of every row: slot 0 of its descending tail, or the cutoff's where the tail is empty."""
    return xp.where(Lf > 0, lam[:, 0], lam_c) if M else lam_c


def _psis_rows(xp, lam, Lf, lam_c, M):
    """The middle of `predictive._loo_rows`, and the host form of `psis.smooth_tails` (csrc/psis.hip restates it formula for
    formula): (khat, lam_max, lse_w, lse_wl, omega, live) of a chunk of rows whose (rows, M) log ratios `lam` descend over the
    L live slots; slot s < L holds the ratio of ascending rank j = L - s.  khat is the fitted shape or +inf where nothing was
    smoothed; omega (rows, M) is meaningful in the live slots only."""
    zero = Lf * 0.0
    slot = xp.arange(M, Lf)
    zeros = zero[:, None] + slot[None, :] * 0.0                                    # (rows, M)
    minus_inf = zeros - float("inf")
    live = slot[None, :] < Lf[:, None]
    j = Lf[:, None] - slot[None, :]                                                # ascending rank of the ratio, 1 .. L
    top = lam_max(xp, lam, Lf, lam_c, M)
    floor_c = xp.exp(lam_c - top)                                                  # the cutoff's ratio over the largest one
    x = xp.where(live, xp.exp(lam - top[:, None]) - floor_c[:, None], zeros)
    fit = Lf >= MIN_TAIL_FIT
    Ls = xp.where(fit, Lf, zero + MIN_TAIL_FIT)                                    # (a placeholder length where nothing is fitted)
    # Zhang & Stephens (2009) with the prior of `loo`: the profile likelihood on a grid of theta, theta's posterior mean
    jt = xp.arange(theta_grid_len(M), Lf) + 1.0
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
    omega = xp.where(smooth[:, None], xp.minimum(xp.log(qj + floor_c[:, None]), zeros), lam - top[:, None])
    lse_wl = _lse(xp, xp.where(live, omega - lam, minus_inf), zero)
    lse_w = _lse(xp, xp.where(live, omega, minus_inf), zero)
    khat = xp.where(smooth, k, zero + float("inf"))
    return khat, top, lse_w, lse_wl, omega, live


def _khat_fields(khat, S):
    """`khat_threshold` = min(1 - 1 / log10 S, 0.7) and the two counts of rows above a threshold."""
    with np.errstate(all="ignore"):
        threshold = min(1.0 - 1.0 / np.log10(S), KHAT_BAD) if S > 1 else KHAT_BAD
        return dict(khat_threshold=threshold, n_bad=int(np.sum(khat > KHAT_BAD)), n_above_threshold=int(np.sum(khat > threshold)))


def _se_rows(v):
    """sqrt(n var_i(v_i)), the standard error of a sum over n rows (sample variance; NaN for one row)"""
    n = v.shape[0]
    return float(np.sqrt(n * v.var(ddof=1))) if n > 1 else float("nan")


def _loo_summary(khat, elpd_i, lppd_i, n_tail, S, M):
    """The `Summary` of PSIS-LOO from its per-row numbers (the fields: `predictive.loo_finish`)."""
    with np.errstate(all="ignore"):
        p_loo_i = lppd_i - elpd_i
        elpd, p_loo, lppd = float(elpd_i.sum()), float(p_loo_i.sum()), float(lppd_i.sum())
        se = _se_rows(elpd_i)
    return Summary(elpd_loo_i=elpd_i, p_loo_i=p_loo_i, lppd_i=lppd_i, khat=khat, n_tail=n_tail, elpd_loo=elpd, p_loo=p_loo,
                   lppd=lppd, looic=-2.0 * elpd, se=se, **_khat_fields(khat, S), tail_len=M, n_draws=S, n_rows=elpd_i.shape[0],
                   n_underflow=int(np.sum(np.isneginf(lppd_i))))
