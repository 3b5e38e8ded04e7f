"""Model criticism of a generalised linear model over every recorded draw -- the host side of csrc/glm.hip, behind
`distributions.PoissonRegression`, `BinomialRegression`, `NegativeBinomialRegression` and `ProbitRegression` (the likelihood is
a family object: `Poisson`, `Binomial`, `NegBinomial`, `Probit` below -- the ABI number, the row constants, the float64 host ll and the mean):

    m = PoissonRegression(X, y, offset=log_exposure)
    ll = m.log_lik(x_hist[burn_in:], rows=slice(0, 512))      # the (S, 512) matrix, when it is wanted (the slow route)
    mu = m.predict_mean(x_hist[burn_in:])                     # (n,) posterior predictive mean
    s = m.waic(x_hist[burn_in:])                              # the fields of `predictive.waic`
    s = m.loo(x_hist[burn_in:], r_eff="auto")                 # the fields of `psis.loo_from_log_lik`

For row i and draw s, with eta = x_i . w_s, h = eta + o_i and mu = exp(h): ll = y_i h - mu - lgamma(y_i + 1).  The per-row
constants travel as `row_constants(y, offset)` (3, n) float32: the offset, g_i = lgamma(y_i + 1) (float64, rounded once) and
the saturated log-likelihood sat_i = y log y - y - lgamma(y + 1) (0 at y = 0), the supremum of ll over eta: exp(ll - sat_i)
lies in (0, 1] for every draw, so the likelihood sums need no pass that looks for a shift.

A ROCm tensor of draws goes to the kernels where it lies (a first-axis slice of a history is read in place); the
(draws, rows) matrix is formed only by `log_lik` and, a group of at most 512 rows at a time, by `relative_eff`, which hands
each group to `l2hmc_chain_stats_exp` with shift = sat.  `loo` finishes through `psis._finish_raw` / `l2hmc_psis_smooth` where
the tails lie, the rows in groups whose tails stay under `max_tail_bytes`, as `predictive.loo` groups them.  numpy or a CPU
tensor is float64 numpy: the matrix in float64, then the numpy routes of `psis`.

The binomial and the negative binomial share one log-likelihood (csrc/glm_family.hpp; include/l2hmc.h): with a per-row offset
o_i, weight m_i and constant c_i, t = eta + o_i and ll = y_i t - m_i softplus(t) + c_i.  Their row constants are (4, n):
[o, m, sat, c] with sat = y log(y / m) + (m - y) log(1 - y / m) + c (0 log 0 = 0), each formed in float64 and rounded once.
A float32 ll loses absolute accuracy in proportion to m |t| (the products y t and m softplus(t) are rounded at their own
magnitude and then cancel), as the Poisson family's does with large counts.

The probit family (`Probit`) is the binomial with the probit link: ll = y log Phi(t) + (m - y) log Phi(-t) + c, mean m Phi(t),
the same (4, n) row constants (the supremum of ll is at Phi(t) = y / m: the binomial's sat).  The device forms log Phi from one
float32 erfcx (csrc/l2hmc_kernels.hpp, ProbitLink), accurate in both tails; the host route is `torch.special.log_ndtr` in
float64."""
import math

import numpy as np

from . import _ffi, diagnostics, predictive, psis
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace
from ._pareto import loo_tail_len
from .diagnostics import Summary

MAX_COUNT = 1 << 24           # counts are exact in the float32 label slot of `l2hmc_pack_logistic` up to here
REFF_GROUP_ROWS = 512         # l2hmc_chain_stats_exp: columns of one launch
_REFF_BYTES = 256 << 20       # the float32 (draws, rows) block `relative_eff` forms at a time
_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def lgamma1p(y):
    """lgamma(y + 1) of an array, float64."""
    return _lgamma(np.asarray(y, dtype=np.float64) + 1.0).astype(np.float64)


def row_constants(y, offset):
    """(3, n) float32: the offset, g = lgamma(y + 1) and sat = y log y - y - g (0 at y = 0), formed in float64."""
    y = np.asarray(y, dtype=np.float64)
    g = lgamma1p(y)
    with np.errstate(all="ignore"):
        sat = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0)) - y - g, 0.0)
    return np.ascontiguousarray(np.stack([np.asarray(offset, dtype=np.float64), g, sat]), dtype=np.float32)


def _rows(rows, n):
    """(a, m) of `rows`: None (all), a slice with step 1 or a pair (first, stop)."""
    if rows is None:
        return 0, n
    if isinstance(rows, slice):
        a, b, step = rows.indices(n)
        if step != 1:
            raise ValueError("rows is a range of consecutive rows (a slice with step 1)")
    else:
        a, b = (int(v) for v in rows)
    if not 0 <= a < b <= n:
        raise ValueError("rows must be a non-empty range inside 0 .. %d (got %d .. %d)" % (n, a, b))
    return a, b - a


def _xlogy(a, b):
    """a log b with 0 log 0 = 0, float64."""
    with np.errstate(all="ignore"):
        return np.where(a > 0, a * np.log(np.where(a > 0, b, 1.0)), 0.0)


class Poisson(object):
    """The Poisson family with the log link: ll = y h - exp(h) - lgamma(y + 1), h = eta + offset; mean exp(h)."""
    abi = _ffi.GLM_POISSON
    mean_scale = 1.0                                         # the device's sum of means times this is the sum of E[y]

    def row_constants(self, y, offset, weight=None):
        return row_constants(y, offset)

    def host_ll(self, eta, y, offset, weight=None):
        """(ll, mean) float64 of eta (S, m) = x_i . w_s."""
        h = eta + offset
        mu = np.exp(h)
        return y * h - mu - lgamma1p(y), mu


class Binomial(object):
    """y successes out of `weight` = m trials, the logit link: t = eta + offset, ll = y t - m softplus(t) + log C(m, y); mean
    m sigmoid(t)."""
    abi = _ffi.GLM_BINOMIAL
    mean_scale = 1.0

    def terms(self, y, offset, weight):
        """(o, m, c) float64 of the shared log-likelihood y t - m softplus(t) + c, t = eta + o."""
        y, m = np.asarray(y, dtype=np.float64), np.asarray(weight, dtype=np.float64)
        return np.asarray(offset, dtype=np.float64), m, lgamma1p(m) - lgamma1p(y) - lgamma1p(m - y)

    def saturated(self, y, offset, weight=None):
        """sat = y log(y / m) + (m - y) log(1 - y / m) + c (0 log 0 = 0), float64: the supremum of ll over eta."""
        y = np.asarray(y, dtype=np.float64)
        _, m, c = self.terms(y, offset, weight)
        return _xlogy(y, y / m) + _xlogy(m - y, (m - y) / m) + c

    def row_constants(self, y, offset, weight=None):
        """(4, n) float32: o, m, sat and c, each formed in float64 and rounded once."""
        o, m, c = self.terms(y, offset, weight)
        return np.ascontiguousarray(np.stack([o, m, self.saturated(y, offset, weight), c]), dtype=np.float32)

    def mean(self, t, m):
        return m / (1.0 + np.exp(-t))

    def host_ll(self, eta, y, offset, weight=None):
        o, m, c = self.terms(y, offset, weight)
        t = eta + o
        return y * t - m * np.logaddexp(0.0, t) + c, self.mean(t, m)


class NegBinomial(Binomial):
    """NB2 counts with mean mu = exp(eta + offset) and variance mu + mu^2 / phi, phi fixed: the binomial's log-likelihood with
    m = y + phi, o = offset - log phi and c = lgamma(y + phi) - lgamma(phi) - lgamma(y + 1) (`weight` is not used).  The device
    sums exp(t) = mu / phi: `mean_scale` = phi."""
    abi = _ffi.GLM_NEGBINOMIAL

    def __init__(self, dispersion):
        self.phi = self.mean_scale = float(dispersion)

    def terms(self, y, offset, weight=None):
        y = np.asarray(y, dtype=np.float64)
        c = _lgamma(y + self.phi).astype(np.float64) - math.lgamma(self.phi) - lgamma1p(y)
        return np.asarray(offset, dtype=np.float64) - math.log(self.phi), y + self.phi, c

    def mean(self, t, m):
        return self.phi * np.exp(t)


class Probit(Binomial):
    """y successes out of `weight` = m trials, the probit link: t = eta + offset, ll = y log Phi(t) + (m - y) log Phi(-t) +
    log C(m, y); mean m Phi(t).  The row constants are the binomial's."""
    abi = _ffi.GLM_PROBIT

    @staticmethod
    def log_ndtr(t):
        """log Phi(t) of a float64 array, by torch.special.log_ndtr (accurate in both tails)."""
        import torch
        return torch.special.log_ndtr(torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64))).numpy()

    def mean(self, t, m):
        import torch
        return m * torch.special.ndtr(torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64))).numpy()

    def host_ll(self, eta, y, offset, weight=None):
        o, m, c = self.terms(y, offset, weight)
        t = eta + o
        return y * self.log_ndtr(t) + (m - y) * self.log_ndtr(-t) + c, self.mean(t, m)


class Glm(object):
    """The data of one model (X (n, d), y (n,), offset (n,), float32; `weight` (n,) where the family has one: the binomial's
    trials) and its statistics over draws under the likelihood `family` (an object: `Poisson()`, `Binomial()`,
    `NegBinomial(phi)`, `Probit()`); `self.family` is its ABI number."""

    def __init__(self, X, y, offset, family=None, weight=None):
        self.X, self.y, self.offset, self.weight = X, y, offset, weight
        self.lik = Poisson() if family is None else family
        self.family = self.lik.abi
        self.consts = self.lik.row_constants(y, offset, weight)
        self.n, self.d = X.shape
        self._dev = {}                                       # device -> ((X, y, consts) there, {(a, m): packed rows})

    # ---- shapes --------------------------------------------------------------------------------------------------------------
    def _check(self, draws, X=None):
        return predictive._check(draws, self.X if X is None else X, None)

    # ---- the host route ------------------------------------------------------------------------------------------------------
    def _host_ll(self, draws, S, a=0, m=None):
        """(ll, mu) float64 (S, m) of rows [a, a + m)."""
        m = self.n - a if m is None else m
        W = as_numpy(draws, np.float64).reshape(S, self.d)
        X, y, o = (np.asarray(v[a:a + m], dtype=np.float64) for v in (self.X, self.y, self.offset))
        wt = None if self.weight is None else np.asarray(self.weight[a:a + m], dtype=np.float64)
        with np.errstate(all="ignore"):
            return self.lik.host_ll(W @ X.T, y, o, wt)

    # ---- the device route ----------------------------------------------------------------------------------------------------
    def _device_data(self, dev, X=None, y=None, consts=None):
        """`pack(a, m)` -> (packed, consts (3, m) contiguous) of rows [a, a + m) on `dev`."""
        import torch
        own = X is None
        if own and str(dev) in self._dev:                    # the model's own data: moved and packed once per device
            (Xd, yd, cd), cache = self._dev[str(dev)]
        else:
            Xd, yd, cd = (torch.as_tensor(v).to(device=dev, dtype=torch.float32).contiguous()
                          for v in ((self.X, self.y, self.consts) if own else (X, y, consts)))
            cache = {}
            if own:
                self._dev[str(dev)] = ((Xd, yd, cd), cache)
        d, L = int(Xd.shape[1]), _ffi.lib()

        def pack(a, m):
            if (a, m) not in cache:
                packed = workspace(dev, torch.float32, L.l2hmc_packed_logistic_floats, m, d)
                launch(dev, L.l2hmc_pack_logistic, Xd[a:a + m].data_ptr(), yd[a:a + m].data_ptr(), m, d, packed.data_ptr())
                if len(cache) >= 64:                         # (a caller that walks many row ranges does not grow it without end)
                    cache.clear()
                cache[(a, m)] = (packed, cd[:, a:a + m].contiguous())
            return cache[(a, m)]
        return pack

    def _device_ll(self, W, S, pack, a, m):
        """The float32 (S, m) matrix of rows [a, a + m): `l2hmc_glm_log_lik`."""
        import torch
        dev, L = W.device, _ffi.lib()
        packed, consts = pack(a, m)
        out = torch.empty((S, m), dtype=torch.float32, device=dev)
        launch(dev, L.l2hmc_glm_log_lik, W.data_ptr(), S, self.d, packed.data_ptr(), consts.data_ptr(), m, self.family,
               out.data_ptr())
        return out

    # ---- public ---------------------------------------------------------------------------------------------------------------
    def log_lik(self, draws, rows=None):
        """The pointwise log-likelihood matrix (S, m) of the rows `rows` (None: all; a slice or (first, stop)): a float32 ROCm
        tensor from `l2hmc_glm_log_lik` for a ROCm tensor of draws -- the very values the fused `loo` and `waic` work on -- or
        float64 numpy.  The slow route: the caller forms it in row groups when it is large."""
        S, d, n = self._check(draws)
        a, m = _rows(rows, n)
        if not is_device_tensor(draws):
            return self._host_ll(draws, S, a, m)[0]
        W = in_place(draws)
        return self._device_ll(W, S, self._device_data(W.device), a, m)

    def pointwise_sums(self, draws, X=None, offset=None, weight=None):
        """{'sum_mu', 'sum_lik', 'sum_ll', 'sum_ll2' (n,) float64 numpy, 'sat', 'n_draws'} over the draws, sum_lik = the sum of
        exp(ll - sat).  With `X` (and `offset`, default 0; `weight`, default 1, where the family has one) the rows are new ones
        without responses: only 'sum_mu' means anything (y = 0 is packed)."""
        w_ = None
        if X is None:
            X_, y_, c_ = self.X, self.y, self.consts
        else:
            X_ = np.ascontiguousarray(as_numpy(X, np.float64), dtype=np.float32)
            if X_.ndim != 2 or X_.shape[0] < 1 or X_.shape[1] != self.d or not np.all(np.isfinite(X_)):
                raise ValueError("X must be finite (n_rows, %d) with n_rows >= 1; got shape %s" % (self.d, X_.shape))
            o_ = np.zeros(X_.shape[0]) if offset is None else as_numpy(offset, np.float64)
            if o_.shape != (X_.shape[0],) or not np.all(np.isfinite(o_)):
                raise ValueError("offset must be finite (n_rows,) = (%d,)" % X_.shape[0])
            y_ = np.zeros(X_.shape[0], dtype=np.float32)
            if self.weight is not None:
                w_ = np.ones(X_.shape[0]) if weight is None else np.broadcast_to(as_numpy(weight, np.float64), (X_.shape[0],))
                if not np.all(np.isfinite(w_)) or not np.all((w_ >= 1.0) & (w_ == np.floor(w_)) & (w_ <= MAX_COUNT)):
                    raise ValueError("trials must be integers with 1 <= trials <= 2^24")
                w_ = np.ascontiguousarray(w_, dtype=np.float32)
            c_ = self.lik.row_constants(y_, o_, w_)
        S, d, n = self._check(draws, X_)
        sat = c_[2].astype(np.float64)
        if is_device_tensor(draws):
            import torch
            if n > predictive.MAX_DEVICE_ROWS:
                raise ValueError("the kernels hold n_rows <= %d (got %d)" % (predictive.MAX_DEVICE_ROWS, n))
            W = in_place(draws)
            dev, L = W.device, _ffi.lib()
            packed, consts = (self._device_data(dev) if X is None else self._device_data(dev, X_, y_, c_))(0, n)
            ws = workspace(dev, torch.float64, L.l2hmc_glm_predict_workspace_doubles, S, n, d)
            sums = torch.empty((4, n), dtype=torch.float64, device=dev)
            launch(dev, L.l2hmc_glm_predict, W.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), n, self.family,
                   sums.data_ptr(), ws.data_ptr())
            s = sums.cpu().numpy()
            sum_mu = s[0] if self.lik.mean_scale == 1.0 else s[0] * self.lik.mean_scale
            return {"sum_mu": sum_mu, "sum_lik": s[1], "sum_ll": s[2], "sum_ll2": s[3], "sat": sat, "n_draws": S}
        model = self if X is None else Glm(X_, y_, np.ascontiguousarray(o_, dtype=np.float32), self.lik, w_)
        out = {k: np.zeros(n) for k in ("sum_mu", "sum_lik", "sum_ll", "sum_ll2", "m2_ll")}
        step = max(1, predictive._HOST_CHUNK_ELEMS // S)
        with np.errstate(all="ignore"):
            for a in range(0, n, step):                      # (a block of rows at a time: every draw of a row in one block)
                ll, mu = model._host_ll(draws, S, a, min(step, n - a))
                b = slice(a, a + ll.shape[1])
                out["sum_mu"][b], out["sum_ll"][b], out["sum_ll2"][b] = mu.sum(axis=0), ll.sum(axis=0), (ll * ll).sum(axis=0)
                out["sum_lik"][b] = np.exp(ll - sat[b]).sum(axis=0)
                z = ll - ll.mean(axis=0)
                out["m2_ll"][b] = (z * z).sum(axis=0)
        out.update(sat=sat, n_draws=S)
        return out

    def predict_mean(self, draws, X=None, offset=None, weight=None):
        """The posterior predictive mean E[y | x] = mean over the draws of the family's mean (Poisson: exp(x . w + offset)) of
        every row of X (default: the model's own rows and offsets; new rows take `offset`, default 0, and `weight`, default
        1): (n,) float64."""
        s = self.pointwise_sums(draws, X, offset, weight)
        return s["sum_mu"] / s["n_draws"]

    def waic(self, draws):
        """WAIC of the model's own data under the draws: the `Summary` of `predictive.finish` (elpd_waic, p_waic, lppd, se,
        elpd_i, p_waic_i, lppd_i, n_high_variance, n_underflow, ...; its `p_mean` is the predictive mean)."""
        s = self.pointwise_sums(draws)
        with np.errstate(all="ignore"):
            sums = {"sum_p": s["sum_mu"], "sum_lik": s["sum_lik"], "sum_ll": s["sum_ll"], "sum_ll2": s["sum_ll2"],
                    "log_sum_lik": np.log(s["sum_lik"]) + s["sat"], "n_draws": s["n_draws"]}
        if "m2_ll" in s:
            sums["m2_ll"] = s["m2_ll"]
        return predictive.finish(sums)

    def _tail_groups(self, W, S, lens, max_tail_bytes):
        """The raw dict of `psis._device_raw` of one group of consecutive rows at a time: `l2hmc_glm_loo_tails`."""
        import torch
        dev, L, n, d = W.device, _ffi.lib(), self.n, self.d
        if n > predictive.MAX_DEVICE_ROWS:
            raise ValueError("the kernels hold n_rows <= %d (got %d)" % (predictive.MAX_DEVICE_ROWS, n))
        pack = self._device_data(dev)
        M = loo_tail_len(S) if lens is None else (int(lens.max()) if n else 0)
        rows = max(1, min(n, int(max_tail_bytes) // max(1, 4 * M), (1 << 31) // max(1, M)))
        for a in range(0, n, rows):
            m = min(rows, n - a)
            packed, consts = pack(a, m)
            group = None if lens is None else lens[a:a + m]
            stride = M if group is None else int(group.max())
            lens_d = None if group is None else torch.as_tensor(np.ascontiguousarray(group, dtype=np.int64)).to(dev)
            ws = workspace(dev, torch.uint8, L.l2hmc_glm_loo_workspace_bytes, S, m, d)
            cutoff = torch.empty(m, dtype=torch.float32, device=dev)
            top = torch.empty(m, dtype=torch.float32, device=dev)
            n_tail = torch.empty(m, dtype=torch.int64, device=dev)
            tail = torch.empty((m, stride), dtype=torch.float32, device=dev)
            sums = torch.empty((3, m), dtype=torch.float64, device=dev)
            launch(dev, L.l2hmc_glm_loo_tails, W.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, self.family,
                   None if lens_d is None else lens_d.data_ptr(), stride, cutoff.data_ptr(), top.data_ptr(), n_tail.data_ptr(),
                   tail.data_ptr() if stride else None, sums.data_ptr(), ws.data_ptr())
            yield a, m, {"cutoff": cutoff, "top": top, "n_tail": n_tail, "tail": tail, "tail_pos": None, "body": sums[0],
                         "body_sq": sums[1], "lik": sums[2], "flag": ws[:8].view(torch.int64).clone()}

    def loo_tails(self, draws, tail_len_row=None, max_tail_bytes=256 << 20):
        """The raw material of PSIS-LOO of every row, as `l2hmc_loglik_tails` would give it for the matrix `log_lik` writes --
        without the matrix: {'cutoff', 'top', 'n_tail', 'tail' (n, stride), 'body', 'body_sq', 'lik', 'flag'} device tensors
        (ROCm draws only)."""
        import torch
        S, d, n = self._check(draws)
        if not is_device_tensor(draws):
            raise ValueError("loo_tails runs l2hmc_glm_loo_tails on a ROCm device; host draws take `loo`'s numpy route")
        lens = None if tail_len_row is None else predictive._check_lengths(tail_len_row, n, S)
        groups = [g for _, _, g in self._tail_groups(in_place(draws), S, lens, max_tail_bytes)]
        stride = max(int(g["tail"].shape[1]) for g in groups)
        for g in groups:                                     # (one stride for the concatenation: +inf pads)
            pad = stride - int(g["tail"].shape[1])
            if pad:
                g["tail"] = torch.cat([g["tail"], g["tail"].new_full((g["tail"].shape[0], pad), float("inf"))], dim=1)
        out = {k: torch.cat([g[k] for g in groups]) for k in ("cutoff", "top", "n_tail", "tail", "body", "body_sq", "lik", "flag")}
        out["flag"] = out["flag"].any().reshape(1).to(torch.int64)
        return out

    def loo(self, draws, r_eff=None, max_lag=None, split=False, max_tail_bytes=256 << 20):
        """PSIS-LOO of the model's own data under the draws: the `Summary` of `psis.loo_from_log_lik` (elpd_loo, p_loo, looic,
        se, khat, n_bad, ...; with `r_eff` also n_eff, mcse_elpd_loo, ...).  `r_eff`: None, "auto" (a history (steps, chains,
        dim) only: `relative_eff(draws, max_lag, split).r_eff`) or an array (n,)."""
        S, d, n = self._check(draws)
        if isinstance(r_eff, str):
            if r_eff != "auto":
                raise ValueError('r_eff is None, "auto" or an array (n_rows,) (got %r)' % (r_eff,))
            r_eff = self.relative_eff(draws, max_lag=max_lag, split=split).r_eff
        if not is_device_tensor(draws):
            return psis.loo_from_log_lik(self._host_ll(draws, S)[0], r_eff=r_eff)
        r = lens = None
        if r_eff is not None:
            r, lens = psis._lens_of(r_eff, n, S)
        parts, flags = [], []
        for a, m, raw in self._tail_groups(in_place(draws), S, lens, max_tail_bytes):     # each group is finished before the next
            flags.append(raw["flag"])
            parts.append(psis._finish_raw(raw, S, None if r is None else r[a:a + m]))
        import torch
        if bool(torch.cat(flags).any()):
            raise RuntimeError("l2hmc_glm_loo_tails: a tail outgrew its slots: the passes disagree")
        return psis._loo_of_parts(parts, S, r, lens)

    def relative_eff(self, draws, max_lag=None, split=False, max_bytes=_REFF_BYTES):
        """The per-row relative efficiency r_eff_i = ESS(p(y_i | w)) / S of a recorded history (steps, chains, dim): the
        `Summary` of `psis.relative_eff_from_log_lik`.  On the device the history form of the log-likelihood is materialised a
        group of rows at a time -- at most 512 rows and at most `max_bytes` -- by `l2hmc_glm_log_lik` and handed to
        `l2hmc_chain_stats_exp` with shift = sat; host draws form the float64 matrix."""
        M, N, _ = history_shape(draws, says="relative_eff needs a history (steps, chains, dim): the chains of a matrix of draws "
                                            "are not known")
        S, d, n = self._check(draws)
        Mh, C, max_lag = diagnostics._shape(M, N, split, max_lag)
        if not is_device_tensor(draws):
            return psis.relative_eff_from_log_lik(self._host_ll(draws, S)[0].reshape(M, N, n), max_lag=max_lag, split=split)
        import torch
        W = in_place(draws)
        dev, L = W.device, _ffi.lib()
        pack = self._device_data(dev)
        sat = torch.as_tensor(self.consts[2].astype(np.float64)).to(dev)
        rows = max(1, min(n, REFF_GROUP_ROWS, int(max_bytes) // (4 * S)))
        parts = []
        for a in range(0, n, rows):
            m = min(rows, n - a)
            ll = self._device_ll(W, S, pack, a, m)
            ws = workspace(dev, torch.float64, L.l2hmc_chain_stats_workspace_doubles, M, N, m, max_lag, int(split))
            mean = torch.empty((C, m), dtype=torch.float64, device=dev)
            m2 = torch.empty((C, m), dtype=torch.float64, device=dev)
            G = torch.empty((m, max_lag + 1), dtype=torch.float64, device=dev)
            launch(dev, L.l2hmc_chain_stats_exp, ll.data_ptr(), M, N, m, max_lag, int(split), sat[a:a + m].contiguous().data_ptr(),
                   mean.data_ptr(), m2.data_ptr(), G.data_ptr(), ws.data_ptr())
            parts.append(diagnostics.finish(diagnostics.reduce_sums({"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C})))
        ess = np.concatenate([p.ess for p in parts])
        truncated = np.concatenate([p.truncated for p in parts])
        return Summary(r_eff=ess / S, ess=ess, truncated=truncated, n_truncated=int(truncated.sum()),
                       n_nan=int(np.isnan(ess).sum()), n_draws=S, n_steps=Mh, n_chains=C, max_lag=max_lag)
