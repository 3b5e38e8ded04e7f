"""Per-coordinate convergence diagnostics of a recorded history (steps, chains, dim): split R-hat and the effective sample size
in the form of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021) / Stan, without rank normalisation.

Unlike `func_utils.acl_spectrum` / `ESS` (the reference's diagnostic: no mean subtraction, one number summed over every
coordinate) the series are centred with their own means, every coordinate gets its own numbers, and the chains are compared
with each other -- what a posterior whose mean is not 0 needs.

    s = summarize(x_hist[burn_in:])          # x_hist of sample_chain / Dynamics.run, cold_hist of ParallelTempering.run
    s.max_rhat, s.min_ess, s.rhat, s.ess, s.mean, s.sd, s.truncated

A ROCm tensor goes to the HIP kernels behind `l2hmc_chain_stats` (csrc/chain_stats.hip) where it lies -- a first-axis slice of a
history is contiguous -- and only the per-coordinate sums (3 d + d (max_lag + 1) numbers) come back; a numpy history is computed in float64 numpy (`_history`
has the rule and the host side of the launch).

The estimator.  With `split` every chain becomes two, rows [0, Mh) and [M - Mh, M) with Mh = M // 2: C = 2 N series of length
Mh per coordinate (first halves, then second halves); without it Mh = M, C = N.  Per series: mean m and M2 = sum (x - m)^2.  Per
coordinate: W = mean_c M2 / (Mh - 1), B = Mh var_c(m), varp = (Mh - 1) / Mh W + B / Mh, rhat = sqrt(varp / W); lag sums
G[t] = sum_c sum_{i < Mh - t} (x_i - m_c)(x_{i+t} - m_c), rho_t = 1 - (W - G[t] / (C (Mh - 1))) / varp; pairs
P_j = rho_2j + rho_2j+1 up to the first P_j <= 0 (none within max_lag: `truncated`, ask for more lags), replaced by their running
minimum; tau = -1 + 2 sum P; ess = C Mh / tau.
"""
import numpy as np

from . import _ffi
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace

DEFAULT_MAX_LAG = 255
MAX_DEVICE_DIM = 512          # l2hmc_chain_stats: d <= 512


def _shape(M, N, split, max_lag):
    """(Mh, C, max_lag) of a (M, N, .) history, or ValueError."""
    Mh = M // 2 if split else M
    C = 2 * N if split else N
    if Mh < 4 or C < 2:
        raise ValueError("diagnostics need >= 4 steps per (split) chain and >= 2 chains (got %d, %d)" % (Mh, C))
    if max_lag is None:
        max_lag = min(Mh - 1, DEFAULT_MAX_LAG)
    max_lag = int(max_lag)
    if not 0 <= max_lag <= Mh - 1:
        raise ValueError("max_lag must be in 0 .. steps per chain - 1 = %d (got %d)" % (Mh - 1, max_lag))
    return Mh, C, max_lag


def _device_sums(X, Mh, C, max_lag, split, thresholds=None):
    """`thresholds` (d float64): the sums of the indicator series [x <= thresholds[k]] (`l2hmc_chain_stats_below`)."""
    import torch
    X = in_place(X)
    M, N, d = X.shape
    L, dev = _ffi.lib(), X.device
    ws = workspace(dev, torch.float64, L.l2hmc_chain_stats_workspace_doubles, M, N, d, max_lag, int(split))
    mean = torch.empty((C, d), dtype=torch.float64, device=dev)
    m2 = torch.empty((C, d), dtype=torch.float64, device=dev)
    G = torch.empty((d, max_lag + 1), dtype=torch.float64, device=dev)
    out = (mean.data_ptr(), m2.data_ptr(), G.data_ptr(), ws.data_ptr())
    if thresholds is None:
        launch(dev, L.l2hmc_chain_stats, X.data_ptr(), M, N, d, max_lag, int(split), *out)
    else:
        thr = torch.as_tensor(np.ascontiguousarray(thresholds, dtype=np.float64)).to(dev)
        launch(dev, L.l2hmc_chain_stats_below, X.data_ptr(), M, N, d, max_lag, int(split), thr.data_ptr(), *out)
    return mean, m2, G


def _host_sums(X, Mh, max_lag, split):
    X = np.asarray(X)
    if X.dtype != np.float64:
        X = X.astype(np.float64)
    M = X.shape[0]
    S = np.concatenate([X[:Mh], X[M - Mh:]], axis=1) if split else X             # (Mh, C, d)
    with np.errstate(all="ignore"):                         # a non-finite entry makes its own coordinate NaN, quietly
        mean = S.mean(axis=0)
        Z = S - mean
        m2 = np.einsum("tck,tck->ck", Z, Z)
        G = np.empty((X.shape[2], max_lag + 1))
        for t in range(max_lag + 1):
            G[:, t] = np.einsum("tck,tck->k", Z[:Mh - t], Z[t:])
    return mean, m2, G


def chain_sums_below(X, thresholds, max_lag=None, split=True):
    """`chain_sums` of the indicator series y = [x <= thresholds[k]] (compared in float64) of a (M, N, d) history, which is
    never written out: what the effective sample size of a quantile estimate is computed from (`quantiles.describe`).  A NaN
    value or threshold gives y = 0."""
    thresholds = np.asarray(thresholds, dtype=np.float64)
    if thresholds.shape != (int(X.shape[-1]),):
        raise ValueError("thresholds must be (dim,) = (%d,); got shape %s" % (int(X.shape[-1]), thresholds.shape))
    return chain_sums(X, max_lag=max_lag, split=split, _thresholds=thresholds)


def chain_sums(X, max_lag=None, split=True, _thresholds=None):
    """The raw sums of a (M, N, d) history: {'mean': (C, d), 'm2': (C, d), 'G': (d, max_lag + 1), 'n_steps': Mh, 'n_chains': C}.
    A ROCm tensor -> HIP kernels, float64 device tensors (bitwise reproducible); numpy -> float64 numpy."""
    M, N, d = history_shape(X)
    Mh, C, max_lag = _shape(M, N, split, max_lag)
    if d < 1:
        raise ValueError("a history needs dim >= 1")
    if is_device_tensor(X):
        if d > MAX_DEVICE_DIM:
            raise ValueError("the diagnostic kernels hold dim <= %d (got %d)" % (MAX_DEVICE_DIM, d))
        mean, m2, G = _device_sums(X, Mh, C, max_lag, split, _thresholds)
    else:
        X = as_numpy(X)
        if _thresholds is not None:
            with np.errstate(invalid="ignore"):
                X = (X.astype(np.float64) <= _thresholds).astype(np.float64)
        mean, m2, G = _host_sums(X, Mh, max_lag, split)
    return {"mean": mean, "m2": m2, "G": G, "n_steps": Mh, "n_chains": C}


def reduce_sums(sums):
    """The per-coordinate reductions `finish` works from -- and ranks that hold different chains add up:
    {'count': C, 'sum_mean': sum_c m, 'sum_mean_sq': sum_c m^2, 'sum_m2': sum_c M2, 'G', 'n_steps'} (float64 numpy).  Device
    sums are reduced over chains on the device: 3 d + d (max_lag + 1) numbers come to the host, not the (C, d) arrays."""
    mean, m2 = sums["mean"], sums["m2"]
    if hasattr(mean, "detach"):
        mean, m2 = mean.double(), m2.double()
        parts = (mean.sum(dim=0), (mean * mean).sum(dim=0), m2.sum(dim=0))
    else:
        mean, m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
        parts = (mean.sum(axis=0), (mean * mean).sum(axis=0), m2.sum(axis=0))
    return {"count": float(mean.shape[0]), "sum_mean": as_numpy(parts[0]), "sum_mean_sq": as_numpy(parts[1]),
            "sum_m2": as_numpy(parts[2]), "G": as_numpy(sums["G"], np.float64), "n_steps": int(sums["n_steps"])}


class Summary(dict):
    """The result of `summarize`: a dict whose entries also read as attributes (it pickles and copies like a dict)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def finish(sums):
    """Steps 3, 5, 6 of the estimator on the host in float64 (d (max_lag + 1) numbers: not a kernel), from `chain_sums`'
    result or from its `reduce_sums` form (the sharded path all-reduces that form).  A coordinate with W = 0 or a non-finite
    entry gets rhat = ess = NaN, the others are untouched."""
    r = sums if "sum_mean" in sums else reduce_sums(sums)
    C, Mh, G = float(r["count"]), int(r["n_steps"]), np.asarray(r["G"], dtype=np.float64)
    d, nlag = G.shape
    with np.errstate(all="ignore"):
        mean = r["sum_mean"] / C
        W = r["sum_m2"] / C / (Mh - 1)
        B = Mh * (r["sum_mean_sq"] - r["sum_mean"] ** 2 / C) / (C - 1)
        varp = (Mh - 1) / Mh * W + B / Mh
        ok = np.isfinite(W) & np.isfinite(varp) & np.isfinite(G).all(axis=1) & (W > 0)
        rhat = np.where(ok, np.sqrt(varp / W), np.nan)
        rho = 1.0 - (W[:, None] - G / (C * (Mh - 1))) / varp[:, None]
        n_pairs = nlag // 2                                   # a trailing unpaired lag is ignored
        P = rho[:, 0:2 * n_pairs:2] + rho[:, 1:2 * n_pairs:2]
        P = np.where(ok[:, None], P, 1.0)                     # placeholders: the coordinate is NaN below
        stop = P <= 0
        K = np.where(stop.any(axis=1), stop.argmax(axis=1), n_pairs) if n_pairs else np.zeros(d, dtype=np.int64)
        Pm = np.minimum.accumulate(P, axis=1) if n_pairs else P
        tau = -1.0 + 2.0 * np.where(np.arange(n_pairs)[None, :] < K[:, None], Pm, 0.0).sum(axis=1)
        ess = np.where(ok, C * Mh / tau, np.nan)
        sd = np.sqrt(varp)
    truncated = ok & (K == n_pairs)
    return Summary(mean=mean, sd=sd, rhat=rhat, ess=ess, truncated=truncated, n_steps=Mh, n_chains=int(round(C)),
                   max_lag=nlag - 1, min_ess=float(np.min(ess)) if d else float("nan"),
                   max_rhat=float(np.max(rhat)) if d else float("nan"))


def summarize(X, max_lag=None, split=True):
    """Per-coordinate `mean`, `sd`, `rhat`, `ess`, `truncated` of a (steps, chains, dim) history, with `n_steps`, `n_chains`,
    `max_lag`, `min_ess` and `max_rhat` (NaN when any coordinate is degenerate: a constant or non-finite series).  On the
    host a constant series whose value is not exactly representable may keep a tiny M2 from the rounding of its mean and then
    is not reported as degenerate; `predictive.relative_eff` sets M2 = 0 for such a series itself, as the device does."""
    return finish(chain_sums(X, max_lag=max_lag, split=split))
