"""Posterior quantiles of a recorded history with what says whether they can be trusted: exact order statistics, quantiles,
the effective sample size of every quantile estimate, tail-ESS and the Monte Carlo standard errors, per coordinate.  The
names and definitions are those of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021) and Stan's `posterior` package:
`ess_quantile`, `ess_tail`, `mcse_mean`, `mcse_quantile`.

    s = describe(x_hist[burn_in:])               # everything `summarize` returns, and
    s.quantiles, s.probs                         # (Q, d): by default the 5 %, 50 % and 95 % points of every coordinate
    s.ess_quantile, s.ess_tail, s.mcse_quantile, s.mcse_mean, s.truncated_quantile, s.n_nan

A ROCm tensor is read where it lies: `order_statistics` is a radix select on the device (csrc/order_stats.hip behind
`l2hmc_order_stats`, a few reads of the history and R d numbers back; no sort, no second copy), `ess_quantile` is the
split-chain ESS of the indicator series [x <= Q_p], formed by `l2hmc_chain_stats_below` as the values are loaded.  A numpy
history is host arithmetic (`np.sort`); `_history` has that rule and the host side of every launch.

Definitions.  Quantiles follow numpy's default ("linear"): h = (S - 1) p, lo = floor(h), hi = min(lo + 1, S - 1), and with
a, b the order statistics at lo, hi the result is a when a == b (or h == lo), else a + (h - lo) (b - a), in float64.
`ess_quantile(p)` = `diagnostics.finish` of the sums of I_t = [x_t <= Q_p]; `ess_tail` = the smaller of `ess_quantile` at
0.05 and 0.95; `mcse_mean` = sd / sqrt(ess); `mcse_quantile(p)`: with ess = ess_quantile(p),
a = betaincinv(ess p + 1, ess (1 - p) + 1, [0.1586553, 0.8413447]), the 1-based positions i1 = max(floor(a1 S), 1) and
i2 = min(ceil(a2 S), S) of the sorted draws, mcse = (x_(i2) - x_(i1)) / 2.  A coordinate with a NaN has NaN quantiles, alone;
+-inf are ordinary values.  Rank-normalised R-hat and bulk-ESS need the rank of every draw and are not computed.
"""
import numpy as np

from . import _ffi, diagnostics as dg
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace

MAX_RANKS = 32                    # l2hmc_order_stats: n_ranks <= 32 per call; more go in chunks
TAIL_PROBS = (0.05, 0.95)
ONE_SIGMA = (0.1586553, 0.8413447)
HOST_BITS, HOST_PASSES = 8, 4     # the radix select restated in numpy (histories sharded over ranks that hold numpy arrays)


def _as_draws(X):
    """The history as (S, d) float32: a device tensor read in place (`_history.in_place`), anything else as a numpy array."""
    d = history_shape(X, flat_ok=True)[-1]
    if d < 1 or int(np.prod([int(v) for v in X.shape[:-1]])) < 1:
        raise ValueError("a history needs at least one draw and dim >= 1; got shape %s" % (tuple(X.shape),))
    if is_device_tensor(X):
        if d > dg.MAX_DEVICE_DIM:
            raise ValueError("the order-statistics kernels hold dim <= %d (got %d)" % (dg.MAX_DEVICE_DIM, d))
        return in_place(X).view(-1, d)
    return np.ascontiguousarray(as_numpy(X), dtype=np.float32).reshape(-1, d)


def _rank_table(ranks, S, d):
    """(R, d) int64 from (R,) or (R, d); ValueError unless every rank is an integer in 0 .. S - 1."""
    r = np.asarray(ranks)
    if r.dtype.kind not in "iu":
        if r.dtype.kind != "f" or not np.all(r == np.floor(r)):
            raise ValueError("ranks must be integers")
    r = r.astype(np.int64)
    if r.ndim == 1:
        r = np.repeat(r[:, None], d, axis=1)
    if r.ndim != 2 or r.shape[1] != d or r.shape[0] < 1:
        raise ValueError("ranks must be (R,) or (R, dim) with R >= 1; got shape %s" % (np.shape(ranks),))
    if r.min() < 0 or r.max() >= S:
        raise ValueError("ranks must be in 0 .. draws - 1 = %d (got %d .. %d)" % (S - 1, r.min(), r.max()))
    return np.ascontiguousarray(r)


def _check_probs(probs):
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if p.ndim != 1 or p.shape[0] < 1 or not np.all((p >= 0) & (p <= 1)):      # NaN fails the comparison too
        raise ValueError("probs must be a non-empty sequence of numbers in [0, 1]; got %r" % (probs,))
    return p


# ---- order statistics ------------------------------------------------------------------------------------------------------
def _device_select(X2, ranks):
    """One `l2hmc_order_stats` call per chunk of 32 ranks."""
    import torch
    L, dev = _ffi.lib(), X2.device
    S, d = (int(v) for v in X2.shape)
    out, n_nan = [], None
    for a in range(0, ranks.shape[0], MAX_RANKS):
        rk = torch.as_tensor(ranks[a:a + MAX_RANKS]).to(dev)
        R = int(rk.shape[0])
        ws = workspace(dev, torch.uint8, L.l2hmc_order_stats_workspace_bytes, d, R)
        values = torch.empty((R, d), dtype=torch.float32, device=dev)
        nn = torch.empty(d, dtype=torch.int64, device=dev)
        launch(dev, L.l2hmc_order_stats, X2.data_ptr(), S, d, rk.data_ptr(), R, values.data_ptr(), nn.data_ptr(), ws.data_ptr())
        out.append(values.cpu().numpy())
        n_nan = nn.cpu().numpy() if n_nan is None else n_nan
    return np.concatenate(out, axis=0), n_nan


def _host_keys(X2):
    """The monotone uint32 key of every float32: bits ^ 0xFFFFFFFF when negative, else bits | 0x80000000; NaN = 0xFFFFFFFF."""
    b = X2.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    k[np.isnan(X2)] = np.uint32(0xFFFFFFFF)
    return k


def _host_count(keys, prefix, p, R):
    """(R, d, bins) int64: the histogram of digit p of the keys whose higher digits equal the prefix of (r, k)."""
    d, shift, bins = keys.shape[1], 32 - HOST_BITS * (p + 1), 1 << HOST_BITS
    hist = np.zeros((R, d, bins), dtype=np.int64)
    for k in range(d):
        digit = ((keys[:, k] >> np.uint32(shift)) & np.uint32(bins - 1)).astype(np.int64)
        if p == 0:
            hist[:, k] = np.bincount(digit, minlength=bins)
            continue
        high = keys[:, k] >> np.uint32(shift + HOST_BITS)
        for r in range(R):
            hist[r, k] = np.bincount(digit[high == (prefix[r, k] >> np.uint32(shift + HOST_BITS))], minlength=bins)
    return hist


def _host_advance(hist, remaining, prefix, p):
    """The digit in which the remaining rank falls extends the prefix; the counts below it leave the rank (in place)."""
    cum = np.cumsum(hist, axis=2)
    rem = np.clip(remaining, 0, np.maximum(cum[:, :, -1] - 1, 0))             # a rank past the end: the maximum
    digit = (cum > rem[:, :, None]).argmax(axis=2)
    below = np.take_along_axis(cum - hist, digit[:, :, None], axis=2)[:, :, 0]
    prefix |= (digit.astype(np.uint32) << np.uint32(32 - HOST_BITS * (p + 1)))
    remaining[...] = rem - below


def _host_decode(prefix):
    bits = np.where(prefix & np.uint32(0x80000000), prefix & np.uint32(0x7FFFFFFF), ~prefix)
    return bits.astype(np.uint32).view(np.float32)


def _sharded_select(X2, ranks, allreduce):
    """The select pass by pass, the histograms all-reduced between count and advance: `passes` all-reduces per chunk of 32
    ranks, the first of them carrying n_nan.  Every rank ends with the same values, bit-identical to the single-process
    result on the concatenated draws (integer histograms add exactly)."""
    import torch
    S, d = (int(v) for v in X2.shape)
    device = is_device_tensor(X2)
    out, n_nan = [], None
    if device:
        L, dev = _ffi.lib(), X2.device
        passes, bins = L.l2hmc_order_stats_passes(), L.l2hmc_order_stats_bins()
    else:
        passes, bins, keys = HOST_PASSES, 1 << HOST_BITS, _host_keys(X2)
    for a in range(0, ranks.shape[0], MAX_RANKS):
        R = min(MAX_RANKS, ranks.shape[0] - a)
        if device:
            remaining = torch.as_tensor(ranks[a:a + R]).to(dev)
            prefix = torch.zeros((R, d), dtype=torch.int32, device=dev)                  # uint32 bits
            flat = torch.empty(R * d * bins + d, dtype=torch.int64, device=dev)          # hist | n_nan: one all-reduce
            values = torch.empty((R, d), dtype=torch.float32, device=dev)
        else:
            remaining, prefix = ranks[a:a + R].copy(), np.zeros((R, d), dtype=np.uint32)
        for p in range(passes):
            if device:
                launch(dev, L.l2hmc_order_stats_count, X2.data_ptr(), S, d, R, p, prefix.data_ptr(), flat.data_ptr(),
                       flat[R * d * bins:].data_ptr() if p == 0 else None)
                red = allreduce(flat if p == 0 else flat[:R * d * bins])
                if red.data_ptr() != flat.data_ptr():
                    flat[:red.numel()] = red.to(dev)
                if p == 0 and n_nan is None:
                    n_nan = flat[R * d * bins:].cpu().numpy().copy()
                launch(dev, L.l2hmc_order_stats_advance, flat.data_ptr(), remaining.data_ptr(), prefix.data_ptr(), d, R, p,
                       values.data_ptr() if p == passes - 1 else None)
            else:
                hist = _host_count(keys, prefix, p, R)
                parts = [hist.ravel(), np.isnan(X2).sum(axis=0).astype(np.int64)] if p == 0 else [hist.ravel()]
                red = allreduce(torch.from_numpy(np.concatenate(parts))).numpy()
                if p == 0 and n_nan is None:
                    n_nan = red[R * d * bins:].copy()
                _host_advance(red[:R * d * bins].reshape(R, d, bins), remaining, prefix, p)
        out.append(values.cpu().numpy() if device else _host_decode(prefix))
    return np.concatenate(out, axis=0), n_nan


def _select(X2, ranks, allreduce=None):
    if allreduce is not None:
        return _sharded_select(X2, ranks, allreduce)
    if is_device_tensor(X2):
        return _device_select(X2, ranks)
    srt = np.sort(X2, axis=0)                                                  # NaNs last
    return np.take_along_axis(srt, ranks, axis=0), np.isnan(X2).sum(axis=0).astype(np.int64)


def order_statistics(X, ranks):
    """(values (R, d) float32, n_nan (d) int64) of a history (steps, chains, d) or (S, d): values[r, k] is the element a full
    ascending sort of coordinate k puts at position ranks[r, k] (0-based; `ranks` is (R,) or a per-coordinate table (R, d)).
    Exact -- one of the history's own float32 values.  NaNs sort last."""
    X2 = _as_draws(X)
    return _select(X2, _rank_table(ranks, int(X2.shape[0]), int(X2.shape[1])))


# ---- quantiles -------------------------------------------------------------------------------------------------------------
def _quantile_ranks(S, probs):
    h = (S - 1) * probs
    lo = np.floor(h).astype(np.int64)
    return lo, np.minimum(lo + 1, S - 1), h - lo


def _interpolate(a, b, frac, n_nan):
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where((a == b) | (frac[:, None] == 0), a, a + frac[:, None] * (b - a))
    q[:, np.asarray(n_nan) > 0] = np.nan
    return q


def _quantiles(X2, probs, allreduce=None, S=None):
    S = int(X2.shape[0]) if S is None else S
    d, Q = int(X2.shape[1]), probs.shape[0]
    lo, hi, frac = _quantile_ranks(S, probs)
    vals, n_nan = _select(X2, _rank_table(np.concatenate([lo, hi]), S, d), allreduce)
    return _interpolate(vals[:Q], vals[Q:], frac, n_nan), n_nan


def quantiles(X, probs):
    """(Q, d) float64: the quantiles of every coordinate by numpy's default ("linear") definition, from two exact order
    statistics each.  A coordinate that holds a NaN is NaN, alone."""
    return _quantiles(_as_draws(X), _check_probs(probs))[0]


def _describe(X, probs, max_lag, split, allreduce=None, finish=dg.finish):
    """`describe`; with `allreduce` / `finish` of `sharding.describe` the same on chains sharded over ranks."""
    from scipy.special import betaincinv
    probs = _check_probs(probs)
    out = finish(dg.chain_sums(X, max_lag=max_lag, split=split))
    X2 = _as_draws(X)
    S, d, Q = int(X2.shape[0]), int(X2.shape[1]), probs.shape[0]
    if allreduce is not None:
        import torch
        S = int(allreduce(torch.tensor([S], dtype=torch.int64))[0])
    every = np.concatenate([probs, [t for t in TAIL_PROBS if t not in probs]])
    q, n_nan = _quantiles(X2, every, allreduce, S)
    ess = np.empty((every.shape[0], d))
    trunc = np.empty((every.shape[0], d), dtype=bool)
    for i in range(every.shape[0]):
        s = finish(dg.chain_sums_below(X, q[i], max_lag=out["max_lag"], split=split))
        ess[i], trunc[i] = s["ess"], s["truncated"]
    tail = [int(np.flatnonzero(every == t)[0]) for t in TAIL_PROBS]
    with np.errstate(all="ignore"):
        ess_tail = np.minimum(ess[tail[0]], ess[tail[1]])                      # NaN when either is
        mcse_mean = out["sd"] / np.sqrt(out["ess"])
        e, p = ess[:Q], probs[:, None]
        ok = np.isfinite(e) & (e > 0) & (np.asarray(n_nan) == 0)[None, :]
        es = np.where(ok, e, 1.0)                                              # placeholders: the entry is NaN below
        a1, a2 = (betaincinv(es * p + 1, es * (1 - p) + 1, c) for c in ONE_SIGMA)
        i1 = np.maximum(np.floor(a1 * S), 1)
        i2 = np.minimum(np.ceil(a2 * S), S)
    pos = np.clip(np.concatenate([i1, i2]).astype(np.int64) - 1, 0, S - 1)
    v = _select(X2, _rank_table(pos, S, d), allreduce)[0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        mcse_q = np.where(ok, (v[Q:] - v[:Q]) / 2, np.nan)
    out.update(probs=probs, quantiles=q[:Q], n_nan=np.asarray(n_nan), ess_quantile=ess[:Q], truncated_quantile=trunc[:Q],
               ess_tail=ess_tail, mcse_mean=mcse_mean, mcse_quantile=mcse_q)
    return out


def describe(X, probs=(0.05, 0.5, 0.95), max_lag=None, split=True):
    """The coefficient table of a (steps, chains, dim) history as a `diagnostics.Summary`: everything `summarize` returns,
    unchanged, and per coordinate `quantiles` (Q, d) at `probs`, `n_nan`, `ess_quantile` and `truncated_quantile` (Q, d),
    `ess_tail`, `mcse_mean`, `mcse_quantile` (Q, d) -- the module docstring has the definitions.  An estimate is NaN where its
    coordinate is degenerate (a constant or non-finite series), alone."""
    return _describe(X, probs, max_lag, split)
