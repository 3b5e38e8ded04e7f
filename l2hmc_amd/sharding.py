"""Chain sharding across the GPUs of a node (one process per GPU, torch.distributed).

Chains never interact on the sampling path (every tensor is (N, ...) with no
cross-chain term), so the chain batch is cut into contiguous blocks -- rank r owns rows
[r*N/W, (r+1)*N/W) -- and the leapfrog kernels run with NO data-path collective.  The only
exchanges are small statistics: the mean accept probability, the autocovariance partial
sums behind ESS (utils/func_utils.py:45-54,114-120), the per-coordinate sums behind split R-hat /
ESS (`diagnostics`), the integer digit histograms behind posterior quantiles (`describe`), the four per-row sums behind the posterior predictive and WAIC (`predictive`), the raw moments behind the posterior covariance and the multivariate ESS (`multivariate`) and the two doubles per window of the step-size warm-up (`warmup`), each ONE flat all-reduce (`_allreduce_pieces` says it once for the float64 sums; `_on_device_collective` decides where it runs).  Backend
"nccl" is RCCL over xGMI on the GPU box; "gloo" is used by the CPU tests.
"""
import numpy as np
import torch
import torch.distributed as dist

from ._history import is_device_tensor


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_range(n_total, rank=None, world_size=None):
    """Contiguous block [lo, hi) of the n_total chains owned by `rank` (sizes differ by <= 1)."""
    if rank is None or world_size is None:
        rank, world_size = world()
    base, rem = divmod(int(n_total), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def _allreduce_sum(t):
    if world()[1] > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def mean_accept(p_local):
    """Global mean accept probability from this rank's (N_local,) probabilities."""
    p_local = torch.as_tensor(p_local)
    acc = torch.stack([p_local.double().sum(), torch.tensor(float(p_local.numel()), dtype=torch.float64,
                                                             device=p_local.device)])
    acc = _allreduce_sum(acc)
    return float(acc[0] / acc[1])


def autocov_partial_sums(X_local):
    """S(tau) = sum_t sum_{n,k} X[t,n,k] X[t+tau,n,k] for tau = 0..steps-2 on this rank's chains
    (X_local: (steps, N_local, d)); the per-lag normalisation is applied after the reduction."""
    X = torch.as_tensor(X_local, dtype=torch.float64)
    steps = X.shape[0]
    flat = X.reshape(steps, -1)
    out = torch.empty(steps - 1, dtype=torch.float64, device=X.device)
    for tau in range(steps - 1):
        out[tau] = (flat[:steps - tau] * flat[tau:]).sum()
    return out


def acl_spectrum(X_local, scale, n_total):
    """`acl_spectrum` of utils/func_utils.py:114-116 for chains sharded over ranks: one
    all-reduce of the (steps-1,) partial sums; equals the single-process value on the
    concatenated chains."""
    if is_device_tensor(X_local):                                  # HIP kernel, history stays in HBM
        from .func_utils import device_autocov
        steps = X_local.shape[0]
        s = _allreduce_sum(device_autocov(X_local, 1.0)[0] / (scale * scale))
    else:
        X = torch.as_tensor(X_local, dtype=torch.float64) / scale
        steps = X.shape[0]
        s = _allreduce_sum(autocov_partial_sums(X))
    lags = torch.arange(steps - 1, dtype=torch.float64, device=s.device)
    return (s / float(n_total) / (steps - lags)).cpu().numpy()


def ess(X_local, scale, n_total):
    """ESS per MH step (utils/func_utils.py:118-120) of sharded chains."""
    from .func_utils import ESS
    return float(ESS(acl_spectrum(X_local, scale, n_total)))


def diagnostics(X_local, max_lag=None, split=True):
    """`diagnostics.summarize` (split R-hat, per-coordinate ESS) for chains sharded over ranks: every rank forms the raw
    sums of its own chains (a ROCm tensor: the HIP kernels, the history stays in HBM), ONE all-reduce of
    [count | sum_c m | sum_c m^2 | sum_c M2 | G] per coordinate, then `diagnostics.finish`; equals the single-process value
    on the concatenated chains.  Ranks may hold different numbers of chains (each at least one; two without `split`), but
    the same number of steps, and must pass the same `max_lag`."""
    from . import diagnostics as dg
    return _finish_chain_sums(dg.chain_sums(X_local, max_lag=max_lag, split=split), X_local)


def _on_device_collective(X_local):
    return is_device_tensor(X_local) and world()[1] > 1 and dist.get_backend() != "gloo"


def _allreduce_where(t, X_local):
    """`_allreduce_sum` of `t` where the backend of the local history reduces: on its device (`_on_device_collective`), else
    on the host -- gloo does not reduce device tensors.  A tensor that had to move for it comes back on the host."""
    on_device = _on_device_collective(X_local)
    if t.is_cuda == on_device:
        return _allreduce_sum(t)
    return _allreduce_sum(t.to(X_local.device) if on_device else t.cpu()).cpu()


def _cut(flat, like):
    """The consecutive pieces of a flat vector in the shapes of `like`."""
    ends = np.cumsum([p.size for p in like])
    return [flat[e - p.size:e].reshape(p.shape) for e, p in zip(ends, like)]


def _allreduce_pieces(pieces, X_local):
    """ONE all-reduce of float64 numbers and arrays, concatenated in the order given; the reduced pieces in their shapes."""
    pieces = [np.asarray(p, dtype=np.float64) for p in pieces]
    flat = torch.from_numpy(np.concatenate([p.ravel() for p in pieces]))
    return _cut(_allreduce_where(flat, X_local).numpy(), pieces)


def _finish_chain_sums(sums, X_local):
    """`diagnostics.finish` of this rank's `chain_sums` after ONE all-reduce of their per-coordinate reductions."""
    from . import diagnostics as dg
    r = dg.reduce_sums(sums)
    keys = ("count", "sum_mean", "sum_mean_sq", "sum_m2", "G")
    return dg.finish(dict(zip(keys, _allreduce_pieces([r[k] for k in keys], X_local)), n_steps=r["n_steps"]))


def describe(X_local, probs=(0.05, 0.5, 0.95), max_lag=None, split=True):
    """`quantiles.describe` (quantiles, `ess_quantile`, `ess_tail`, `mcse_quantile` on top of `diagnostics`) for chains sharded
    over ranks.  The exchanges: one all-reduce of [S_local]; per `order_statistics` call (two: the quantiles, the MCSE
    positions) one all-reduce of the integer digit histograms per radix pass, between `l2hmc_order_stats_count` and
    `l2hmc_order_stats_advance` (the first carries n_nan); the single all-reduce of `diagnostics` per chain-sums call (one for
    the values, one per quantile's indicator series).  Integer histograms add exactly, so the quantiles are bit-identical to
    the single-process value on the concatenated chains; the `ess_*` agree to all-reduce rounding.  Ranks may hold different
    numbers of chains, but the same number of steps, and must pass the same `probs` and `max_lag`."""
    from . import quantiles as qt
    return qt._describe(X_local, probs, max_lag, split, allreduce=lambda t: _allreduce_where(t, X_local),
                        finish=lambda sums: _finish_chain_sums(sums, X_local))


def predictive(draws_local, X, y=None):
    """`predictive.finish(predictive.pointwise_sums(...))` (posterior predictive, lppd, WAIC) for chains sharded over ranks:
    every rank forms the four per-row sums of its own draws (a ROCm tensor: the HIP kernel, the history stays in HBM), ONE
    all-reduce of [n_draws | sum_p | sum_lik | sum_ll | sum_ll2], then `finish`; equals the single-process value on the
    concatenated draws.  Every rank passes the same rows X (and labels y); ranks may hold different numbers of draws."""
    from . import predictive as pd
    s = pd.pointwise_sums(draws_local, X, y)
    keys = ("n_draws", "sum_p", "sum_lik", "sum_ll", "sum_ll2")
    r = dict(zip(keys, _allreduce_pieces([s[k] for k in keys], draws_local)))
    r["n_draws"] = int(round(float(r["n_draws"])))
    return pd.finish(r)


def multivariate(X_local, batch_size=None):
    """`multivariate.multi_ess` (posterior covariance, correlation, multivariate ESS) for chains sharded over ranks: every
    rank forms the raw moments of its own chains (a ROCm tensor: the HIP kernels, the history stays in HBM), ONE all-reduce of
    [n | sum | cross | A | batch_sum | batch_cross] (each number as a head of 24 bits and a float64 rest), then
    `multivariate.finish`; equals the single-process value on the concatenated chains up to the rounding of the all-reduce.  Ranks may hold different numbers of chains, but the same
    number of steps, and must pass the same `batch_size`."""
    from . import multivariate as mv
    s = mv.moment_sums(X_local, mv._batch_size(X_local, batch_size))
    keys = ("n_draws", "sum", "cross", "n_batches", "batch_sum", "batch_cross")
    like = [mv._wide(s[k]) for k in keys]
    wide = np.concatenate([p.ravel() for p in like])
    # every number travels as two float64: a head of 24 significant bits, whose sums over ranks are exact, and the rest (for a
    # device sum, what float64 holds beyond the head; for a numpy sum, what long double holds) -- still ONE all-reduce.  The
    # head is cut by scaling, so it has the range of float64 and a finite moment stays finite
    with np.errstate(all="ignore"):
        frac, expo = np.frexp(wide)
        hi = np.ldexp(np.rint(frac * 2.0 ** 24) / 2.0 ** 24, expo).astype(np.float64)
        lo = np.where(np.isfinite(hi), wide - hi, 0.0).astype(np.float64)
    hi, lo = _allreduce_pieces([hi, lo], X_local)
    r = dict(zip(keys, _cut(hi.astype(np.longdouble) + lo.astype(np.longdouble), like)), batch_size=s["batch_size"])
    r["n_draws"], r["n_batches"] = int(round(float(r["n_draws"]))), int(round(float(r["n_batches"])))
    return mv.finish(r)


def warmup(x_local, dynamics, n_updates=100, *, n_total=None, **kwargs):
    """`warmup.warmup` (step size by dual averaging, on the device) for chains sharded over ranks: per window every rank
    reduces its own accept probabilities to {sum, count} (`l2hmc_adapt_update`, mode REDUCE), ONE all-reduce of the two
    doubles, then every rank applies the same update (mode APPLY) -- so every rank holds bit-identical state and alpha.
    `n_total`: chains over all ranks (default: this rank's count times the world size); the Philox `chain_offset` comes
    from `shard_range`, so a seeded run draws the same numbers however the chains are sharded."""
    from .warmup import warmup as _warmup
    if "chain_offset" in kwargs:
        raise TypeError("sharding.warmup derives chain_offset from shard_range")
    rank, size = world()
    n_local = int(x_local.shape[0])
    lo, hi = shard_range(n_local * size if n_total is None else n_total, rank, size)
    if hi - lo != n_local:
        raise ValueError("rank %d owns chains [%d, %d) of %s but was given %d" % (rank, lo, hi, n_total, n_local))
    return _warmup(x_local, dynamics, n_updates, chain_offset=lo, _allreduce=_allreduce_sum, **kwargs)
