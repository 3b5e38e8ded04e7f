"""Shared by tests/test_loglik_cpu.py, tests/test_gpu_loglik.py and tools/loglik_accuracy.py: PSIS-LOO of a pointwise
log-likelihood matrix with per-column tail lengths, relative efficiencies and Monte Carlo standard errors
(`psis.loo_from_log_lik(r_eff=, select=)`, `psis.psis(r_eff=, select=)`, `psis.relative_eff_from_log_lik`) and the kernels
under them (`l2hmc_loglik_tails`, `l2hmc_chain_stats_exp`).

The restatement.  `restate_column(ll, M, r_eff)` is written from the definitions, one column at a time, independent of
l2hmc_amd/psis.py and l2hmc_amd/_pareto.py (the model is `psis_case.restate_column`; the Pareto fit is `loo_case._gpdfit`): a
full sort, the cut at rank M, the smoothed weights written back into all S log weights, and n_eff = r_eff / sum w^2 and
mcse = sqrt(sum w^2 (lik - E)^2 / r_eff) / E from the normalised weight vector -- no body / tail split anywhere.

The exact selection.  `select_exact(ll32, lens)` is what `l2hmc_loglik_tails` must return for a float32 matrix, in the total
order of the monotone uint32 key (-0 before +0, every NaN last): cutoff, top, n_tail, the tail as a sorted set of (key, draw)
pairs, and the three sums in extended precision with their bounds.

The bound of the sums.  A term is exp(a) with a = c - ll (body), 2 (c - ll) (body_sq) or ll - top (lik), a <= 0.  The kernel
forms d = fl(c - ll) in float64 from the exact float32 values: |d - (c - ll)| <= |c - ll| 2^-53, and doubling is exact, so the
argument is off by at most |c - ll| 2^-52 (body_sq; half that for body, |ll - top| 2^-53 for lik) and the exponential by that
much relatively; the double-precision exp adds at most one ulp, 2^-52.  Per term, relatively: at most (|c - ll| + 2) 2^-52
(|ll - top| in the place of |c - ll| for lik), the figure the issue sets.  The additions: S - 1 float64 additions of positive
numbers in whatever fixed order, each within 2^-53 of a partial sum that never exceeds the total: S 2^-53 relative to the sum.
The reference is `numpy.longdouble`, whose own error (its epsilon times (|a| + 2) per term) is added -- 2^-63 where long double
is the x87 format.  `sum_bounds` returns the reference and the bound.

The gates of the finished numbers follow the rule of `psis_case.gate`: tools/loglik_accuracy.py measures, on the CPU, the
disagreement of the module's numpy route and the restatement on every tested matrix; `MEASURED` holds the figures by the number
of draws, and `gate(S)` = 100 x the worst figure at any S' <= S, under the absolute cap 1e-9 for khat and elpd_loo_i; n_eff and
mcse are relative.  Nothing is taken from the kernel under test.  profiles/loglik_accuracy.txt records the run.

The gather's plan (csrc/loglik_tails.hip).  The draws are cut into segments of rows = max(64, ceil(S / 2048)) draws, one
thread per (segment, column) walks its draws four at a time, and a workgroup is 256 threads.  `GPU_SHAPES` names, besides the
shapes the issue sets (S in 25, 70, 4099, 65609; n in 1, 3, 65 -- past one 64-coordinate group of the count -- and 513 at
S = 70 -- two column groups):
    S = 63, 64, 65          one segment short of full, exactly full, one draw into a second segment
    S = 66, 67              a remainder of 2 and 3 after the four-draw steps of the last segment (25 and 70 have 1 and 2)
    (64, 4), (65, 4)        1 x 4 = 4 threads; and (4099, 3) / (4099, 4): 65 x 3 = 195 threads in one workgroup, 65 x 4 = 260 in two
    S = 131072, 131073      2048 segments of 64 draws, and the first S with 65 draws per segment (2017 segments)
    (70, 512)               the widest matrix one launch takes (the select's count walks eight 64-coordinate groups)
"""
import math

import numpy as np

from tests import lik_stats_case as lsc
from tests import loo_case as lc
from tests import psis_case as pc

CAP = 1e-9
MARGIN = 100.0

# (S, n): the raw-output and bit tests run every one of GPU_SHAPES; the finished-number tests (CPU: numpy route against the
# restatement; GPU: fused against numpy) and tools/loglik_accuracy.py run FINISH_SHAPES -- every n the issue names (1, 3, 65,
# 513) at the smallest and at a several-workgroup S, and one large S; the other GPU_SHAPES sit on boundaries of the gather's
# plan, which the raw tests hold bit for bit and the finish does not see
GPU_SHAPES = [(25, 1), (25, 3), (63, 3), (64, 4), (65, 4), (66, 3), (67, 1), (70, 3), (70, 65), (4099, 1), (4099, 3), (4099, 4),
              (4099, 65), (65609, 1), (65609, 3), (131072, 1), (131073, 2), (70, 512)]
WIDE = (70, 513)              # two column groups of the Python route; its halves are [0, 256) and [256, 513)
FINISH_SHAPES = [(25, 1), (25, 3), (70, 3), (70, 65), (4099, 1), (4099, 3), (4099, 65), (65609, 3), WIDE]
# where a group of columns is finished against the same columns inside the whole call: per-column tail lengths 184 .. 496 from
# `r_eff_for`, so the two groups' strides differ (at WIDE every length is S // 5 = 14 and they do not)
GROUP_CASE = (4099, 65, 32)   # S, n, first column of the group [32, 65)
# AR(1) log-likelihood histories: the fixtures of lik_stats_case whose r_eff range is recorded there
AR1_FIXTURES = [f for f in lsc.FIXTURES if f in lsc.R_EFF_RANGE]

# n_draws -> the worst disagreement of the numpy route and the restatement: (khat abs, elpd_loo_i abs, n_eff rel, mcse rel),
# over the matrices of FINISH_SHAPES and the AR(1) histories with that many draws, with and without r_eff
# (tools/loglik_accuracy.py on the CPU; profiles/loglik_accuracy.txt)
MEASURED = {
    25: (4.44e-16, 8.88e-16, 7.77e-16, 1.33e-14),
    70: (2.89e-15, 3.11e-15, 4.44e-15, 7.99e-15),
    1152: (8.1e-15, 1.29e-14, 2.15e-14, 1.05e-14),
    3360: (1.68e-14, 3.02e-14, 3.69e-14, 1.97e-14),
    4000: (3.47e-14, 3.38e-14, 5.68e-14, 4.22e-14),
    4099: (1.72e-14, 3.73e-14, 6.22e-14, 3.04e-14),
    65609: (7.05e-14, 1.46e-13, 1.4e-13, 8.4e-14),
}


def gate(S):
    """(khat, elpd_loo_i, n_eff rel, mcse rel) gates at S draws: 100 x the worst disagreement measured at any S' <= S; khat and
    elpd at most 1e-9."""
    rows = [v for s, v in MEASURED.items() if s <= S]
    k, e, n, m = (max(v[j] for v in rows) for j in range(4))
    return min(MARGIN * k, CAP), min(MARGIN * e, CAP), MARGIN * n, MARGIN * m


def matrix(S, n, ties=True):
    """`psis_case.log_lik_case` with the tie block in column 0, seeded by the shape."""
    return pc.log_lik_case(S, n, 7000 + S + n, ties=ties)


def r_eff_for(n):
    """relative efficiencies 0.15 .. 1.1 over the columns (n = 1: 0.4)"""
    return np.array([0.4]) if n == 1 else 0.15 + 0.95 * np.arange(n) / (n - 1)


def lengths_for(S, n):
    """per-column tail lengths that include 0, 1, 4, 5 and S // 5 in one call"""
    return np.array([(0, 1, 4, 5, S // 5)[i % 5] for i in range(n)], dtype=np.int64).clip(0, S // 5)


def ar1_log_lik(fixture):
    """(ll (M, N, n) float64, float32 copy, W, X, y) of a lik_stats_case fixture: the logistic log-likelihood history."""
    M, N, d, rho, _, _ = fixture
    W, X, y = lsc.ar1_case(M, N, d, rho)
    ll = -np.logaddexp(0.0, -lsc.signed_logits(W, X, y))
    return ll, ll.astype(np.float32), W, X, y


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def restate_column(ll, M, r_eff=None):
    """{'khat', 'n_tail', 'elpd_loo_i', 'lppd_i', 'log_weights' (S,)[, 'n_eff', 'mcse']} of one column of log-likelihoods cut
    at rank M."""
    ll = np.asarray(ll, dtype=np.float64)
    S = len(ll)
    lw = -ll
    cutoff = np.sort(lw)[S - M - 1]
    idx = np.nonzero(lw > cutoff)[0]
    L = len(idx)
    mx = lw.max()
    lw = lw - mx
    khat = np.inf
    if L >= 5:
        order = idx[np.argsort(lw[idx], kind="stable")]
        ec = np.exp(cutoff - mx)
        with np.errstate(all="ignore"):
            k, sigma = lc._gpdfit(np.exp(lw[order]) - ec)
            if np.isfinite(k) and np.isfinite(sigma):
                p = (np.arange(1, L + 1) - 0.5) / L
                q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
                lw[order] = np.minimum(np.log(q + ec), 0.0)
                khat = k
    out = {"khat": khat, "n_tail": L, "log_weights": lw,
           "elpd_loo_i": np.logaddexp.reduce(lw + ll) - np.logaddexp.reduce(lw),
           "lppd_i": np.logaddexp.reduce(ll) - math.log(S)}
    if r_eff is not None:
        with np.errstate(all="ignore"):
            w = np.exp(lw - np.logaddexp.reduce(lw))
            top = ll.max()
            lik = np.exp(ll - top)                            # the likelihoods over the largest one: E and lik scale alike
            E = float(np.sum(w * lik))
            out["n_eff"] = r_eff / float(np.sum(w * w))
            out["mcse"] = math.sqrt(float(np.sum(w * w * (lik - E) ** 2)) / r_eff) / E if r_eff > 0 else np.nan
    return out


def restate(ll, lens, r_eff=None):
    """The columns' restatements stacked: arrays (n,) by key ('log_weights' (S, n))."""
    ll = np.asarray(ll, dtype=np.float64)
    cols = [restate_column(ll[:, i], int(lens[i]), None if r_eff is None else float(r_eff[i])) for i in range(ll.shape[1])]
    return {k: np.stack([c[k] for c in cols], axis=-1) for k in cols[0]}


def tail_lengths(r_eff, S):
    return lsc.tail_lengths(r_eff, S)


# ---- the exact selection -----------------------------------------------------------------------------------------------------
def keys(a32):
    """The monotone uint32 key of every float32 (csrc/radix_select.hpp `radix_key`)."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    b = a32.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    k[np.isnan(a32)] = np.uint32(0xFFFFFFFF)
    return k


def select_exact(ll32, lens):
    """What `l2hmc_loglik_tails` must return: {'cutoff', 'top' (n,) float32, 'n_tail' (n,) int64, 'pairs': per column the sorted
    list of (key, draw) of the tail}."""
    ll32 = np.ascontiguousarray(ll32, dtype=np.float32)
    S, n = ll32.shape
    k = keys(ll32)
    order = np.argsort(k, axis=0, kind="stable")
    cut = order[np.asarray(lens), np.arange(n)]
    cutoff = ll32[cut, np.arange(n)]
    top = ll32[order[S - 1], np.arange(n)]
    ckey = k[cut, np.arange(n)]
    below = k < ckey[None, :]
    pairs = [sorted((int(k[s, i]), int(s)) for s in np.nonzero(below[:, i])[0]) for i in range(n)]
    return {"cutoff": cutoff, "top": top, "n_tail": below.sum(axis=0).astype(np.int64), "pairs": pairs, "in_tail": below}


def sum_bounds(ll32, exact):
    """(ref (3, n), bound (3, n)) of body, body_sq, lik (module docstring), in numpy.longdouble."""
    ld = np.longdouble
    eps_ld = float(np.finfo(ld).eps)
    ll = np.asarray(ll32, dtype=ld)
    S = ll.shape[0]
    c, top = np.asarray(exact["cutoff"], dtype=ld), np.asarray(exact["top"], dtype=ld)
    out_of_tail = ~exact["in_tail"]
    ref, bound = [], []
    with np.errstate(all="ignore"):
        for a, dist, mask in ((c[None, :] - ll, c[None, :] - ll, out_of_tail), (2 * (c[None, :] - ll), c[None, :] - ll, out_of_tail),
                              (ll - top[None, :], ll - top[None, :], np.ones_like(out_of_tail))):
            t = np.where(mask, np.exp(a), ld(0))
            total = t.sum(axis=0)
            # a term that is zero (a draw at -inf under a finite cutoff or maximum: e^-inf; a tail member) is exact and adds a
            # zero bound -- not 0 x its infinite distance, a NaN
            per_term = np.where(t == 0, ld(0), t * (np.abs(dist) + 2) * (ld(2.0) ** -52 + eps_ld)).sum(axis=0)
            ref.append(total.astype(np.float64))
            bound.append((per_term + S * ld(2.0) ** -53 * total).astype(np.float64))
    return np.stack(ref), np.stack(bound)


def sums_within(got, ref, bound):
    """The sums of a matrix that holds -inf: NaN exactly where the reference is NaN (a draw at -inf outside the tail of a column
    whose cutoff is -inf: e^(-inf + inf)), and within the bound everywhere else."""
    got, nan = np.asarray(got), np.isnan(ref)
    with np.errstate(all="ignore"):
        return bool(np.array_equal(np.isnan(got), nan) and np.all((np.abs(got - ref) <= bound)[~nan]))


def minus_inf_matrix():
    """(ll (70, 3) float32, lens): `matrix(70, 3)` with two -inf in column 1 (fewer than the tail length 14: they are tail
    members under a finite cutoff) and twenty in column 2 (more: the cutoff is -inf, the tail is empty, body is NaN)."""
    ll = matrix(70, 3)
    ll[[3, 41], 1] = -np.inf
    ll[5:65:3, 2] = -np.inf
    assert np.isneginf(ll).sum(axis=0).tolist() == [0, 2, 20]
    return ll


# ---- the device entries, straight (need a GPU) -------------------------------------------------------------------------------
def device_raw(ll32, lens=None, want_pos=True, explicit_stride=None):
    """`l2hmc_loglik_tails` on a float32 (S, n <= 512) matrix, outputs filled with NaN / -7 before the call so that an element
    the kernel does not write shows: {'cutoff', 'top', 'n_tail', 'tail', 'tail_pos', 'sums' (3, n), 'flag'} numpy."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd._history import launch, workspace
    from l2hmc_amd._pareto import loo_tail_len
    S, n = ll32.shape
    X = torch.as_tensor(np.ascontiguousarray(ll32, dtype=np.float32)).cuda()
    dev, L = X.device, _ffi.lib()
    stride = explicit_stride if explicit_stride is not None else (loo_tail_len(S) if lens is None else int(np.max(lens)))
    lens_d = None if lens is None else torch.as_tensor(np.ascontiguousarray(lens, dtype=np.int64)).to(dev)
    ws = workspace(dev, torch.uint8, L.l2hmc_loglik_tails_workspace_bytes, S, n)
    cutoff = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    top = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    n_tail = torch.full((n,), -7, dtype=torch.int64, device=dev)
    tail = torch.full((n, stride), float("nan"), dtype=torch.float32, device=dev)
    pos = torch.full((n, stride), -7, dtype=torch.int64, device=dev) if want_pos else None
    sums = torch.full((3, n), float("nan"), dtype=torch.float64, device=dev)
    launch(dev, L.l2hmc_loglik_tails, X.data_ptr(), S, n, None if lens_d is None else lens_d.data_ptr(), stride, cutoff.data_ptr(),
           top.data_ptr(), n_tail.data_ptr(), tail.data_ptr() if stride else None, pos.data_ptr() if want_pos and stride else None,
           sums.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    return {"cutoff": cutoff.cpu().numpy(), "top": top.cpu().numpy(), "n_tail": n_tail.cpu().numpy(), "tail": tail.cpu().numpy(),
            "tail_pos": None if pos is None else pos.cpu().numpy(), "sums": sums.cpu().numpy(),
            "flag": int(ws[:8].view(torch.int64)[0])}


def device_chain_stats(X, max_lag, split, shift=None):
    """(mean, m2, G) float64 numpy of `l2hmc_chain_stats` (shift None) or `l2hmc_chain_stats_exp` on a float32 device history."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd._history import launch, workspace
    M, N, d = (int(v) for v in X.shape)
    dev, L = X.device, _ffi.lib()
    C = N * (2 if split else 1)
    ws = workspace(dev, torch.float64, L.l2hmc_chain_stats_workspace_doubles, M, N, d, max_lag, int(split))
    mean = torch.full((C, d), float("nan"), dtype=torch.float64, device=dev)
    m2 = torch.full((C, d), float("nan"), dtype=torch.float64, device=dev)
    G = torch.full((d, max_lag + 1), float("nan"), dtype=torch.float64, device=dev)
    out = (mean.data_ptr(), m2.data_ptr(), G.data_ptr(), ws.data_ptr())
    if shift is None:
        launch(dev, L.l2hmc_chain_stats, X.data_ptr(), M, N, d, max_lag, int(split), *out)
    else:
        launch(dev, L.l2hmc_chain_stats_exp, X.data_ptr(), M, N, d, max_lag, int(split), shift.data_ptr(), *out)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), m2.cpu().numpy(), G.cpu().numpy()
