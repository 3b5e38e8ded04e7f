"""Shared by tests/test_psis_cpu.py, tests/test_gpu_psis.py and tools/psis_accuracy.py: tails built directly in numpy (no draws,
no sampler), a row-at-a-time float64 restatement of PSIS on `loo_case._gpdfit` and in the manner of `loo_case.restate_row`
(independent of l2hmc_amd/psis.py and of `_pareto._psis_rows`: another summation order -- `np.mean`, `np.logaddexp.reduce`
-- and another formation of x and of the ratios), and the gates of the kernel.

A tail.  `tail(M, L, k_true, seed)` draws L importance ratios cutoff_ratio + GPD(k_true, sigma = 1) quantiles at sorted
uniform p, turns them into signed logits t with softplus(-t) = log ratio, and lays them on the float32 grid, strictly
ascending and strictly before the cutoff logit t_c = 0 -- what `predictive.loo_tails` returns for a row.  `tails(...)` stacks
rows into the raw dict of `loo_tails` (float32 cutoff and tail with +inf pads in shuffled slot order, a body sum and a
likelihood sum that a history of S = 10 M + 10 draws could have produced), which `predictive.loo_finish` finishes by any of
its routes.

The gates.  Nothing is taken from the kernel: tools/psis_accuracy.py measures, on the CPU, the disagreement of the two float64
host references (the module's numpy path and the restatement here) per tested tail length over the five k_true, `MEASURED`
holds the figures, and `gate(M)` = 100 x the worst disagreement at any tail length up to M, under one absolute cap of 1e-9 for
khat and for elpd_loo_i whatever was measured.  "Up to M" because a single length's figure is one sample of rounding noise (at
M = 6 the references happened to agree on khat to one ulp, at M = 5 they differ by twelve), while the error of a sum grows with
its length: the running maximum is the references' own error at M or shorter, never a longer tail's.  The margin is 100 because
the kernel has a third summation tree and the device's log1p / exp / log; it is the margin the project already gives its torch
finish.  profiles/psis_accuracy.txt records the run."""
import math

import numpy as np

from tests import loo_case as lc

K_TRUE = (-0.3, 0.0, 0.3, 0.7, 1.2)
CAP = 1e-9
MARGIN = 100.0

# tail length -> the worst |numpy path - restatement| of (khat, elpd_loo_i) over K_TRUE x 3 seeds and shorter tails, and on the
# matrices and histories of the GPU tests with that tail length (tools/psis_accuracy.py on the CPU; profiles/psis_accuracy.txt);
# every tail length a GPU test uses is here
MEASURED = {
    0: (0, 7.11e-15),
    3: (0, 8.88e-16),
    4: (0, 8.88e-16),
    5: (1.3e-15, 1.42e-14),
    6: (1.11e-16, 8.88e-16),
    7: (8.88e-16, 1.33e-15),
    14: (1.67e-15, 2.66e-15),
    52: (6.44e-15, 5.33e-15),
    63: (9.77e-15, 1.78e-15),
    64: (6e-15, 2.33e-15),
    65: (1.22e-14, 7.33e-15),
    69: (5e-15, 8.88e-15),
    193: (1.77e-14, 2.35e-14),
    255: (3.51e-14, 3.31e-14),
    256: (4.75e-14, 2.86e-14),
    257: (3.09e-14, 2.29e-14),
    769: (6.52e-14, 1.49e-13),
    6072: (3.08e-12, 1.12e-11),
    21467: (4.05e-12, 1.16e-11),
}


def gate(M):
    """(khat gate, elpd_loo_i gate) at tail length M: 100 x the worst disagreement of the references measured at any tail
    length up to M, at most 1e-9."""
    k = max(v[0] for m, v in MEASURED.items() if m <= M)
    e = max(v[1] for m, v in MEASURED.items() if m <= M)
    return min(MARGIN * k, CAP), min(MARGIN * e, CAP)


def draws_for(M):
    return 10 * M + 10


def tail(M, L, k_true, seed):
    """{'t': (L,) float32 ascending logits, 'lam': (M,) float64 descending log ratios in slots 0 .. L - 1 and NaN in the dead
    slots (never read), 'L': L, 't_c': 0.0, 'lam_c': log 2}."""
    assert 0 <= L <= M
    rng = np.random.RandomState(seed)
    p = np.sort(rng.uniform(0.0, 1.0, size=L))[::-1]                  # the largest ratio first
    with np.errstate(all="ignore"):
        x = -np.log1p(-p) if k_true == 0.0 else np.expm1(-k_true * np.log1p(-p)) / k_true
    lam = np.log(2.0 + x)                                             # the cutoff's ratio is softplus(-0) = log 2 -> ratio 2
    t = (-np.log(np.expm1(lam))).astype(np.float32)                   # softplus(-t) = lam
    t = np.minimum(t, np.float32(-2.0 ** -20))                        # strictly before the cutoff logit 0
    for i in range(L - 2, -1, -1):                                    # t ascends strictly: slot 0 the smallest logit
        if not t[i] < t[i + 1]:
            t[i] = np.nextafter(t[i + 1], np.float32(-np.inf))
    out = np.full(M, np.nan)
    out[:L] = np.logaddexp(0.0, -t.astype(np.float64))
    return {"t": t, "lam": out, "L": L, "t_c": 0.0, "lam_c": math.log(2.0)}


def tails(M, rows, seed=0):
    """The raw dict of `predictive.loo_tails` (numpy) for rows = [(L, k_true), ...]: the tail's slots shuffled as the device's
    gather leaves them, +inf past L."""
    rng = np.random.RandomState(1000 + seed)
    n, S = len(rows), draws_for(M)
    tl = np.full((n, M), np.inf, dtype=np.float32)
    for i, (L, k) in enumerate(rows):
        tl[i, :L] = rng.permutation(tail(M, L, k, seed + 17 * i)["t"])
    n_tail = np.array([L for L, _ in rows], dtype=np.int64)
    t_body = 1.0 + rng.rand(n)                                        # the other S - L draws: e^m + e^(m - t), m = min(c, 0) = 0
    body = (S - n_tail) * (1.0 + np.exp(-t_body))
    sum_lik = (S - n_tail) / (1.0 + np.exp(-t_body)) + 0.25 * n_tail
    return {"cutoff": np.zeros(n, dtype=np.float32), "n_tail": n_tail, "tail": tl, "body": body, "sum_lik": sum_lik,
            "tail_len": M, "n_draws": S}


def lam_of(raw):
    """(lam (n, M) descending with NaN in the dead slots, n_tail, lam_c (n,)) of a raw dict: the input of `smooth_tails`."""
    t = np.sort(raw["tail"].astype(np.float64), axis=1)
    with np.errstate(all="ignore"):
        lam = np.where(np.isfinite(t), np.logaddexp(0.0, -t), np.nan)
    return lam, raw["n_tail"], np.logaddexp(0.0, -raw["cutoff"].astype(np.float64))


def restate_tail(lam, L, lam_c):
    """(khat, omega (L,) in slot order, lse_w, lse_wl) of one row, the direct form: `loo_case.restate_row` from its line
    `lw = lw - mx` on, given the descending tail instead of all S ratios."""
    lam = np.asarray(lam, dtype=np.float64)[:L]
    mx = lam[0] if L else lam_c
    asc = (lam - mx)[::-1].copy()                                     # ascending, as `order` leaves them
    khat = np.inf
    if L >= 5:
        ec = np.exp(lam_c - mx)
        with np.errstate(all="ignore"):
            k, sigma = lc._gpdfit(np.exp(asc) - ec)
            if np.isfinite(k) and np.isfinite(sigma):
                p = (np.arange(1, L + 1) - 0.5) / L
                q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
                asc = np.minimum(np.log(q + ec), 0.0)
                khat = k
    omega = asc[::-1]
    with np.errstate(all="ignore"):
        lse_w = np.logaddexp.reduce(omega) if L else -np.inf
        lse_wl = np.logaddexp.reduce(omega - lam) if L else -np.inf
    if np.isnan(lse_w) or np.isnan(lse_wl):
        khat = np.nan
    return khat, omega, lse_w, lse_wl


def restate_finish(raw):
    """{'khat', 'elpd_loo_i'} (n,) of a raw dict, one row at a time: elpd = log(sum of w e^-lam over tail and body) -
    log(sum of w), the body's ratios summed in `body` as e^m + e^(m - t)."""
    lam, n_tail, lam_c = lam_of(raw)
    S = raw["n_draws"]
    khat, elpd = [], []
    for i in range(lam.shape[0]):
        L = int(n_tail[i])
        k, _, lse_w, lse_wl = restate_tail(lam[i], L, lam_c[i])
        mx = lam[i, 0] if L else lam_c[i]
        m = min(float(raw["cutoff"][i]), 0.0)
        with np.errstate(all="ignore"):
            e = np.logaddexp(math.log(S - L) - mx, lse_wl) - np.logaddexp(math.log(raw["body"][i]) - m - mx, lse_w)
        khat.append(k)
        elpd.append(e)
    return {"khat": np.array(khat), "elpd_loo_i": np.array(elpd)}


def restate_column(lw):
    """(smoothed log weights (S,) shifted so that the largest raw one is 0, khat, n_tail) of one column of log ratios:
    `loo_case.restate_row` without the logistic likelihood."""
    lw = np.asarray(lw, dtype=np.float64).copy()
    S = len(lw)
    M = lc.tail_len(S)
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
    return lw, khat, L


def restate_psis(r):
    """{'khat', 'n_tail', 'log_weights', 'log_sum', 'n_eff'} of (S, n) log ratios, one column at a time."""
    r = np.asarray(r, dtype=np.float64)
    cols = [restate_column(r[:, i]) for i in range(r.shape[1])]
    lw = np.stack([c[0] for c in cols], axis=1)
    return {"khat": np.array([c[1] for c in cols]), "n_tail": np.array([c[2] for c in cols], dtype=np.int64), "log_weights": lw,
            "log_sum": np.logaddexp.reduce(lw, axis=0),
            "n_eff": np.exp(2.0 * np.logaddexp.reduce(lw, axis=0) - np.logaddexp.reduce(2.0 * lw, axis=0))}


def restate_loo(ll):
    """{'khat', 'n_tail', 'elpd_loo_i', 'lppd_i'} of an (S, n) log-likelihood matrix, one column at a time."""
    ll = np.asarray(ll, dtype=np.float64)
    ps = restate_psis(-ll)
    w = ps["log_weights"]
    return {"khat": ps["khat"], "n_tail": ps["n_tail"],
            "elpd_loo_i": np.logaddexp.reduce(w + ll, axis=0) - np.logaddexp.reduce(w, axis=0),
            "lppd_i": np.logaddexp.reduce(ll, axis=0) - math.log(ll.shape[0])}


def log_lik_case(S, n, seed, ties=False):
    """A float32 (S, n) log-likelihood matrix with columns of different tail weight: -softplus of Gaussian logits whose scale
    grows with the column.  `ties`: column 0 gets a block of equal values around its cutoff, so that its tail is shorter
    than M."""
    rng = np.random.RandomState(seed)
    scale = 0.5 + 1.5 * np.arange(n) / max(n - 1, 1)
    t = rng.randn(S, n) * scale[None, :] + 1.0
    ll = (-np.logaddexp(0.0, -t)).astype(np.float32)
    if ties:
        M = lc.tail_len(S)
        order = np.argsort(ll[:, 0])                                   # ascending ll = descending ratio
        lo = max(M - 2, 0)
        ll[order[lo:M + 3], 0] = ll[order[M], 0]                       # ranks M - 2 .. M + 2 of the ratios all equal the cutoff
    return ll


def poisson_case(n=40, d=3, seed=11):
    """(X (n, d), y (n,)) float32 of a small Poisson regression with log link."""
    rng = np.random.RandomState(seed)
    X = (0.5 * rng.randn(n, d)).astype(np.float32)
    y = rng.poisson(np.exp(X.astype(np.float64) @ np.array([0.8, -0.5, 0.3])[:d] + 0.5)).astype(np.float32)
    return X, y


def poisson_log_lik(W, X, y):
    """(S, n) float64 numpy: y eta - e^eta - log y!, eta = w . x."""
    W, X, y = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    eta = W @ X.T
    return y[None, :] * eta - np.exp(eta) - np.array([math.lgamma(v + 1.0) for v in y])[None, :]


def _cycle(Ls, n):
    return [(Ls[i % len(Ls)], K_TRUE[(i // len(Ls) + i) % 5]) for i in range(n)]


# name -> (M, [(L, k_true), ...]): the tails tests/test_gpu_psis.py sends to the kernels.  The profile kernel's workgroup is 256
# threads (4 waves of 64) and a thread strides the tail by 256: L = 63 / 64 / 65 and 255 / 256 / 257 sit on both sides of a
# wave and of a workgroup; L = 0, 1, 4 are not fitted, 5 and 6 the smallest fits; every case but `full` has L < M rows (dead
# slots) and rows of different L (different theta grids) in one call; M = 21 467 has 176 theta in 22 blocks.
KERNEL_CASES = {
    "unfitted_and_smallest": (5, [(0, 0.0), (1, 0.3), (4, 0.7), (5, 1.2)]),
    "smallest_fits": (6, [(5, -0.3), (6, 0.3), (6, 1.2)]),
    "wave_boundary": (65, _cycle([63, 64, 65], 9)),
    "workgroup_boundary": (257, _cycle([255, 256, 257], 9)),
    "m769": (769, [(769, -0.3), (769, 0.7), (400, 1.2)]),
    "m6072": (6072, [(6072, 0.3), (6072, 0.0), (3000, 0.7)]),
    "m21467": (21467, [(21467, 0.7), (21467, -0.3), (10000, 1.2)]),
    "one_row": (64, [(64, 0.7)]),
    "more_workgroups_than_cus": (64, _cycle([64, 0, 5, 33, 63, 17, 4], 300)),
}
# further (n_rows, tail_len) launched there: tail_len = 0, the degenerate rows, the NaN row, and both sides of the row loop
EXTRA_KERNEL_SHAPES = [(2, 0), (3, 8), (3, 65), (65536, 5), (65539, 5)]
