"""Shared by tests/test_lik_stats_cpu.py, tests/test_gpu_lik_stats.py and tools/lik_stats_accuracy.py: seeded AR(1) histories
for the per-row relative efficiency of PSIS-LOO, a float64 restatement written from the definitions (independent of
l2hmc_amd/predictive.py and l2hmc_amd/diagnostics.py: one row at a time, explicit per-chain autocovariances) and the bounds of
the device path, derived from the inputs alone.

Definitions, for a history W (M, N, d), rows X (n, d), labels y: lik[t, c, i] = sigmoid((2 y_i - 1) x_i . w[t, c]).  With
`split` every chain is two series, rows [0, Mh) and [M - Mh, M), Mh = M // 2 (first halves, then second halves); else Mh = M.
Per row, over its C series of length Mh: m_c the mean, M2_c = sum (lik - m_c)^2, G_c[t] = sum_{s < Mh - t} (lik_s - m_c)
(lik_{s+t} - m_c); Wv = mean_c M2_c / (Mh - 1), B = Mh var_c(m_c) (ddof 1), varp = (Mh - 1) / Mh Wv + B / Mh,
rho_t = 1 - (Wv - mean_c G_c[t] / (Mh - 1)) / varp; pairs P_j = rho_2j + rho_2j+1 (j < (max_lag + 1) // 2) up to the first
P_j <= 0 -- K is that j, or the number of pairs when there is none (`truncated`) -- replaced by their running minimum;
tau = -1 + 2 sum_{j < K} P_j, ess = C Mh / tau, r_eff = ess / (M N).  A series that is constant or not finite: NaN.

The device bounds of the raw sums, with eps = 2^-24: e_si = lik_si B_si (B of tests/predictive_case.py: the float32 logit and
the hardware sigmoid carried to the likelihood) bounds the error of one likelihood.  Per (chain, row), sums over the series:
    |d mean| <= mean_t e        |d M2| <= 2 sqrt(M2 sum e^2) + sum e^2      (Cauchy-Schwarz on sum (z + e')^2 - sum z^2)
    |d G_t|  <= sum_c [2 sqrt(M2_c sum e^2) + sum e^2] + 64 eps G_0
The last term covers the float32 centring (one rounding per factor: 2 eps per product) and the float32 accumulation of 8
products before each fold into float64 (<= 8 eps of sum |products| <= G_0, Cauchy-Schwarz) -- 10 eps G_0 as built, inside the
64 eps that csrc/chain_stats.hip's arithmetic (32 steps per fold) is given.

The finished r_eff is not Lipschitz in the logits (the truncation index K is discrete), so it is gated by a MEASURED
sensitivity: K_REFF below, and rows whose K moves under the perturbations are excluded (`near_boundary`)."""
import math

import numpy as np

from tests import loo_case as lc
from tests import predictive_case as pc

EPS = 2.0 ** -24
MAX_LOGIT = 6.0
EXCLUDED_AT_MOST = 0.10   # of a fixture's rows may sit so near a truncation boundary that +-delta_si moves their K

# The worst |relative change| / delta_i of r_eff of the float64 route under +-delta_si perturbations of the logits, over
# FIXTURES and 8 seeded sign patterns (rows whose truncation index moves excluded), times 4 (sampled sign patterns
# under-estimate the worst case): tools/lik_stats_accuracy.py measures it on the CPU, profiles/lik_stats_accuracy.txt records it.
K_REFF = 4 * 3.9          # worst measured 3.872, on (40, 5, 2, 0.5, 19, False)
# the same for n_eff and mcse_elpd_loo_i of `loo(r_eff="auto")` (relative changes; r_eff and with it M_i move with the logits)
K_NEFF = 4 * 3.9          # worst measured 3.875, on (40, 5, 2, 0.5, 19, False)
K_MCSE = 4 * 1.9          # worst measured 1.810, on (40, 5, 2, 0.5, 19, False)
# the device finishes against the numpy finish on the same tails: 100 x the worst difference measured on the MI355X
# (profiles/lik_stats_accuracy.txt), never looser than 1e-6 (the rule of FINISH_KHAT in tests/loo_case.py); relative
FINISH_NEFF = 6.7e-12     # worst measured 6.61e-14, on (200, 20, 3, 0.7, 63, False), finish="kernel"
FINISH_MCSE = 6.2e-12     # worst measured 6.11e-14, on (40, 5, 2, 0.5, 19, False)

# (M, N, d, rho, max_lag, split), all with N_ROWS rows.  Between them: every NTM geometry (d = 2, 3 -> 1; 17 -> 2; 40 -> 4;
# 100 -> 8), chains below (5), at (16) and above one 16-chain tile with a ragged last tile (18, 20, 35) and without (48), three
# row blocks, max_lag + 1 on a multiple of the kernel's 8-lag tile (63, 31, 39), one past it (32) and inside it (33, 19), both
# halves of a split with an odd number of steps.
N_ROWS = 37
FIXTURES = [(200, 20, 3, 0.7, 63, False), (200, 20, 17, 0.7, 63, False), (96, 35, 40, 0.5, 33, False),
            (64, 18, 100, 0.3, 31, False), (200, 20, 3, 0.0, 63, False), (40, 5, 2, 0.5, 19, False),
            (64, 48, 17, 0.5, 31, False), (48, 16, 5, 0.5, 32, False), (81, 20, 3, 0.3, 39, True)]
# the r_eff each fixture was chosen for (float64, `diagnostics.summarize(lik, split=False)`), where the issue records one
R_EFF_RANGE = {(200, 20, 3, 0.7, 63, False): (0.15, 0.20), (200, 20, 17, 0.7, 63, False): (0.14, 0.23),
               (96, 35, 40, 0.5, 33, False): (0.29, 0.40), (64, 18, 100, 0.3, 31, False): (0.46, 0.70),
               (200, 20, 3, 0.0, 63, False): (0.87, 1.07)}
MAY_TRUNCATE = (200, 20, 17, 0.7, 63, False)      # at most one truncated row; none anywhere else


def seed_of(M, N, d, rho):
    return 3000 + M + N + d + int(round(100 * rho))


def ar1_case(M, N, d, rho, n=N_ROWS, seed=None):
    """(W (M, N, d), X (n, d), y (n,)) float32: every chain an AR(1) series W_t = rho W_{t-1} + sqrt(1 - rho^2) eps_t about a
    common offset, scaled so that the largest |logit| is 6; rows and labels as predictive_case.case makes them."""
    rng = np.random.RandomState(seed_of(M, N, d, rho) if seed is None else seed)
    X = rng.randn(n, d)
    eps = rng.randn(M, N, d)
    W = np.empty((M, N, d))
    W[0] = eps[0]
    for t in range(1, M):
        W[t] = rho * W[t - 1] + math.sqrt(1.0 - rho * rho) * eps[t]
    W += 0.5 * rng.randn(d)
    W *= MAX_LOGIT / np.abs(W.reshape(-1, d) @ X.T).max()
    y = (rng.rand(n) < 0.5).astype(np.float64)
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32)


def exact_case(M, N, d, n, seed):
    """Small-integer W and dyadic X (tests/loo_case.py `exact_case`): every product and partial sum is exact in float32, so the
    device's logits equal the float64 ones bit for bit, with many ties."""
    rng = np.random.RandomState(seed)
    W = rng.randint(-4, 5, size=(M, N, d)).astype(np.float32)
    X = (rng.randint(-8, 9, size=(n, d)) / 4.0).astype(np.float32)
    y = (rng.rand(n) < 0.5).astype(np.float32)
    return W, X, y


def signed_logits(W, X, y):
    """(M, N, n) float64"""
    W, X, y = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    return (W @ X.T) * (2.0 * y - 1.0)


def likelihoods(t):
    with np.errstate(all="ignore"):
        return np.exp(-np.logaddexp(0.0, -t))


def series_of(a, split):
    """(Mh, C, ...) of an (M, N, ...) array: whole chains, or first halves then second halves."""
    M = a.shape[0]
    Mh = M // 2 if split else M
    return np.concatenate([a[:Mh], a[M - Mh:]], axis=1) if split else a


def raw_sums(lik, max_lag, split):
    """(mean (C, n), m2 (C, n), Gc (C, n, max_lag + 1)) float64 of lik (M, N, n): G kept apart by chain."""
    S = series_of(np.asarray(lik, dtype=np.float64), split)
    Mh = S.shape[0]
    with np.errstate(all="ignore"):
        mean = S.mean(axis=0)
        Z = S - mean
        m2 = (Z * Z).sum(axis=0)
        Gc = np.stack([(Z[:Mh - t] * Z[t:]).sum(axis=0) for t in range(max_lag + 1)], axis=-1)
    return mean, m2, Gc


def restate_row(series, max_lag):
    """(ess, K, truncated) of one row from its (Mh, C) likelihood series, the direct form: explicit per-chain autocovariances."""
    Mh, C = series.shape
    with np.errstate(all="ignore"):
        m = series.mean(axis=0)
        z = series - m
        m2 = np.array([float(np.dot(z[:, c], z[:, c])) for c in range(C)])
        Wv = m2.mean() / (Mh - 1)
        B = Mh * m.var(ddof=1)
        varp = (Mh - 1) / Mh * Wv + B / Mh
        rho = np.empty(max_lag + 1)
        for t in range(max_lag + 1):
            acov = np.array([float(np.dot(z[:Mh - t, c], z[t:, c])) for c in range(C)]) / (Mh - 1)
            rho[t] = 1.0 - (Wv - acov.mean()) / varp
    if not (np.isfinite(Wv) and np.isfinite(varp) and np.all(np.isfinite(rho)) and Wv > 0):
        return np.nan, -1, False
    n_pairs = (max_lag + 1) // 2
    tau, K, low = -1.0, n_pairs, np.inf
    for j in range(n_pairs):
        P = rho[2 * j] + rho[2 * j + 1]
        if P <= 0:
            K = j
            break
        low = min(low, P)
        tau += 2.0 * low
    return C * Mh / tau, K, K == n_pairs


def restatement(W, X, y, max_lag, split, t=None):
    """{'r_eff', 'ess' (n,), 'K' (n,) int, 'truncated' (n,) bool}; `t` (M, N, n) replaces the logits (the sensitivity runs)."""
    t = signed_logits(W, X, y) if t is None else t
    S = series_of(likelihoods(t), split)
    rows = [restate_row(S[:, :, i], max_lag) for i in range(S.shape[2])]
    ess = np.array([r[0] for r in rows])
    return {"ess": ess, "r_eff": ess / (t.shape[0] * t.shape[1]), "K": np.array([r[1] for r in rows]),
            "truncated": np.array([r[2] for r in rows], dtype=bool)}


def tail_lengths(r_eff, S):
    """M_i = min(S // 5, ceil(3 sqrt(S / r_eff_i))), r_eff_i taken as 1 where it is NaN or <= 0."""
    r = np.asarray(r_eff, dtype=np.float64)
    r = np.where(np.isfinite(r) & (r > 0), r, 1.0)
    return np.minimum(S // 5, np.ceil(3.0 * np.sqrt(S / r))).astype(np.int64)


def delta(W, X):
    """(delta_i (n,), delta_si (M, N, n)): the bound of the float32 logit error (tests/loo_case.py `delta`)."""
    W, X = np.asarray(W, dtype=np.float64), np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    D = (d + 8) * EPS * (np.abs(W) @ np.abs(X).T)
    return D.reshape(-1, X.shape[0]).max(axis=0), D


_SENS = {}


def sensitivity(fixture):
    """(ref, near_boundary (n,) bool, worst |relative change of r_eff| / delta_i over the other rows) of a fixture: the float64
    route under logits moved by +-delta_si, 8 seeded sign patterns.  A row is near a boundary when any pattern moves its K."""
    if fixture not in _SENS:
        M, N, d, rho, max_lag, split = fixture
        W, X, y = ar1_case(M, N, d, rho)
        t = signed_logits(W, X, y)
        ref = restatement(W, X, y, max_lag, split, t)
        di, dsi = delta(W, X)
        moved = np.zeros(t.shape[2], dtype=bool)
        change = np.zeros(t.shape[2])
        for pattern in range(8):
            sign = np.where(np.random.RandomState(100 * pattern + M).rand(*t.shape) < 0.5, -1.0, 1.0)
            per = restatement(W, X, y, max_lag, split, t + sign * dsi)
            moved |= per["K"] != ref["K"]
            with np.errstate(all="ignore"):
                change = np.maximum(change, np.abs(per["r_eff"] / ref["r_eff"] - 1.0) / di)
        worst = float(np.max(change[~moved])) if (~moved).any() else 0.0
        _SENS[fixture] = (ref, moved, worst)
    return _SENS[fixture]


def raw_bounds(W, X, y, max_lag, split, exact=False):
    """Float64 references and bounds of the kernel's raw sums (module docstring): {'mean', 'm2' (C, n), 'G' (n, max_lag + 1)} and
    {'mean', 'm2', 'G'} of the same shapes.  `exact`: the inputs of `exact_case`, whose float32 logits carry no error -- B keeps
    only its second term, 8 eps (1 + |ll|), the hardware sigmoid."""
    M, N, d = W.shape
    b = pc.device_bounds(W.reshape(M * N, d), X, y)
    lik = np.exp(b["ll"]).reshape(M, N, -1)
    B = 8 * EPS * (1.0 + np.abs(b["ll"])) if exact else b["B"]
    e = series_of(lik * B.reshape(M, N, -1), split)
    mean, m2, Gc = raw_sums(lik, max_lag, split)
    se2 = (e * e).sum(axis=0)
    bm2 = 2.0 * np.sqrt(m2 * se2) + se2
    G = Gc.sum(axis=0)
    ref = {"mean": mean, "m2": m2, "G": G}
    bound = {"mean": e.mean(axis=0), "m2": bm2, "G": (bm2.sum(axis=0) + 64 * EPS * G[:, 0])[:, None] + np.zeros_like(G)}
    return ref, bound


def restate_loo_row(t, r_eff):
    """(elpd_loo_i, khat, n_tail, n_eff, mcse, M_i) of one row from its S signed logits and its r_eff, the direct form: a full
    sort, the tail `lw > cutoff` with M_i from r_eff, smoothed weights written back into all S log weights, n_eff and mcse from
    the normalised weight vector (no body / tail decomposition)."""
    S = len(t)
    ll = -np.logaddexp(0.0, -t)
    lw = -ll
    M = int(tail_lengths(np.array([r_eff]), S)[0])
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
    with np.errstate(all="ignore"):
        w = np.exp(lw - np.logaddexp.reduce(lw))
        lik = np.exp(ll)
        E = float(np.sum(w * lik))
        n_eff = r_eff / float(np.sum(w * w))
        mcse = math.sqrt(float(np.sum(w * w * (lik - E) ** 2)) / r_eff) / E if r_eff == r_eff and r_eff > 0 else np.nan
    return math.log(E), khat, L, n_eff, mcse, M


def restate_loo(t, r_eff):
    """{'elpd_loo_i', 'khat', 'n_tail', 'n_eff', 'mcse', 'tail_len_row'} (n,) of logits t (M, N, n) and r_eff (n,)."""
    flat = t.reshape(-1, t.shape[-1])
    rows = [restate_loo_row(flat[:, i], float(r_eff[i])) for i in range(flat.shape[1])]
    keys = ("elpd_loo_i", "khat", "n_tail", "n_eff", "mcse", "tail_len_row")
    return {k: np.array([r[j] for r in rows]) for j, k in enumerate(keys)}


_LOO_SENS = {}


def loo_sensitivity(fixture):
    """(ref, worst |relative change of n_eff| / delta_i, the same of mcse) of `loo(r_eff="auto")` in the float64 restatement
    under the perturbations of `sensitivity` (r_eff is computed again from the moved logits), over the rows whose truncation
    index does not move."""
    if fixture not in _LOO_SENS:
        M, N, d, rho, max_lag, split = fixture
        W, X, y = ar1_case(M, N, d, rho)
        t = signed_logits(W, X, y)
        auto = min(M - 1, 255)                                # `relative_eff`'s defaults inside loo(r_eff="auto")
        r0 = restatement(W, X, y, auto, False, t)
        ref = restate_loo(t, r0["r_eff"])
        di, dsi = delta(W, X)
        moved = np.zeros(t.shape[2], dtype=bool)
        cn, cm = np.zeros(t.shape[2]), np.zeros(t.shape[2])
        for pattern in range(8):
            sign = np.where(np.random.RandomState(100 * pattern + M).rand(*t.shape) < 0.5, -1.0, 1.0)
            tp = t + sign * dsi
            rp = restatement(W, X, y, auto, False, tp)
            per = restate_loo(tp, rp["r_eff"])
            moved |= rp["K"] != r0["K"]
            with np.errstate(all="ignore"):
                cn = np.maximum(cn, np.abs(per["n_eff"] / ref["n_eff"] - 1.0) / di)
                cm = np.maximum(cm, np.abs(per["mcse"] / ref["mcse"] - 1.0) / di)
        keep = ~moved
        _LOO_SENS[fixture] = (dict(ref, r_eff=r0["r_eff"]), moved, float(cn[keep].max()), float(cm[keep].max()))
    return _LOO_SENS[fixture]


def device_raw(W, X, y, max_lag, split):
    """(mean (C, n), m2 (C, n), G (n, max_lag + 1)) float64 numpy, straight from `l2hmc_logistic_lik_stats` (needs a GPU);
    the outputs are filled with NaN before the call, so an element the kernel does not write shows."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd._history import launch, workspace
    from l2hmc_amd.predictive import _device_packer
    M, N, d = W.shape
    n = X.shape[0]
    Wd = torch.as_tensor(W).cuda()
    dev = Wd.device
    packed = _device_packer(dev, X, y, n, d, "test")(0, n)
    L = _ffi.lib()
    C = N * (2 if split else 1)
    ws = workspace(dev, torch.uint8, L.l2hmc_logistic_lik_stats_workspace_bytes, M, N, d, n, max_lag, int(split))
    mean = torch.full((C, n), float("nan"), dtype=torch.float64, device=dev)
    m2 = torch.full((C, n), float("nan"), dtype=torch.float64, device=dev)
    G = torch.full((n, max_lag + 1), float("nan"), dtype=torch.float64, device=dev)
    launch(dev, L.l2hmc_logistic_lik_stats, Wd.data_ptr(), M, N, d, packed.data_ptr(), n, max_lag, int(split), mean.data_ptr(),
           m2.data_ptr(), G.data_ptr(), ws.data_ptr())
    return mean.cpu().numpy(), m2.cpu().numpy(), G.cpu().numpy()
