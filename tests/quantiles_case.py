"""Shared by tests/test_quantiles_cpu.py and tests/test_gpu_quantiles.py: an adversarial history and a restatement of
`l2hmc_amd.quantiles` written from the definitions, one coordinate at a time, independently of the module (whose numpy path
and HIP kernels are both held against it).  The AR(1) fixtures and the ESS estimator are those of tests/diagnostics_case.py.

 - order statistics: `np.sort` of the float32 column, indexed;
 - quantiles: `np.quantile` (numpy's default definition) of the column as float64;
 - ess_quantile(p): the estimator of diagnostics_case.reference_summary on the indicator history [x <= Q_p] (float64 compare);
 - ess_tail: the smaller of ess_quantile(0.05) and ess_quantile(0.95);
 - mcse_mean: sd / sqrt(ess);
 - mcse_quantile(p): with ess = ess_quantile(p), a = betaincinv(ess p + 1, ess (1 - p) + 1, [0.1586553, 0.8413447]),
   i1 = max(floor(a1 S), 1), i2 = min(ceil(a2 S), S) (1-based positions of the sorted draws), (x_(i2) - x_(i1)) / 2."""
import numpy as np

from tests import diagnostics_case as dc

PROBS = (0.05, 0.5, 0.95)
NAN_COORDINATE = 11


def adversarial():
    """Fixture "F" (96 x 77 x 17, N d = 1309) with one hostile coordinate each; coordinate 0 and 12 .. 16 stay as they are."""
    X, max_lag = dc.fixture("F")
    Y = X.copy()
    rng = np.random.RandomState(17)
    shape = Y.shape[:2]
    Y[:, :, 1] = 2.5                                                    # a constant
    Y[:, :, 2] = np.round(Y[:, :, 2] * 2) / 2                           # multiples of 0.5: heavy ties
    Y[:, :, 3] = np.where(rng.rand(*shape) < 0.5, np.float32(0.0), np.float32(-0.0))      # a +-0 mix
    Y[3, 5, 4], Y[70, 20, 4] = np.inf, -np.inf                          # one of each
    Y[:, :, 5] = (np.uint32(0x3FC00000) | rng.randint(0, 256, size=shape).astype(np.uint32)).view(np.float32)   # top 24 bits equal
    Y[:, :, 6] = -np.abs(Y[:, :, 6]) - np.float32(0.125)                # all negative
    Y[:, :, 7] = (rng.randint(1, 1 << 20, size=shape).astype(np.uint32)
                  | (rng.randint(0, 2, size=shape).astype(np.uint32) << np.uint32(31))).view(np.float32)        # denormals, both signs
    Y[40, 7, NAN_COORDINATE] = np.nan
    return Y, max_lag


# The shapes that reach the branches of csrc/order_stats.hip's plan which the fixtures of diagnostics_case do not; the plan of
# each is derived in tests/test_gpu_quantiles.py.  name -> (M, N, d, seed)
PLAN_FIXTURES = {
    "long-walk-d70": (140, 1000, 70, 30),    # every block walks 17 to 124 steps; hostile values in coordinates 1 .. 7 and 69
    "groups-d512": (9, 500, 512, 31),        # the widest history the entry accepts: 8 coordinate groups of 64
    "copies-d3": (300, 100, 3, 32),          # 21 histogram copies of 3 coordinates, the last thread of a block idle
}
LONG_WALK_NAN_COORDINATE = 69


def plan_history(name):
    """float32 (M, N, d), every coordinate with its own phi, mean and sd (diagnostics_case.spread).  "long-walk-d70" carries the
    hostile coordinates of `adversarial` -- ties, a +-0 mix, +-inf, equal top 24 bits, denormals -- and one NaN in its LAST
    coordinate, which belongs to the second coordinate group of the count passes."""
    M, N, d, seed = PLAN_FIXTURES[name]
    phi, mean, sd = dc.spread(d)
    Y = dc.ar1(M, N, phi, seed, mean, sd)
    if name == "long-walk-d70":
        rng = np.random.RandomState(seed + 1000)
        shape = Y.shape[:2]
        Y[:, :, 1] = 2.5                                                # a constant
        Y[:, :, 2] = np.round(Y[:, :, 2] * 2) / 2                       # multiples of 0.5: heavy ties
        Y[:, :, 3] = np.where(rng.rand(*shape) < 0.5, np.float32(0.0), np.float32(-0.0))  # a +-0 mix
        Y[3, 5, 4], Y[70, 20, 4], Y[139, 999, 4] = np.inf, -np.inf, np.inf                # the last draw of all among them
        Y[:, :, 5] = (np.uint32(0x3FC00000) | rng.randint(0, 256, size=shape).astype(np.uint32)).view(np.float32)
        Y[:, :, 6] = -np.abs(Y[:, :, 6]) - np.float32(0.125)            # all negative
        Y[:, :, 7] = (rng.randint(1, 1 << 20, size=shape).astype(np.uint32)
                      | (rng.randint(0, 2, size=shape).astype(np.uint32) << np.uint32(31))).view(np.float32)    # denormals
        Y[137, 993, LONG_WALK_NAN_COORDINATE] = np.nan
    return Y


def draws(X):
    return np.ascontiguousarray(X, dtype=np.float32).reshape(-1, X.shape[-1])


def standard_ranks(S):
    return np.array([0, 1, S // 2, S - 2, S - 1], dtype=np.int64)


def rank_table(S, d, seed=0, R=32):
    """(32, d): different ranks for every coordinate, the extremes included."""
    t = np.random.RandomState(seed).randint(0, S, size=(R, d)).astype(np.int64)
    t[0], t[-1] = 0, S - 1
    return t


def reference_order_statistics(X, ranks):
    X2 = draws(X)
    S, d = X2.shape
    ranks = np.asarray(ranks, dtype=np.int64)
    if ranks.ndim == 1:
        ranks = np.repeat(ranks[:, None], d, axis=1)
    out = np.empty(ranks.shape, dtype=np.float32)
    for k in range(d):
        out[:, k] = np.sort(X2[:, k])[ranks[:, k]]                      # NaNs last
    return out, np.isnan(X2).sum(axis=0)


def reference_quantiles(X, probs):
    X2 = draws(X).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([np.quantile(X2[:, k], probs) for k in range(X2.shape[1])], axis=1)


def indicator_history(X, thresholds):
    with np.errstate(invalid="ignore"):
        return (np.asarray(X, dtype=np.float64) <= np.asarray(thresholds, dtype=np.float64)).astype(np.float64)


def reference_mcse_quantile(column_sorted, ess, p):
    from scipy.special import betaincinv
    if not np.isfinite(ess):
        return np.nan
    S = column_sorted.shape[0]
    a1, a2 = (betaincinv(ess * p + 1, ess * (1 - p) + 1, c) for c in (0.1586553, 0.8413447))
    i1, i2 = max(int(np.floor(a1 * S)), 1), min(int(np.ceil(a2 * S)), S)
    return (float(column_sorted[i2 - 1]) - float(column_sorted[i1 - 1])) / 2


def reference_describe(X, max_lag, split=True, probs=PROBS):
    """{'base': reference_summary of X, 'quantiles' (Q, d), 'ess_quantile', 'tau_quantile', 'truncated_quantile' (Q, d),
    'below' [per p: reference_summary of the indicator history], 'ess_tail', 'mcse_mean' (d), 'mcse_quantile' (Q, d)}"""
    X2 = draws(X)
    d = X2.shape[1]
    every = list(probs) + [t for t in (0.05, 0.95) if t not in probs]
    q = reference_quantiles(X, every)
    below = [dc.reference_summary(indicator_history(X, q[i]), max_lag, split) for i in range(len(every))]
    ess = np.stack([b["ess"] for b in below])
    base = dc.reference_summary(X, max_lag, split)
    Q = len(probs)
    mcse = np.full((Q, d), np.nan)
    for k in range(d):
        col = np.sort(X2[:, k])
        if np.isnan(col).any():
            continue
        for i, p in enumerate(probs):
            mcse[i, k] = reference_mcse_quantile(col, ess[i, k], p)
    with np.errstate(all="ignore"):
        return {"base": base, "probs": np.array(probs), "quantiles": q[:Q], "ess_quantile": ess[:Q], "below": below[:Q],
                "tau_quantile": np.stack([b["tau"] for b in below[:Q]]),
                "truncated_quantile": np.stack([b["truncated"] for b in below[:Q]]),
                "ess_tail": np.minimum(ess[every.index(0.05)], ess[every.index(0.95)]),
                "mcse_mean": base["sd"] / np.sqrt(base["ess"]), "mcse_quantile": mcse}
