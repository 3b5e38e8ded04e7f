"""Shared by tests/test_diagnostics_cpu.py and tests/test_gpu_diagnostics.py: the AR(1) fixtures of the convergence diagnostics
and a float64 restatement of the estimator -- split R-hat and the per-coordinate effective sample size of Vehtari, Gelman,
Simpson, Carpenter, Buerkner (2021) without rank normalisation -- written from its definition, one coordinate and one chain at a
time, independently of l2hmc_amd/diagnostics.py (whose numpy path and HIP kernels are both held against it).

The estimator, on a history X (M, N, d) read as float64:
 1. split: Mh = M // 2, every chain becomes rows [0, Mh) and rows [M - Mh, M): C = 2 N chains, first halves then second halves
    (unsplit: Mh = M, C = N);
 2. per chain c and coordinate k: mean m, M2 = sum_t (x_t - m)^2;
 3. W = mean_c M2 / (Mh - 1), B = Mh var_c(m) (ddof 1), varp = (Mh - 1) / Mh W + B / Mh, rhat = sqrt(varp / W), sd = sqrt(varp);
 4. G[k, t] = sum_c sum_{i < Mh - t} (x_i - m)(x_{i+t} - m), t = 0 .. max_lag;
 5. rho_t = 1 - (W - G[k, t] / (C (Mh - 1))) / varp, P_j = rho_2j + rho_2j+1 for j < (max_lag + 1) // 2, K = the first j with
    P_j <= 0 (none: all pairs, `truncated`), tau = -1 + 2 sum_{j < K} min(P_0 .. P_j), ess = C Mh / tau;
 6. W = 0 or a non-finite entry: rhat = ess = NaN for that coordinate alone."""
import numpy as np


def ar1(M, N, phis, seed, mean=0.0, sd=1.0):
    """Stationary AR(1) chains, one coefficient per coordinate: (M, N, d) float32."""
    phis = np.atleast_1d(np.asarray(phis, dtype=np.float64))
    d = phis.shape[0]
    rng = np.random.RandomState(seed)
    x = np.empty((M, N, d))
    x[0] = rng.randn(N, d)
    for t in range(1, M):
        x[t] = phis * x[t - 1] + np.sqrt(1 - phis ** 2) * rng.randn(N, d)
    return (np.asarray(mean, dtype=np.float64) + np.asarray(sd, dtype=np.float64) * x).astype(np.float32)


# name -> (M, N, phis, seed, mean, sd, max_lag)
FIXTURES = {
    "A": (1000, 64, [0.0, 0.5, 0.9, 0.97], 0, [0.0, 3.0, -20.0, 1.0], [1.0, 0.05, 2.0, 1.0], 255),
    "B": (257, 200, [0.3, 0.8], 1, [1.0, -1.0], 1.0, 127),                                   # odd M
    "C": (400, 1000, np.linspace(0, 0.95, 25), 2, np.linspace(-2, 2, 25), np.linspace(0.02, 1, 25), 99),
    "D": (64, 16, np.linspace(0, 0.6, 130), 3, 0.0, 1.0, 31),                                # d = 130 > 128
    "E": (50, 5, [0.5], 4, 10.0, 1.0, 9),                                                    # d = 1, tiny
    "F": (96, 77, np.linspace(0, 0.9, 17), 5, 0.0, 1.0, 47),                                 # N d = 1309, odd
}


def fixture(name):
    """(X float32, max_lag of the split analysis)"""
    M, N, phis, seed, mean, sd, max_lag = FIXTURES[name]
    return ar1(M, N, phis, seed, mean, sd), max_lag


def spread(d):
    """(phi, mean, sd) that differ in every coordinate -- phi 0 .. 0.9, mean -2 .. 2, sd 0.05 .. 2 -- so that a series read under
    another coordinate's mean, or added to another coordinate's sum, moves G[k, 0] by orders of magnitude, and a chunk of 256
    columns dropped or added twice moves it by one part in the number of chunks (>= 1 / 600 in the fixtures below)."""
    phi = np.array([0.0, 0.5, 0.9]) if d == 3 else np.linspace(0, 0.9, d)
    return phi, np.linspace(-2, 2, d), np.linspace(0.05, 2, d)


# The shapes that reach the branches of csrc/chain_stats.hip's plan which "A" .. "F" do not (they all get one column chunk per
# block, and d <= 130).  With J = N d columns in chunks of 256, `halves` 2 when split, ntile = max_lag // 32 + 1 lag tiles and
# period = d / gcd(256, d), the plan is nb = ceil(ceil(1024 / (ntile halves)) / period) period blocks along x, at most the number
# of chunks; block b walks the chunks b, b + nb, ...  tests/test_diagnostics_cpu.py reads nb back from the workspace size and
# holds every name to the branch stated here.
# name -> (M, N, d, seed, max_lag, split)
PLAN_FIXTURES = {
    # 514 chunks, period 3, nb = 513: block 0 alone walks a second chunk, the ragged last one (3 live columns)
    "two-chunks-d3": (64, 43777, 3, 10, 31, True),
    # odd M (the middle row is dropped), 2 lag tiles, 259 chunks, nb = 258: the tile that reloads x_t carried across chunks
    "two-tiles-d3": (130, 22017, 3, 11, 63, True),
    # period 15, 516 chunks, nb = 270, 2 lag tiles (the second holds lags 32 and 33), Mh = 35 odd: most blocks walk 2 chunks
    "period15-d60": (70, 2200, 60, 12, 33, True),
    # period 65, 559 chunks, nb = 520: several chunks with d < 256 not dividing 256, threads tid and tid + d added
    "period65-d130": (64, 1100, 130, 13, 31, True),
    # period 257, 516 chunks, nb = 514: a block holds 256 of 257 coordinates AND walks two chunks
    "period257-d257": (64, 513, 257, 23, 31, True),
    # the widest history the entry accepts: period 2, 600 chunks, nb = 512
    "period2-d512": (64, 300, 512, 33, 31, True),
    # unsplit, period 75, 528 chunks, nb = 1050 clamped to 528: d > 256 with one chunk per block
    "one-chunk-d300": (40, 450, 300, 16, 31, False),
    # 24 chunks of which a block holds 256 of 300 coordinates; small enough for every path
    "tiny-d300": (16, 20, 300, 17, 7, True),
}


def plan_fixture(name):
    """(X float32, max_lag, split)"""
    M, N, d, seed, max_lag, split = PLAN_FIXTURES[name]
    phi, mean, sd = spread(d)
    return ar1(M, N, phi, seed, mean, sd), max_lag, split


def split_chains(X, split=True):
    """(Mh, C, d) float64"""
    X = np.asarray(X, dtype=np.float64)
    if not split:
        return X
    M = X.shape[0]
    Mh = M // 2
    return np.concatenate([X[:Mh], X[M - Mh:]], axis=1)


def reference_sums(X, max_lag, split=True):
    """mean (C, d), M2 (C, d), G (d, max_lag + 1) in float64, chain by chain."""
    S = split_chains(X, split)
    Mh, C, d = S.shape
    mean, m2, G = np.empty((C, d)), np.empty((C, d)), np.zeros((d, max_lag + 1))
    for c in range(C):
        x = S[:, c, :]
        m = x.sum(axis=0) / Mh
        z = x - m
        mean[c], m2[c] = m, (z * z).sum(axis=0)
        for t in range(max_lag + 1):
            G[:, t] += (z[:Mh - t] * z[t:]).sum(axis=0)
    return mean, m2, G


def reference_sums_columns(X, max_lag, split=True):
    """`reference_sums` with every chain at once: the same definition -- centre per (chain, coordinate) in float64, then for each
    lag the products (z[:Mh - t] * z[t:]) summed over steps and chains -- for the histories of PLAN_FIXTURES, whose 87 554
    series the chain-by-chain loop cannot walk in a test's time.  tests/test_diagnostics_cpu.py holds it to `reference_sums`."""
    S = split_chains(X, split)
    Mh, C, d = S.shape
    mean = S.sum(axis=0) / Mh
    Z = S - mean
    m2 = np.einsum("tck,tck->ck", Z, Z)
    G = np.empty((d, max_lag + 1))
    for t in range(max_lag + 1):
        G[:, t] = np.einsum("tck,tck->k", Z[:Mh - t], Z[t:])
    return mean, m2, G


def reference_summary_columns(X, max_lag, split=True):
    """`reference_summary` on top of `reference_sums_columns`"""
    mean, m2, G = reference_sums_columns(X, max_lag, split)
    out = reference_finish(mean, m2, G, split_chains(X[:, :1], split).shape[0])
    out["sums"] = (mean, m2, G)
    return out


def reference_finish(mean, m2, G, Mh):
    """Steps 3, 5, 6, one coordinate at a time; also the pair sums up to and including the stopping pair (the fixtures'
    condition |P_j| >= 1e-4 is stated on them)."""
    C, d = mean.shape
    nlag = G.shape[1]
    out = {k: np.full(d, np.nan) for k in ("mean", "sd", "rhat", "ess", "tau")}
    out["truncated"] = np.zeros(d, dtype=bool)
    out["pairs"] = []
    for k in range(d):
        out["mean"][k] = mean[:, k].mean()
        W = m2[:, k].mean() / (Mh - 1)
        B = Mh * mean[:, k].var(ddof=1)
        varp = (Mh - 1) / Mh * W + B / Mh
        out["sd"][k] = np.sqrt(varp) if np.isfinite(varp) else np.nan
        if not (np.isfinite(W) and np.isfinite(varp) and np.all(np.isfinite(G[k])) and W > 0):
            out["pairs"].append(np.zeros(0))
            continue
        out["rhat"][k] = np.sqrt(varp / W)
        rho = [1.0 - (W - G[k, t] / (C * (Mh - 1))) / varp for t in range(nlag)]
        pairs, tau, run_min, stopped = [], -1.0, np.inf, False
        for j in range(nlag // 2):
            P = rho[2 * j] + rho[2 * j + 1]
            pairs.append(P)
            if P <= 0:
                stopped = True
                break
            run_min = min(run_min, P)
            tau += 2.0 * run_min
        out["truncated"][k] = not stopped
        out["tau"][k] = tau
        out["ess"][k] = C * Mh / tau
        out["pairs"].append(np.array(pairs))
    out["n_steps"], out["n_chains"] = Mh, C
    return out


def reference_summary(X, max_lag, split=True):
    mean, m2, G = reference_sums(X, max_lag, split)
    Mh = split_chains(X[:, :1], split).shape[0]
    out = reference_finish(mean, m2, G, Mh)
    out["sums"] = (mean, m2, G)
    return out
