"""numpy restatement of the parallel-tempering swap sweep of `l2hmc_trajectory_ladder` (include/l2hmc.h): the deterministic
even-odd sweep, the Metropolis swap rule, the swap counters, the round-trip counting and the Philox stream of the swap uniforms.
Float64 throughout; the GPU tests skip the pairs whose decision lies within 1e-5 of the threshold."""
import numpy as np

from oracle.l2hmc_oracle import philox4x32_10


def swap_uniforms(seed, n_ladders, K, rnd, ladder0=0):
    """(n_ladders, K // 2) uniforms of round `rnd`, pair (k, k + 1) at index k // 2: Philox stream 2 of
    csrc/l2hmc_kernels.hpp, counter (global ladder, 0xFFFFFFFF, rnd mod 2^32, (rnd >> 32) << 4 | (k >> 1) << 1 | 1)."""
    P = K // 2
    c = np.zeros((n_ladders, P, 4), dtype=np.uint64)
    c[..., 0] = (ladder0 + np.arange(n_ladders, dtype=np.uint64))[:, None]
    c[..., 1] = 0xFFFFFFFF
    c[..., 2] = rnd & 0xFFFFFFFF
    c[..., 3] = (((rnd >> 32) << 4) | (np.arange(P, dtype=np.uint64) << 1) | 1)[None, :]
    r = philox4x32_10(c, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (r[..., 0] >> 8).astype(np.float64) * 2.0 ** -24


def sweep(labels, U, temps, rnd, u, tol=0.0):
    """One sweep of round `rnd`.  labels (n_ladders, K) rung of each row (row-ordered within its ladder), U (n_ladders, K)
    untempered energies by row, u (n_ladders, K // 2).  Returns (new labels, accepted (K - 1), attempted (K - 1),
    near (n_ladders, K - 1) bool: decisions within `tol` of the threshold)."""
    labels = np.array(labels, dtype=np.int64)
    nl, K = labels.shape
    U = np.asarray(U, dtype=np.float64)
    beta = 1.0 / np.asarray(temps, dtype=np.float64)
    acc, att = np.zeros(K - 1, np.int64), np.zeros(K - 1, np.int64)
    near = np.zeros((nl, K - 1), dtype=bool)
    inv = np.argsort(labels, axis=1)                           # row of rung k, per ladder
    new = labels.copy()
    idx = np.arange(nl)
    for k in range(rnd & 1, K - 1, 2):
        a, b = inv[:, k], inv[:, k + 1]
        with np.errstate(divide='ignore', invalid='ignore'):
            lhs = np.log(np.asarray(u, dtype=np.float64)[:, k // 2])
            rhs = (beta[k] - beta[k + 1]) * (U[idx, a] - U[idx, b])
            ok = lhs < rhs                                     # (NaN compares False: rejected)
            near[:, k] = np.abs(lhs - rhs) <= tol
        att[k] += nl
        acc[k] += int(ok.sum())
        new[idx[ok], a[ok]] = k + 1
        new[idx[ok], b[ok]] = k
    return new, acc, att, near


def update_trips(labels, trip, K):
    """Round trips after a sweep: a row that has reached rung K - 1 since it last left rung 0 completes one when it is back at
    rung 0.  labels, trip (n_ladders, K); returns (new trip states, completed trips per ladder)."""
    trip = np.array(trip, dtype=np.int64)
    top, bottom = labels == K - 1, labels == 0
    done = (bottom & (trip == 1)).sum(axis=1)
    trip = np.where(top, 1, np.where(bottom, 0, trip))
    return trip, done
