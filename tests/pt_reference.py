"""numpy restatement of the parallel-tempering swap sweep of `l2hmc_trajectory_ladder` (include/l2hmc.h): the deterministic
even-odd sweep, the Metropolis swap rule, the swap counters, the round-trip counting and the Philox stream of the swap uniforms.
Float64 throughout; the GPU tests replay it on the kernel's own states (`replay`) and leave out the ladders with a decision inside
a near-tie margin of the threshold (1e-5, or a margin per ladder and pair)."""
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
    near (n_ladders, K - 1) bool: decisions within `tol` of the threshold).  `tol`: a scalar, or an array that broadcasts to
    (n_ladders, K - 1) -- one margin per ladder and pair."""
    labels = np.array(labels, dtype=np.int64)
    nl, K = labels.shape
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (nl, K - 1))
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
            near[:, k] = np.abs(lhs - rhs) <= tol[:, k]
        att[k] += nl
        acc[k] += int(ok.sum())
        new[idx[ok], a[ok]] = k + 1
        new[idx[ok], b[ok]] = k
    return new, acc, att, near


def replay(pt, o, x_hist, U_of, temps, R, M, u_inj, seed, labels0, tol=1e-5):
    """Replay the sweeps of a `ParallelTempering.run` on the kernel's own states: `pt` the ladder, `o` its output (with
    rung_hist), x_hist (R M, N, d) the recorded states, U_of(states) their untempered energies as float64 (N,), u_inj the
    injected swap uniforms (R, n_ladders, K // 2) or None for the Philox stream of `seed`, labels0 (n_ladders, K) the labels in
    front of round 0.  A ladder with a decision inside the near-tie margin is left out of that round's comparison; `tol` is
    that margin as `sweep` takes it, or a callable (labels, U) -> margin.  Every other ladder's labels must equal the
    kernel's.  Returns (ladders compared, accepted (K - 1), attempted (K - 1), round trips per ladder)."""
    K, nl = pt.K, pt.n_ladders
    rh = o["rung_hist"].detach().cpu().numpy().astype(np.int64)
    prev, trip = np.array(labels0, dtype=np.int64), np.zeros((nl, K), np.int64)
    acc, att, trips, compared = np.zeros(K - 1, np.int64), np.zeros(K - 1, np.int64), np.zeros(nl, np.int64), 0
    for j in range(R):
        U = U_of(x_hist[j * M + M - 1]).reshape(nl, K)
        uj = u_inj[j] if u_inj is not None else swap_uniforms(seed, nl, K, j)
        new, a, t, near = sweep(prev, U, temps, j, uj, tol=tol(prev, U) if callable(tol) else tol)
        got = rh[j].reshape(nl, K)
        ok = ~near.any(axis=1)
        assert np.array_equal(new[ok], got[ok]), (j, np.nonzero(~np.all(new == got, axis=1) & ok))
        compared += int(ok.sum())
        acc += a
        att += t
        prev = got
        trip, done = update_trips(got, trip, K)
        trips += done
    return compared, acc, att, trips


def update_trips(labels, trip, K):
    """Round trips after a sweep: a row that has reached rung K - 1 since it last left rung 0 completes one when it is back at
    rung 0.  labels, trip (n_ladders, K); returns (new trip states, completed trips per ladder)."""
    trip = np.array(trip, dtype=np.int64)
    top, bottom = labels == K - 1, labels == 0
    done = (bottom & (trip == 1)).sum(axis=1)
    trip = np.where(top, 1, np.where(bottom, 0, trip))
    return trip, done
