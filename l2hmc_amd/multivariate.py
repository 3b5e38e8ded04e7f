"""What the coordinates of a recorded history (steps, chains, dim) have to do with each other, and what the run is worth as
a whole: the posterior covariance and correlation, and the multivariate effective sample size of Vats, Flegal & Jones
(Biometrika 2019), mESS = n (det Lambda / det Sigma)^(1/d) with Lambda the sample covariance and Sigma the batch-means
estimate of the asymptotic covariance -- one number that, unlike `min_ess`, no invertible linear map of the coordinates moves.

    c = covariance(x_hist[burn_in:])         # c.mean, c.cov, c.corr, c.sd, c.n_draws, c.degenerate
    m = multi_ess(x_hist[burn_in:])          # all of that, and m.multi_ess, m.cov_asymptotic, m.ess_batch, m.batch_size, m.n_batches

A ROCm tensor goes to the HIP kernels behind `l2hmc_moment_sums` (csrc/moment_sums.hip: float64 on the matrix pipe, one read of
the history for d <= 64) where it lies -- a first-axis slice of a history is contiguous -- and only 2 (d + d^2) numbers come
back; a numpy history is float64 numpy (`_history` has that rule and the host side of the launch).  The device holds dim <= 128; beyond it use numpy.

The estimator.  n = steps * chains draws; raw sums s = sum x, C = sum x x^T.  mu = s / n, P = C - n mu mu^T, Lambda = P / (n - 1).
A batch is `batch_size` consecutive steps of one chain (default floor(sqrt(steps))): a = steps // batch_size per chain over
rows [steps - a batch_size, steps), A = a * chains in all, with batch means ybar; sbar = sum ybar, Cb = sum ybar ybar^T,
Q = Cb - mu sbar^T - sbar mu^T + A mu mu^T = sum (ybar - mu)(ybar - mu)^T, Sigma = batch_size Q / (A - 1);
multi_ess = n exp((logdet Lambda - logdet Sigma) / d), ess_batch[k] = n Lambda_kk / Sigma_kk.  Sigma is singular unless A > d.
A coordinate is `degenerate` when it holds a non-finite entry or Lambda_kk <= n 2^-53 C_kk / n -- the resolution of the
raw-moment form, what a chain of n float64 additions can lose of the raw moment (4.5e-11 at 4e5 draws): a constant.  The
threshold grows with n: a coordinate whose variance is that small a part of its raw moment cannot be told from a constant.
Rank-normalised quantities are not computed, and Lambda is not used as a metric by the sampler.

The numpy path carries its raw sums in the host's long double and `finish` takes every raw moment apart in it.  Where long
double is wider than float64 (x86: 64 bits of mantissa) the numpy path agrees with a two-pass evaluation to 1e-12 of
sqrt(P_ii P_jj); where it is float64 the path still works and loses what a float64 raw moment loses, 2^-53 C_kk / P_kk.
"""
import numpy as np

from . import _ffi, diagnostics as dg
from ._history import as_numpy, history_shape, in_place, is_device_tensor, launch, workspace

MAX_DEVICE_DIM = 128          # l2hmc_moment_sums: d <= 128
MAX_FLAT_CHAINS = 4096        # (draws, d) is read as (draws / c, c, d), c <= this: one wave per SIMD on 256 CUs
ULP = 2.0 ** -53              # the resolution of the raw-moment form is n_draws ULP, relative to C_kk / n


def _layout(X, batch_size):
    """(steps, chains, d) of a history (steps, chains, d) or, without batches, (draws, d); ValueError otherwise.
    Without batches any factorisation of the draws gives the same sums, and the kernels fill their lanes with adjacent
    "chains": (draws, d) is read as (draws / c, c, d) with c the largest divisor of draws up to 4096 (a prime number of
    draws stays one chain, a sixteenth of the lanes live)."""
    batch_size = int(batch_size)
    shape = history_shape(X, flat_ok=batch_size == 0,
                          says=None if batch_size == 0 else "a history is (steps, chains, dim) when batches are asked for")
    if len(shape) == 2:
        c = max([k for k in range(1, min(shape[0], MAX_FLAT_CHAINS) + 1) if shape[0] % k == 0] or [1])
        shape = (shape[0] // c, c, shape[1])
    M, N, d = shape
    if M < 1 or N < 1 or d < 1:
        raise ValueError("a history needs at least one draw and dim >= 1; got shape %s" % (tuple(X.shape),))
    if not 0 <= batch_size <= M:
        raise ValueError("batch_size must be in 0 .. steps = %d (got %d)" % (M, batch_size))
    return M, N, d


def _device_sums(X, M, N, d, batch):
    import torch
    X = in_place(X)
    L, dev = _ffi.lib(), X.device
    ws = workspace(dev, torch.float64, L.l2hmc_moment_sums_workspace_doubles, M, N, d, batch)
    out = [torch.empty(d, dtype=torch.float64, device=dev), torch.empty((d, d), dtype=torch.float64, device=dev)]
    if batch:
        out += [torch.empty(d, dtype=torch.float64, device=dev), torch.empty((d, d), dtype=torch.float64, device=dev)]
    launch(dev, L.l2hmc_moment_sums, X.data_ptr(), M, N, d, batch, out[0].data_ptr(), out[1].data_ptr(),
           out[2].data_ptr() if batch else None, out[3].data_ptr() if batch else None, ws.data_ptr())
    return out + [None] * (4 - len(out))


def _host_sums(X, M, N, d, batch):
    """The raw sums of a numpy history as long double arrays.  The float64 work (BLAS) is done on values shifted by a pivot
    c near the mean, where nothing cancels; the raw form sum x x^T = Z^T Z + c sz^T + sz c^T + n c c^T is then put together in
    the host's long double, so that `finish` can take it apart again without the 1e-11 a float64 raw moment would cost."""
    X = np.asarray(X)
    if X.dtype != np.float64:
        X = X.astype(np.float64)
    X = X.reshape(M, N, d)
    ld = np.longdouble

    def raw(Y):
        n = Y.shape[0]
        c = Y[0] + (Y - Y[0]).sum(axis=0) / n
        c = np.where(np.isfinite(c), c, 0.0)                # a non-finite coordinate is not shifted: it stays non-finite
        Z = Y - c
        sz, Pz, c = Z.sum(axis=0).astype(ld), (Z.T @ Z).astype(ld), c.astype(ld)
        return sz + n * c, Pz + np.outer(c, sz) + np.outer(sz, c) + n * np.outer(c, c)

    with np.errstate(all="ignore"):                         # a non-finite entry: its own rows and columns, quietly
        out = list(raw(X.reshape(-1, d))) + [None, None]
        if batch:
            a = M // batch
            out[2:] = raw(X[M - a * batch:].reshape(a, batch, N, d).sum(axis=1).reshape(-1, d) / float(batch))
    return out


def moment_sums(X, batch_size=0):
    """The raw sums of a (steps, chains, d) history -- or, with `batch_size` 0, of (draws, d):
    {'n_draws', 'sum' (d), 'cross' (d, d), 'batch_size', 'n_batches', 'batch_sum' (d), 'batch_cross' (d, d)}; the batch
    entries are None without batches.  A ROCm tensor -> the HIP kernels, float64 device tensors (bitwise reproducible);
    numpy -> float64 numpy arithmetic, the sums as long double arrays (`_host_sums`).  Sums of ranks that hold different
    chains simply add."""
    M, N, d = _layout(X, batch_size)
    batch = int(batch_size)
    if is_device_tensor(X):
        if d > MAX_DEVICE_DIM:
            raise ValueError("the moment kernels hold dim <= %d (got %d): pass the history as a numpy array" % (MAX_DEVICE_DIM, d))
        s, c, bs, bc = _device_sums(X, M, N, d, batch)
    else:
        s, c, bs, bc = _host_sums(as_numpy(X), M, N, d, batch)
    return {"n_draws": M * N, "sum": s, "cross": c, "batch_size": batch, "n_batches": (M // batch) * N if batch else 0,
            "batch_sum": bs, "batch_cross": bc}


def _wide(a):
    """A sum as a long double numpy array (device float64 tensors and float64 arrays widen exactly)."""
    return as_numpy(a, np.longdouble)


def finish(sums):
    """`covariance` -- and, when the sums hold batches, `multi_ess` -- from `moment_sums`' result (or the all-reduced sums of
    `sharding.multivariate`): host arithmetic on 2 (d + d^2) numbers -- the raw moments are taken apart (P, Q) in the host's
    long double, which costs device sums nothing and keeps what the numpy path's sums carry; everything after is float64."""
    n, A, b = int(sums["n_draws"]), int(sums["n_batches"]), int(sums["batch_size"])
    s, C = _wide(sums["sum"]), _wide(sums["cross"])
    d = s.shape[0]
    with np.errstate(all="ignore"):
        mu_w = s / n
        mu = mu_w.astype(np.float64)
        P = (C - n * np.outer(mu_w, mu_w)).astype(np.float64)
        cov = P / (n - 1) if n > 1 else np.full((d, d), np.nan)
        raw = np.diag(C).astype(np.float64)
        s = s.astype(np.float64)
        var = np.diag(cov)
        finite = np.isfinite(s) & np.isfinite(raw)
        degenerate = ~finite | ~(var > (n * ULP) * raw / n)
        cov[~finite, :] = np.nan
        cov[:, ~finite] = np.nan
        sd = np.sqrt(np.where(var > 0, var, np.where(finite, 0.0, np.nan)))
        corr = cov / np.outer(sd, sd)
        corr[degenerate, :] = np.nan
        corr[:, degenerate] = np.nan
        corr[~degenerate, ~degenerate] = 1.0
    out = dg.Summary(mean=mu, cov=cov, corr=corr, sd=sd, n_draws=n, degenerate=degenerate)
    if not A:
        return out
    if A <= d:
        raise ValueError("multi_ess needs more batches than coordinates (n_batches = %d, dim = %d): the batch-means estimate "
                         "of the asymptotic covariance would be singular -- use a smaller batch_size or more chains" % (A, d))
    sb, Cb = _wide(sums["batch_sum"]), _wide(sums["batch_cross"])
    with np.errstate(all="ignore"):
        # the two mean terms are added to each other first: a + b is b + a bit for bit, (c - a) - b is not (c - b) - a, and
        # Sigma is promised as symmetric as `batch_cross` is
        Q = (Cb - (np.outer(mu_w, sb) + np.outer(sb, mu_w)) + A * np.outer(mu_w, mu_w)).astype(np.float64)
        Sigma = b * Q / (A - 1)
        Sigma[~finite, :] = np.nan
        Sigma[:, ~finite] = np.nan
        ess_batch = n * np.diag(cov) / np.diag(Sigma)
        ess_batch[degenerate] = np.nan
        if degenerate.any():
            mess = float("nan")
        else:
            (sl, ll), (ss, ls) = np.linalg.slogdet(cov), np.linalg.slogdet(Sigma)
            mess = float(n * np.exp((ll - ls) / d)) if sl > 0 and ss > 0 else float("nan")
    out.update(multi_ess=mess, cov_asymptotic=Sigma, ess_batch=ess_batch, batch_size=b, n_batches=A)
    return out


def default_batch_size(steps):
    return max(1, int(np.floor(np.sqrt(int(steps)))))


def covariance(X):
    """`mean`, `cov` (the sample covariance Lambda, ddof 1), `corr`, `sd`, `n_draws` and `degenerate` (d bools) of a history
    (steps, chains, dim) or (draws, dim), as a `diagnostics.Summary`.  The `cov` and `corr` rows and columns of a coordinate
    with a non-finite entry are NaN, alone; a constant coordinate is `degenerate` too, its `cov` stays finite and its
    `corr` is NaN.  Constant means Lambda_kk <= n_draws 2^-53 (C_kk / n_draws), C_kk = sum x_k^2: the threshold is what
    n_draws float64 additions can lose of the raw moment, so it grows with the number of draws (4.5e-11 of the raw moment at
    4e5 draws, 4.5e-7 at 4e9)."""
    return finish(moment_sums(X, 0))


def _batch_size(X, batch_size):
    M = history_shape(X, says="multi_ess needs a history (steps, chains, dim)")[0]
    if batch_size is None:
        return default_batch_size(M)
    if int(batch_size) != batch_size or not 1 <= int(batch_size) <= M:
        raise ValueError("batch_size must be an integer in 1 .. steps = %d (got %r)" % (M, batch_size))
    return int(batch_size)


def multi_ess(X, batch_size=None):
    """Everything `covariance` returns, and `multi_ess` (Vats, Flegal & Jones 2019), `cov_asymptotic` (the batch-means Sigma),
    `ess_batch` (d: n Lambda_kk / Sigma_kk), `batch_size` (default floor(sqrt(steps))) and `n_batches`, of a
    (steps, chains, dim) history.  ValueError unless n_batches > dim.  Any degenerate coordinate makes `multi_ess` NaN;
    `degenerate` says which."""
    return finish(moment_sums(X, _batch_size(X, batch_size)))
