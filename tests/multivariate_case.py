"""Shared by tests/test_multivariate_cpu.py and tests/test_gpu_multivariate.py: a float64 restatement of
`l2hmc_amd.multivariate` written from the definitions, independently of the module (whose numpy path and HIP kernels are both
held against it), and the gates of the raw sums.  The AR(1) fixtures are those of tests/diagnostics_case.py, plus "G".

The restatement is TWO-pass: centre in float64, then Z^T Z (the module and the kernels are one-pass, on raw moments).
 - n = steps * chains draws x; mu = mean x; P = sum (x - mu)(x - mu)^T; Lambda = P / (n - 1);
 - a batch is b consecutive steps of one chain, a = steps // b per chain over rows [steps - a b, steps), A = a * chains in all,
   with means ybar; Q = sum (ybar - mu)(ybar - mu)^T (mu of ALL draws); Sigma = b Q / (A - 1);
 - multi_ess = n exp((logdet Lambda - logdet Sigma) / d) (Vats, Flegal & Jones 2019); ess_batch[k] = n Lambda_kk / Sigma_kk.
The raw form of the same numbers (what `moment_sums` returns): sum = n mu, cross = P + n mu mu^T, and with m the mean of the
batch means and Qc their centred cross product, batch_sum = A m, batch_cross = Qc + A m m^T."""
import numpy as np

from tests import diagnostics_case as dc

GATE = 1e-10          # of sqrt(raw_ii raw_jj): 2^-53 x the longest chain of additions (<= the 4e5 rows of "C") = 4.4e-11
G_FIXTURE = (64, 32, np.linspace(0, 0.6, 100), 6, np.linspace(-3, 3, 100), 1.0)
ROTATION_HISTORY = (1024, 64, [0.0, 0.3, 0.5, 0.6], 7, [0.0, 5.0, -3.0, 1.0], [1.0, 0.1, 2.0, 1.0])
_CACHE = {}


def history(name):
    """float32 (steps, chains, d): the fixtures of diagnostics_case, "G" (d = 100) and "R" (the rotation history)."""
    if name not in _CACHE:
        X = dc.ar1(*G_FIXTURE) if name == "G" else dc.ar1(*ROTATION_HISTORY) if name == "R" else dc.fixture(name)[0]
        X.setflags(write=False)
        _CACHE[name] = X
    return _CACHE[name]


def default_batch(steps):
    return int(np.floor(np.sqrt(steps)))


def reference(X, batch):
    """Everything, two-pass in float64; `batch` 0: the covariance part alone."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[:, None, :]
    M, N, d = X.shape
    n = M * N
    X2 = X.reshape(n, d)
    with np.errstate(all="ignore"):
        mu = X2.sum(axis=0) / n
        Z = X2 - mu
        P = Z.T @ Z
        out = {"n_draws": n, "mean": mu, "P": P, "cov": P / (n - 1), "sum": n * mu, "cross": P + n * np.outer(mu, mu)}
        sd = np.sqrt(np.diag(out["cov"]))
        out["sd"], out["corr"] = sd, out["cov"] / np.outer(sd, sd)
        if not batch:
            return out
        a = M // batch
        A = a * N
        Y = X[M - a * batch:].reshape(a, batch, N, d).sum(axis=1).reshape(A, d) / batch
        m = Y.sum(axis=0) / A
        Yc = Y - m
        Qc = Yc.T @ Yc
        Ym = Y - mu
        Q = Ym.T @ Ym
        Sigma = batch * Q / (A - 1)
        out.update(n_batches=A, batch_size=batch, Q=Q, cov_asymptotic=Sigma, batch_sum=A * m,
                   batch_cross=Qc + A * np.outer(m, m), ess_batch=n * np.diag(out["cov"]) / np.diag(Sigma))
        if A > d:
            out["multi_ess"] = n * np.exp((np.linalg.slogdet(out["cov"])[1] - np.linalg.slogdet(Sigma)[1]) / d)
    return out


def sum_gates(cross_diag, count):
    """(gate of the vector sum, gate of the cross matrix) from the diagonal of the raw cross matrix and the number of terms.
    The matrix: GATE sqrt(raw_ii raw_jj).  The vector sum is the cross moment of the coordinate with the constant 1, whose
    raw diagonal is the count: GATE sqrt(raw_ii count) -- the same rule, and the one reading of it that has the units of a
    sum (by Cauchy-Schwarz |sum_i| <= sqrt(raw_ii count), as |cross_ij| <= sqrt(raw_ii raw_jj))."""
    raw = np.asarray(cross_diag, dtype=np.float64)
    return GATE * np.sqrt(raw * count), GATE * np.sqrt(np.outer(raw, raw))


def theory_tau_batch(phi, b):
    """n Var(batch mean of b steps) / Var(x) ... per step: tau_b = (1 + phi) / (1 - phi) - 2 phi (1 - phi^b) / (b (1 - phi)^2)."""
    phi = np.asarray(phi, dtype=np.float64)
    return (1 + phi) / (1 - phi) - 2 * phi * (1 - phi ** b) / (b * (1 - phi) ** 2)


def rotation():
    """A fixed 4 x 4 orthogonal matrix: coordinates 0 and 3 (phi = 0 and 0.6) turned by 45 degrees, 1 and 2 by 30."""
    R = np.eye(4)
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    R[0, 0], R[0, 3], R[3, 0], R[3, 3] = c, -s, s, c
    G = np.eye(4)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    G[1, 1], G[1, 2], G[2, 1], G[2, 2] = c, -s, s, c
    return G @ R
