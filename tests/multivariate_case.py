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
# The shapes that reach the branches of csrc/moment_sums.hip's plan which the fixtures above do not (they have at most 1000
# chains and T = ceil(d / 16) = 1, 2 or 7 tiles).  A block is 4 waves x 4 chains: nchunks = ceil(chains / 16) chunks over
# nbx = min(nchunks, 256) blocks (block b walks chunk b, b + 256, ...), the steps cut into nseg = min(ceil(256 / nbx), steps //
# batch) segments after the rem = steps % batch leading rows that belong to no batch.  d <= 64: one panel of T tiles; above, a
# panel of tiles [0, 4), one of the T - 4 others and an off-diagonal one.  Every coordinate has its own phi, mean and sd
# (diagnostics_case.spread).  tests/test_multivariate_cpu.py reads nbx nseg back from the workspace size.
# name -> (steps, chains, d, batch, seed)
PLAN_FIXTURES = {
    # 258 chunks > 256, nseg = 1, rem = 1: blocks 0 and 1 walk a second chunk and start it with the leading remainder again;
    # chunk 257 has one live chain, in wave 0
    "two-chunks-d17": (21, 4113, 17, 4, 20),
    # 257 chunks across the three panels of T = 5 (the off-diagonal one is <4, 1>), rem = 0
    "two-chunks-d70": (12, 4100, 70, 3, 21),
    # 33 chains = 2 chunks and one chain, nseg = 6, rem = 4; A = 198 batches > d
    "panel-d40": (40, 33, 40, 6, 22),        # T = 3, one panel
    "panel-d64": (40, 33, 64, 6, 23),        # T = 4, one panel, every column live
    "panel-d65": (40, 33, 65, 6, 24),        # T = 5: second diagonal panel of 1 tile with one live column, off-diagonal <4, 1>
    "panel-d96": (40, 33, 96, 6, 25),        # T = 6: second diagonal panel of 2 tiles, off-diagonal <4, 2>
    "panel-d113": (40, 33, 113, 6, 26),      # T = 8, the last tile with one live column, off-diagonal <4, 4>
    "panel-d128": (40, 33, 128, 6, 27),      # T = 8, the widest history the entry accepts
}
_CACHE = {}


def history(name):
    """float32 (steps, chains, d): the fixtures of diagnostics_case, "G" (d = 100), "R" (the rotation history) and
    PLAN_FIXTURES."""
    if name not in _CACHE:
        if name in PLAN_FIXTURES:
            steps, chains, d, _, seed = PLAN_FIXTURES[name]
            phi, mean, sd = dc.spread(d)
            X = dc.ar1(steps, chains, phi, seed, mean, sd)
        else:
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
