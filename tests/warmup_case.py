"""The warm-up's float64 restatement and its two fixtures (no GPU, no library): `DualAveraging` follows the update rules of
include/l2hmc.h (`l2hmc_adapt_update`) line by line, `hmc_step` is a plain numpy HMC proposal, `fixture` builds

  L  Bayesian logistic regression: n = 500, d = 25, X and the true w standard normal from a fixed seed, prior variance 1;
  G  a diagonal Gaussian: d = 50, standard deviations logspace(-1, 0, 50);

both at 256 chains with T = 10 leapfrog steps, chains started at 0.1 N(0, I)."""
import math

import numpy as np

LN2, LN10 = math.log(2.0), math.log(10.0)
N_CHAINS, T = 256, 10
TARGET, N_UPDATES, N_CHECK = 0.8, 100, 100
EPS0 = {"L": (1e-4, 2.0), "G": (1e-3, 4.0)}
CAP_ACCEPT, CAP_RATIO = 0.03, 1.05            # |accept - target| and eps(start a) / eps(start b), set by the issue


class DualAveraging(object):
    """state[0 .. 15] as include/l2hmc.h lays it out; `update(a)` returns the trace row."""

    def __init__(self, log_eps, search=True, target=0.8, gamma=0.05, t0=10.0, kappa=0.75, log_eps_min=math.log(1e-8),
                 log_eps_max=math.log(1e3)):
        self.phase, self.dir, self.t = (0 if search else 1), 0, 0
        self.log_eps = float(log_eps)
        self.log_eps_bar = self.H_bar = 0.0
        self.mu = 0.0 if search else self.log_eps + LN10
        self.accept, self.count = 0.0, 0
        self.target, self.gamma, self.t0, self.kappa = float(target), float(gamma), float(t0), float(kappa)
        self.lo, self.hi = float(log_eps_min), float(log_eps_max)

    def _clamp(self, v):
        return min(max(v, self.lo), self.hi)

    def _start_averaging(self):
        self.phase, self.mu, self.t, self.H_bar, self.log_eps_bar = 1, self.log_eps + LN10, 0, 0.0, 0.0

    def update(self, a):
        a = float(a)
        ran = self.log_eps
        if self.phase == 0:
            d = 1 if a > 0.5 else -1
            if self.dir == 0:
                self.dir = d
            if d == self.dir:
                stepped = self.log_eps + self.dir * LN2
                self.log_eps = self._clamp(stepped)
                if self.log_eps != stepped:
                    self._start_averaging()
            else:
                self._start_averaging()
        elif self.phase == 1:
            self.t += 1
            t = float(self.t)
            w = 1.0 / (t + self.t0)
            self.H_bar = (1.0 - w) * self.H_bar + w * (self.target - a)
            self.log_eps = self._clamp(self.mu - math.sqrt(t) / self.gamma * self.H_bar)
            e = t ** (-self.kappa)
            self.log_eps_bar = e * self.log_eps + (1.0 - e) * self.log_eps_bar
        self.accept = a
        self.count += 1
        return np.array([a, ran, self.log_eps, float(self.phase)])

    def finish(self):
        if self.t >= 1:
            self.log_eps = self.log_eps_bar
        self.phase = 2

    @property
    def alpha(self):
        return np.float32(self.log_eps)

    def state(self):
        return np.array([self.phase, self.dir, self.t, self.log_eps, self.log_eps_bar, self.H_bar, self.mu, self.accept,
                         self.count, self.target, self.gamma, self.t0, self.kappa, self.lo, self.hi, 0.0], dtype=np.float64)


def window_mean(p):
    """a of a window of float32 accept probabilities: non-finite entries count as 0, the sum is float64"""
    p = np.asarray(p, dtype=np.float32).ravel()
    return float(np.where(np.isfinite(p), p, np.float32(0)).astype(np.float64).sum() / p.size)


def hmc_step(x, eps, U, grad_U, rng, n_steps=T):
    """One HMC proposal + Metropolis step on every row of x: (x_next, p)."""
    v = rng.standard_normal(x.shape)
    h0 = U(x) + 0.5 * np.sum(v * v, axis=1)
    q = x.copy()
    v = v - 0.5 * eps * grad_U(q)
    for s in range(n_steps):
        q = q + eps * v
        v = v - (eps if s < n_steps - 1 else 0.5 * eps) * grad_U(q)
    with np.errstate(all="ignore"):
        h1 = U(q) + 0.5 * np.sum(v * v, axis=1)
        p = np.exp(np.minimum(h0 - h1, 0.0))
    p = np.where(np.isfinite(p), p, 0.0)
    take = rng.uniform(size=p.shape) < p
    return np.where(take[:, None], q, x), p


_FIXTURES = {}


def fixture(name):
    """{'d', 'x0' (256, d) float32, 'U', 'grad_U' (float64 numpy callables), and what builds the library's energy:
    'X', 'y' (L) or 'sd' (G)}; built once."""
    if name not in _FIXTURES:
        if name == "L":
            rng = np.random.RandomState(1234)
            n, d = 500, 25
            X = rng.standard_normal((n, d)).astype(np.float32)
            w = rng.standard_normal(d)
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ w))).astype(np.float32)
            X64, y64 = X.astype(np.float64), y.astype(np.float64)

            def U(q):
                Lg = q @ X64.T
                return (np.logaddexp(0.0, Lg) - Lg * y64).sum(axis=1) + 0.5 * np.sum(q * q, axis=1)

            def grad_U(q):
                with np.errstate(all="ignore"):
                    return (1.0 / (1.0 + np.exp(-(q @ X64.T))) - y64) @ X64 + q
            f = {"d": d, "X": X, "y": y, "U": U, "grad_U": grad_U}
        elif name == "G":
            d = 50
            sd = np.logspace(-1.0, 0.0, d)
            prec = (1.0 / (sd * sd).astype(np.float32)).astype(np.float64)        # the float32 precision the kernels hold
            f = {"d": d, "sd": sd, "U": lambda q: 0.5 * np.sum(q * q * prec, axis=1), "grad_U": lambda q: q * prec}
        else:
            raise KeyError(name)
        f["x0"] = (0.1 * np.random.RandomState(99).standard_normal((N_CHAINS, f["d"]))).astype(np.float32)
        _FIXTURES[name] = f
    return _FIXTURES[name]


def restated_warmup(name, eps0, target=TARGET, n_updates=N_UPDATES, n_check=N_CHECK, seed=0):
    """The whole warm-up in numpy: n_updates windows of one proposal, finish, then n_check proposals at the finished step size.
    Returns (eps, mean accept of the check proposals, trace (n_updates, 4))."""
    f = fixture(name)
    rng = np.random.RandomState(seed)
    x = f["x0"].astype(np.float64)
    da = DualAveraging(float(np.float32(math.log(eps0))), target=target)
    trace = np.empty((n_updates, 4))
    for k in range(n_updates):
        x, p = hmc_step(x, math.exp(float(da.alpha)), f["U"], f["grad_U"], rng)
        trace[k] = da.update(window_mean(p))
    da.finish()
    eps = math.exp(float(da.alpha))
    acc = []
    for _ in range(n_check):
        x, p = hmc_step(x, eps, f["U"], f["grad_U"], rng)
        acc.append(p.mean())
    return eps, float(np.mean(acc)), trace
