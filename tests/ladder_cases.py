"""The launches tests/test_gpu_ladder_geometries.py holds the ladder kernel to, one per compiled geometry, energy kind, hidden
k-step count and rung count of `traj_ladder_kernel<EK, DT, NW, KH>` (l2hmc_amd/csrc/traj_body.inc under `if constexpr (LAD)`).

One place says what a case launches, so that the CPU check of its inputs (tests/test_tempering_cpu.py) and the GPU tests cannot
drift apart.  Every case is the smallest shape at which the ladder additions can go wrong: 40 rows of a K = 4 ladder are two full
16-chain tiles and one half-live tile holding two ladders; R = 4 rounds of M = 2 proposals run both sweep parities twice and
put one proposal of every round behind a sweep and one in front of it; distinct temperatures send every accepted swap through
the re-evaluation of grad U, U and the VNet layer-1 partial at the new rung.

Step sizes: the float32 oracle's mean accept probability of the first proposal (oracle.l2hmc_oracle.propose on the case's own
inputs) lies in 0.3 ... 0.85 at every rung for the Gaussian, mixture and Rough-Well cases and in 0.2 ... 0.9 for the funnel and
the logistic cases; the figures of the latter stand beside their rows.  (The HMC twin g20_hmc keeps the step size of its
net-driven sibling and accepts nearly every proposal there, p = 0.998 ... 1.0: plain leapfrog at eps = 0.05 conserves H.
`roughwell_ne` at d = 20 accepts nothing at eps = 0.05 or 0.1 and is not used.)
"""
import numpy as np

from l2hmc_amd.tempering import geometric_ladder
from oracle import l2hmc_oracle as O

from . import helpers

N, T, R, M = 40, 5, 4, 2
TEMPS = [1.0, 1.5, 2.5, 4.0]
SEED = 3                    # synthetic_case seed (nets, mask, energy parameters, x)
DRAWS_SEED = 20241019       # the injected proposal draws and swap uniforms
PRIOR_VAR = 2.0
BASE_TOL = 1e-5             # the suite's near-tie margin of a swap decision (tests/test_gpu_tempering.py)
ULPS = 4.0

L = "traj_ladder_kernel"

# name -> what the case launches.  target: a `helpers.synthetic_case` kind, "funnel" or "logistic"; kernel: what
# `_ffi.last_kernel()` must report after the ladder launch (the planner: pick_geometry / pick_geometry_logistic, l2hmc_abi.hip)
CASES = {
    "g16": dict(target="gauss_diag", d=16, variant=100, eps=0.05, kernel=L + "<1, 1, 1, 3>"),
    "g20_w1": dict(target="gauss_diag", d=20, variant=101, eps=0.05, kernel=L + "<1, 2, 1, 3>"),
    "g20_w4": dict(target="gauss_diag", d=20, variant=100, eps=0.05, kernel=L + "<1, 1, 4, 3>"),
    "g50_w1": dict(target="gauss_diag", d=50, variant=101, eps=0.05, kernel=L + "<1, 4, 1, 3>"),
    "g50_w4": dict(target="gauss_diag", d=50, variant=100, eps=0.05, kernel=L + "<1, 1, 4, 3>"),
    "g80": dict(target="gauss_diag", d=80, variant=100, eps=0.03, kernel=L + "<1, 2, 4, 3>"),
    "g200": dict(target="gauss_diag", d=200, variant=100, eps=0.02, kernel=L + "<1, 4, 4, 3>"),
    "g300": dict(target="gauss_diag", d=300, variant=100, eps=0.01, kernel=L + "<1, 8, 4, 3>"),
    "g20_h14": dict(target="gauss_diag", d=20, H=14, variant=100, eps=0.05, kernel=L + "<1, 1, 4, 4>"),
    "g20_hmc": dict(target="gauss_diag", d=20, hmc=True, variant=100, eps=0.05, kernel=L + "<1, 1, 4, 3>"),
    "dense20": dict(target="gauss_dense", d=20, variant=100, eps=0.05, kernel=L + "<2, 1, 4, 3>"),
    "gmm20": dict(target="gmm2", d=20, variant=100, eps=0.05, kernel=L + "<3, 1, 4, 3>"),
    "rw20": dict(target="roughwell_easy", d=20, variant=100, eps=0.1, kernel=L + "<4, 1, 4, 3>"),
    # funnel, x0 = 0.3 randn: oracle mean p by rung 0.54, 0.59, 0.64, 0.68 at eps = 0.1 (0.2 is too coarse: 0.21, 0.17, 0.28, 0.35)
    "funnel20": dict(target="funnel", d=20, variant=100, eps=0.1, kernel=L + "<5, 1, 4, 3>"),
    # logistic d = 12, n = 300: oracle mean p by rung 0.35, 0.39, 0.52, 0.67 at eps = 0.05 (0.1: 0.35 ... 0.45; 0.2: 0.05 at T = 1)
    "lr12_w1": dict(target="logistic", d=12, n=300, variant=101, eps=0.05, kernel=L + "<7, 1, 1, 3>"),
    "lr12_w4": dict(target="logistic", d=12, n=300, variant=100, eps=0.05, kernel=L + "<7, 1, 4, 3>"),
    # logistic d = 80, n = 200: oracle mean p by rung 0.34, 0.46, 0.56, 0.63 at eps = 0.05 (0.1: 0.05 at T = 1)
    "lr80": dict(target="logistic", d=80, n=200, variant=100, eps=0.05, kernel=L + "<7, 2, 4, 3>"),
    "k2": dict(target="gauss_diag", d=20, variant=100, eps=0.05, temps=[1.0, 2.0], kernel=L + "<1, 1, 4, 3>"),
    "k8": dict(target="gauss_diag", d=20, variant=100, eps=0.05, temps=geometric_ladder(1.0, 6.0, 8), kernel=L + "<1, 1, 4, 3>"),
    "k16": dict(target="gauss_diag", d=20, variant=100, eps=0.05, temps=geometric_ladder(1.0, 8.0, 16), n_rows=48,
                kernel=L + "<1, 1, 4, 3>"),
}
ORACLE_CASES = ("g20_w4", "g20_h14", "gmm20", "lr12_w4")     # the post-swap proposal against the float32 oracle


def blr_data(n, d, seed):
    """Synthetic logistic-regression data: features of scale 1 / sqrt(d), labels drawn at weights of scale 1.5."""
    rng = np.random.RandomState(seed)
    X = (rng.randn(n, d) / np.sqrt(d)).astype(np.float32)
    w = rng.randn(d) * 1.5
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ w))).astype(np.float32)
    return X, y


def blr_np(X, y, s2, W, dtype=np.float64):
    """(U, grad U) of the logistic-regression posterior in numpy at `dtype`."""
    X, y, W = (np.asarray(a, dtype) for a in (X, y, W))
    Lg = W @ X.T
    U = (np.logaddexp(dtype(0), Lg) - y * Lg).sum(1) + dtype(0.5) * (W * W).sum(1) / dtype(s2)
    sg = dtype(0.5) * (dtype(1) + np.tanh(dtype(0.5) * Lg))
    G = (sg - y) @ X + W / dtype(s2)
    return U.astype(dtype), G.astype(dtype)


class Case(object):
    """One row of CASES with its inputs: g (golden-shaped dict: nets, mask, step size, energy parameters), temps (float32
    values as doubles), K, nl, N, and the host arrays x0 (N, d), v (R M, N, d), dr (R M, N) u8, u (R M, N), swap_u (R, nl, K / 2)."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.kernel, self.variant = name, c["kernel"], int(c["variant"])
        self.target, self.d, self.H, self.hmc = c["target"], int(c["d"]), int(c.get("H", 10)), bool(c.get("hmc", False))
        self.temps = [float(t) for t in np.asarray(c.get("temps", TEMPS), np.float32)]
        self.K, self.N = len(self.temps), int(c.get("n_rows", N))
        self.nl = self.N // self.K
        self.eps = float(c["eps"])
        kind = self.target if self.target not in ("funnel", "logistic") else "gauss_diag"
        g = helpers.synthetic_case(kind, self.d, H=self.H, T=T, N=self.N, seed=SEED, eps=self.eps)
        rng = np.random.RandomState(DRAWS_SEED)
        self.x0 = g["x"]
        if self.target == "funnel":
            for k in ("energy.mu", "energy.i_sigma"):
                del g[k]
            g.update({"energy.kind": "funnel", "energy.sigma": np.float32(2.0)})
            self.x0 = (0.3 * rng.randn(self.N, self.d)).astype(np.float32)
        elif self.target == "logistic":
            self.X, self.y = blr_data(int(c["n"]), self.d, seed=13)
            self.x0 = (0.3 * rng.randn(self.N, self.d)).astype(np.float32)
        if self.hmc:
            g["hmc"] = 1
        self.g = g
        RM = R * M
        self.v = rng.randn(RM, self.N, self.d).astype(np.float32)
        self.dr = rng.randint(0, 2, size=(RM, self.N)).astype(np.uint8)
        self.u = rng.uniform(size=(RM, self.N)).astype(np.float32)
        self.swap_u = rng.uniform(size=(R, self.nl, self.K // 2)).astype(np.float32)
        self.labels0 = np.tile(np.arange(self.K), (self.nl, 1))

    # ---- the float64 / float32 numpy side --------------------------------------------------------------------------
    def oracle_energy(self, dtype=np.float64):
        """callable x -> (U, grad U) at `dtype`, untempered"""
        if self.target == "logistic":
            return lambda W: blr_np(self.X, self.y, PRIOR_VAR, W, dtype)
        return helpers.oracle_energy(self.g, dtype)

    def energy64(self, x):
        return np.asarray(self.oracle_energy(np.float64)(np.asarray(x, np.float64))[0], np.float64)

    def oracle_dynamics(self, dtype=np.float32, temperature=1.0):
        if self.target == "logistic":
            xn, vn = helpers.golden_nets(self.g)
            od = O.Dynamics(self.d, self.oracle_energy(dtype), T, self.eps, self.g["mask"], xn, vn, dtype=dtype)
        else:
            od = helpers.oracle_dynamics(self.g, dtype)
        od.temperature = dtype(np.float32(temperature))
        return od

    def tol(self, labels, U):
        """Near-tie margin of every pair's decision, (nl, K - 1): the suite's 1e-5 plus 4 float32 ulps of each of the two
        energies, scaled by the inverse-temperature gap -- `Dynamics.energy` and the trajectory kernel may sum a row's U in
        different orders across waves (at d = 300, U is about 150)."""
        U = np.abs(np.asarray(U, np.float64))
        inv = np.argsort(labels, axis=1)                             # row of rung k
        Ur = np.take_along_axis(U, inv, axis=1)                      # |U| by rung
        db = np.abs(np.diff(1.0 / np.asarray(self.temps, np.float64)))
        return BASE_TOL + ULPS * 2.0 ** -23 * db[None, :] * (Ur[:, :-1] + Ur[:, 1:])

    def check_inputs(self):
        """The conditions on a case's inputs, from the float64 oracle energy of x0 alone: round 0's reference sweep accepts at
        least one pair and rejects at least one, and replaying all R rounds on these energies leaves fewer than 1 % of the
        decisions inside the near-tie margin.  Returns (accepted, attempted, near share)."""
        from . import pt_reference as ref
        U = self.energy64(self.x0).reshape(self.nl, self.K)
        assert np.all(np.isfinite(U)), self.name
        lab, near_n, pairs = self.labels0, 0, 0
        acc0 = att0 = None
        for j in range(R):
            tol = self.tol(lab, U)
            lab, a, t, near = ref.sweep(lab, U, self.temps, j, self.swap_u[j], tol=tol)
            if j == 0:
                acc0, att0 = int(a.sum()), int(t.sum())
            near_n += int(near.sum())
            pairs += int(t.sum())
        assert 0 < acc0 < att0, (self.name, acc0, att0)
        assert float(tol.max()) <= 1e-3, (self.name, float(tol.max()))
        assert near_n < 0.01 * pairs, (self.name, near_n, pairs)
        return acc0, att0, near_n / float(pairs)

    # ---- the HIP side ------------------------------------------------------------------------------------------------
    def hip_dynamics(self):
        import torch
        from l2hmc_amd import Dynamics, LogisticRegression, layers
        g = self.g
        if self.target == "logistic":
            e = LogisticRegression(self.X, self.y, prior_var=PRIOR_VAR).get_energy_function()
            dyn = Dynamics(self.d, e, T=T, eps=self.eps, hmc=False, net_factory=layers.stq_network(self.H))
            dyn.mask = g["mask"]
            dyn.eps_override = self.eps
            with torch.no_grad():
                for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
                    for k in O.NET_KEYS:
                        w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
        elif self.hmc:
            dyn = Dynamics(self.d, helpers.hip_energy(g), T=T, eps=self.eps, hmc=True)
            dyn.eps_override = self.eps
        else:
            dyn = helpers.hip_dynamics(g)
        dyn.variant = self.variant
        return dyn


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]
