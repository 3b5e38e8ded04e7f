"""GPU: Bayesian logistic regression (L2HMC_ENERGY_LOGISTIC) on the fused kernels.  U and grad U against float64 numpy on
the LDS-staged and the streamed data path; trajectories against the float32 oracle (HMC, fused nets, nets on the GEMM engine);
the persistent loop against single launches bit for bit; temperature, the AIS bridge and ais_estimate; parallel tempering;
and the posterior mean of 8192 HMC chains against a float64 importance-sampling reference."""
import numpy as np
import pytest
import torch

from l2hmc_amd import Dynamics, LogisticRegression, ParallelTempering, _ffi, geometric_ladder, layers, sample_chain
from l2hmc_amd import distributions as D
from l2hmc_amd.ais import ais_estimate
from oracle import l2hmc_oracle as O
from tests import helpers
from tests import pt_reference as ref
from tests.helpers import abs_err, rel_err, to_dev, to_np

pytestmark = pytest.mark.gpu

PRIOR_VAR = 2.0


def blr_data(n, d, seed=0, scale=None, w_scale=1.5):
    rng = np.random.RandomState(seed)
    X = (rng.randn(n, d) * (1.0 / np.sqrt(d) if scale is None else scale)).astype(np.float32)
    w = rng.randn(d) * w_scale
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ w))).astype(np.float32)
    return X, y


def blr_np(X, y, s2, W, dtype=np.float64):
    """(U, grad U) of the logistic-regression posterior in numpy at `dtype`."""
    X, y, W = (np.asarray(a, dtype) for a in (X, y, W))
    L = W @ X.T
    U = (np.logaddexp(dtype(0), L) - y * L).sum(1) + dtype(0.5) * (W * W).sum(1) / dtype(s2)
    sg = dtype(0.5) * (dtype(1) + np.tanh(dtype(0.5) * L))
    G = (sg - y) @ X + W / dtype(s2)
    return U.astype(dtype), G.astype(dtype)


def oracle_energy(X, y, s2):
    return lambda W: blr_np(X, y, s2, W, np.float32)


def twin(g, e, hmc, H=10, variant=0, eps=None):
    """l2hmc_amd.Dynamics on energy e with the synthetic case's nets, mask and step size."""
    d, T = int(g["x_dim"]), int(g["T"])
    eps = float(g["eps"]) if eps is None else eps
    dyn = Dynamics(d, e, T=T, eps=eps, hmc=hmc, net_factory=None if hmc else layers.stq_network(H))
    dyn.mask = g["mask"]
    dyn.eps_override = eps
    dyn.variant = variant
    if not hmc:
        with torch.no_grad():
            for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
                for k in O.NET_KEYS:
                    w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    return dyn


def oracle_twin(g, X, y, hmc, eps=None, temperature=1.0):
    xn, vn = (None, None) if hmc else helpers.golden_nets(g)
    return O.Dynamics(int(g["x_dim"]), oracle_energy(X, y, PRIOR_VAR), int(g["T"]), float(g["eps"]) if eps is None else eps,
                      g["mask"], xn, vn, temperature=temperature, dtype=np.float32)


# ---- 1. U and grad U --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 1000, 8192])
@pytest.mark.parametrize("d", [2, 5, 25, 50, 128])
def test_energy_and_gradient_against_float64(n, d, monkeypatch):
    _energy_and_gradient_against_float64(n, d, monkeypatch)


# d = 40, 65, 96: 3, 5 and 6 live feature tiles -- 3 of the 4 compiled ones of one state tile per wave, 5 and 6 of the 8 of two
# (the plan goes from one to two state tiles per wave between 4 and 5); above, d = 2 .. 128 has 1, 2, 4 and 8
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("d", [40, 65, 96])
def test_energy_and_gradient_against_float64_at_partly_live_tile_counts(n, d, monkeypatch):
    _energy_and_gradient_against_float64(n, d, monkeypatch)


def _energy_and_gradient_against_float64(n, d, monkeypatch):
    X, y = blr_data(n, d, seed=n + d)
    e = LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function()
    W = (0.7 * np.random.RandomState(1).randn(40, d)).astype(np.float32)       # 40 chains: the last tile is partial
    Ur, Gr = blr_np(X, y, PRIOR_VAR, W)
    # n = 17: one live row in the second block -- the 15 padded rows would add 15 log 2 to U if they were not masked
    for mode in ("planned", "streamed"):
        if mode == "streamed":
            monkeypatch.setenv("L2HMC_LOGISTIC_LDS", "0")
        U, G = e.evaluate(to_dev(W), want_grad=True)
        helpers.check_grads_per_tensor("n=%d d=%d %s" % (n, d, mode), {"U": to_np(U), "g": to_np(G)}, {"U": Ur, "g": Gr},
                                       rel=1e-5, floor=0.0)


# ---- 2. trajectories against the float32 oracle ---------------------------------------------------------------------------
# (n, d, eps, H): H = 0 is HMC, 10 the fused nets, 24 nets on the GEMM engine; d = 100 runs two state tiles per wave
CASES = [(n, d, eps, H) for (n, d, eps) in [(17, 5, 0.1), (200, 25, 0.05), (1000, 25, 0.03), (300, 100, 0.03)] for H in (0, 10)]
CASES += [(200, 25, 0.05, 24)]


@pytest.mark.parametrize("n,d,eps,H", CASES)
def test_trajectories_match_the_oracle(n, d, eps, H):
    hmc = H == 0
    g = helpers.synthetic_case("gauss_diag", d, H=max(H, 1), T=6, N=48, seed=d, eps=eps)
    X, y = blr_data(n, d, seed=7)
    e = LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function()
    dyn, od = twin(g, e, hmc, H=max(H, 1)), oracle_twin(g, X, y, hmc)
    if H == 24:
        assert dyn._split                                          # nets wider than H = 15: the GEMM engine, grad U from l2hmc_energy
    x = (0.5 * np.random.RandomState(2).randn(48, d)).astype(np.float32)
    v = np.random.RandomState(3).randn(48, d).astype(np.float32)
    xd, vd = to_dev(x), to_dev(v)
    for s in (0, 3):
        for got, want in ((dyn._forward_step(xd, vd, s), od.forward_step(x, v, s)),
                          (dyn._backward_step(xd, vd, s), od.backward_step(x, v, s))):
            assert rel_err(to_np(got[0]), want[0]) < 3e-5 and rel_err(to_np(got[1]), want[1]) < 3e-5, (n, d, H, s)
            assert rel_err(to_np(got[2]), want[2]) < 1e-4, (n, d, H, s)
    if not dyn._split:
        assert _ffi.last_kernel().startswith("traj_kernel<7, ")
    X1, V1, lj = dyn.forward(xd, init_v=vd, log_jac=True)
    _, _, p = dyn.forward(xd, init_v=vd)
    rX, rV, rlj = od.forward(x, v, log_jac=True)
    _, _, rp = od.forward(x, v)
    assert rel_err(to_np(X1), rX) < 3e-5 and rel_err(to_np(V1), rV) < 3e-5, (n, d, H)
    assert rel_err(to_np(lj), rlj) < 1e-4 and abs_err(to_np(p), rp) < 1e-4, (n, d, H)
    assert 0.0 < float(to_np(p).mean()) <= 1.0


# ---- 3. the persistent loop is a chain of single launches -----------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_persistent_loop_equals_single_launches_bit_for_bit(hmc):
    n, d = 500, 25
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=64, seed=1, eps=0.04)
    X, y = blr_data(n, d, seed=11)
    dyn = twin(g, LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function(), hmc)
    x0 = to_dev((0.3 * np.random.RandomState(4).randn(64, d)).astype(np.float32))
    M = 6
    xs, ps, hist = sample_chain(x0, dyn, M, seed=99, record=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_kernel<7, ")
    x = x0
    for m in range(M):
        x, p, _ = sample_chain(x, dyn, 1, seed=99, proposal0=m)
        assert torch.equal(p[0], ps[m]) and torch.equal(x, hist[m]), m
    assert torch.equal(x, xs)
    assert 0.2 < float(ps.mean()) <= 1.0
    for variant in (16, 8, 32):                                    # the one-wave tile, LDS-resident-state and lane kernels
        dyn.variant = variant
        with pytest.raises(RuntimeError, match="general kernel only"):
            sample_chain(x0, dyn, 1, seed=99)


# ---- 4. temperature, the AIS bridge, ais_estimate ----------------------------------------------------------------------
def test_temperature_and_anneal_bridge():
    n, d = 300, 8
    X, y = blr_data(n, d, seed=3)
    e = LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function()
    dyn = Dynamics(d, e, T=5, eps=0.05, hmc=True)
    W = (0.5 * np.random.RandomState(5).randn(33, d)).astype(np.float32)
    Ur, Gr = blr_np(X, y, PRIOR_VAR, W)
    dyn.use_temperature, dyn.temperature = True, 2.5
    helpers.check_grads_per_tensor("T = 2.5", {"U": to_np(dyn.energy(to_dev(W))), "g": to_np(dyn.grad_energy(to_dev(W)))},
                                   {"U": Ur / 2.5, "g": Gr / 2.5}, rel=1e-5, floor=0.0)
    dyn.use_temperature, dyn.temperature = False, 1.0
    b = 0.3
    dyn.anneal_beta = b
    q = 0.5 * np.square(W.astype(np.float64)).sum(1)
    helpers.check_grads_per_tensor("beta = 0.3", {"U": to_np(dyn.energy(to_dev(W))), "g": to_np(dyn.grad_energy(to_dev(W)))},
                                   {"U": (1 - b) * q + b * Ur, "g": (1 - b) * W + b * Gr}, rel=1e-5, floor=0.0)


def test_ais_matches_a_float32_replay():
    n, d, N, K, T, eps = 200, 6, 64, 5, 4, 0.1
    X, y = blr_data(n, d, seed=8)
    e = LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function()
    init = D.Gaussian(np.zeros(d), np.eye(d)).get_energy_function()
    rng = np.random.RandomState(6)
    x0 = rng.randn(N, d).astype(np.float32)
    draws = {"v0": rng.randn(N, d).astype(np.float32), "normals": rng.randn(K, N, d).astype(np.float32),
             "u": rng.uniform(size=(K, N)).astype(np.float32)}
    est, mean_alpha, st = ais_estimate(init, e, K, x0, step_size=eps, leapfrogs=T, x_dim=d, draws=draws, return_state=True)
    assert _ffi.last_kernel().startswith("traj_kernel<7, ")

    def std_normal(z):
        return 0.5 * np.square(z).sum(1).astype(np.float32), z.astype(np.float32)
    rest, ralpha, rst = O.ais_estimate(std_normal, oracle_energy(X, y, PRIOR_VAR), K, x0, draws["v0"], draws["normals"],
                                       draws["u"], step_size=eps, leapfrogs=T)
    assert abs_err(to_np(st["w"]), rst["w"]) < 1e-4 * max(1.0, float(np.abs(rst["w"]).max()))
    assert abs(float(mean_alpha) - ralpha) < 1e-5
    assert rel_err(to_np(st["x"]), rst["x"]) < 1e-4
    assert np.isfinite(float(est))


# ---- 5. parallel tempering ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_equal_rungs_are_the_scalar_path_bit_for_bit(hmc):
    n, d = 400, 12
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=64, seed=2, eps=0.05)
    X, y = blr_data(n, d, seed=12)
    dyn = twin(g, LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function(), hmc, variant=100)
    K, nl, R, M = 4, 32, 3, 2
    x0 = to_dev((0.3 * np.random.RandomState(1).randn(K * nl, d)).astype(np.float32))
    dyn.use_temperature, dyn.temperature = True, 2.5
    xs, ps, _ = sample_chain(x0, dyn, R * M, seed=11)
    dyn.use_temperature, dyn.temperature = False, 1.0
    pt = ParallelTempering(dyn, [2.5] * K, nl, seed=11)
    o = pt.run(x0, R, M, record_rungs=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_ladder_kernel<7, ")
    assert torch.equal(o["x"], xs) and torch.equal(o["p"], ps)
    assert torch.equal(o["swaps_accepted"], o["swaps_attempted"]) and int(o["swaps_attempted"].sum()) > 0


def test_swap_counters_and_round_trips_match_the_reference():
    n, d = 300, 4
    X, y = blr_data(n, d, seed=13)
    dyn = Dynamics(d, LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function(), T=5, eps=0.08, hmc=True)
    dyn.eps_override = 0.08
    temps, nl, K, R, M = geometric_ladder(1.0, 8.0, 4), 32, 4, 24, 2
    pt = ParallelTempering(dyn, temps, nl, seed=21)
    x0 = to_dev((0.3 * np.random.RandomState(2).randn(K * nl, d)).astype(np.float32))
    o = pt.run(x0, R, M, record_rungs=True, record_states=True)
    x_hist = o["x_hist"]
    t32 = np.asarray(temps, np.float32).astype(np.float64)

    def U_of(xs):
        return to_np(dyn.energy(xs)).astype(np.float64)
    compared, acc, att, trips = ref.replay(pt, o, x_hist, U_of, t32, R, M, None, 21, np.tile(np.arange(K), (nl, 1)), tol=1e-5)
    assert compared >= 0.95 * R * nl
    assert np.array_equal(att, to_np(o["swaps_attempted"]))
    assert np.abs(acc - to_np(o["swaps_accepted"])).sum() <= R * nl - compared
    assert np.array_equal(trips, to_np(o["round_trips"]))
    assert 0 < int(acc.sum()) < int(att.sum())


# ---- 6. statistics ----------------------------------------------------------------------------------------------------------
def laplace_is_mean(X, y, s2, n_draws=400000, seed=0, chunk=10000):
    """Posterior mean by self-normalised importance sampling from the Laplace approximation (antithetic pairs), float64:
    (mean, its standard error, mode, Cholesky factor of the Laplace covariance)."""
    X, y = X.astype(np.float64), y.astype(np.float64)
    w = np.zeros(X.shape[1])
    for _ in range(50):                                            # Newton on U
        sg = 1.0 / (1.0 + np.exp(-X @ w))
        gr = X.T @ (sg - y) + w / s2
        Hs = (X * (sg * (1 - sg))[:, None]).T @ X + np.eye(X.shape[1]) / s2
        w = w - np.linalg.solve(Hs, gr)
    C = np.linalg.inv(Hs)
    Lc = np.linalg.cholesky(C)
    Z = np.random.RandomState(seed).randn(n_draws // 2, X.shape[1])
    Z = np.concatenate([Z, -Z])
    Wd = w + Z @ Lc.T
    U = np.concatenate([blr_np(X, y, s2, Wd[i:i + chunk])[0] for i in range(0, len(Wd), chunk)])
    lw = -U + 0.5 * np.square(Z).sum(1)
    wt = np.exp(lw - lw.max())
    wt /= wt.sum()
    mean = (wt[:, None] * Wd).sum(0)
    se = np.sqrt((np.square(wt)[:, None] * np.square(Wd - mean)).sum(0))
    return mean, se, w, Lc


def test_posterior_mean_matches_importance_sampling():
    n, d, N, M = 2000, 5, 8192, 300
    X, y = blr_data(n, d, seed=21, scale=1.0, w_scale=0.8)
    ref_mean, ref_se, mode, Lc = laplace_is_mean(X, y, PRIOR_VAR)
    dyn = Dynamics(d, LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function(), T=10, eps=0.01, hmc=True)
    dyn.eps_override = 0.01
    x0 = (mode + np.random.RandomState(3).randn(N, d) @ Lc.T).astype(np.float32)
    _, p, hist = sample_chain(to_dev(x0), dyn, M, seed=5, record=True)
    h = to_np(hist[M // 2:]).astype(np.float64)                   # (M / 2, N, d)
    per_chain = h.mean(axis=0)
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(N)
    z = np.abs(mean - ref_mean) / np.sqrt(np.square(se) + np.square(ref_se))
    print("posterior mean z-scores", z, "accept", float(p.mean()))
    assert float(p.mean()) > 0.5
    assert np.all(z < 5.0), (mean, ref_mean, se)
