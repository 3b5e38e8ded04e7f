"""GPU: Bayesian Poisson regression (L2HMC_ENERGY_POISSON) on the fused kernels, mirroring tests/test_gpu_logistic.py.  U and
grad U within the bounds of tests/poisson_target_case.py on the LDS-staged and the streamed data path; trajectories against the
float32 oracle (HMC, fused nets, nets on the GEMM engine) at tolerances computed from the oracle alone; float32 overflow of exp
as a rejection; the persistent loop against single launches bit for bit; temperature, the AIS bridge and ais_estimate; parallel
tempering; warm-up; the posterior mean of 8192 HMC chains against float64 importance sampling, with the model's own LOO and WAIC
on that history; the training refusal and the state_dict route."""
import numpy as np
import pytest
import torch

from l2hmc_amd import Dynamics, ParallelTempering, PoissonRegression, _ffi, geometric_ladder, layers, sample_chain, warmup
from l2hmc_amd import distributions as D
from l2hmc_amd.ais import ais_estimate
from oracle import l2hmc_oracle as O
from tests import poisson_target_case as pc
from tests import pt_reference as ref
from tests.helpers import to_dev, to_np

pytestmark = pytest.mark.gpu

S2 = pc.PRIOR_VAR


def fused(X, y, o):
    return PoissonRegression(X, y, offset=o, prior_var=S2).get_energy_function(fused=True)


def twin(g, e, hmc, H, eps, variant=0):
    """l2hmc_amd.Dynamics on energy e with the synthetic case's nets, mask and the step size eps."""
    dyn = Dynamics(int(g["x_dim"]), e, T=int(g["T"]), eps=eps, hmc=hmc, net_factory=None if hmc else layers.stq_network(H))
    dyn.mask = g["mask"]
    dyn.eps_override = eps
    dyn.variant = variant
    if not hmc:
        with torch.no_grad():
            for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
                for k in O.NET_KEYS:
                    w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    return dyn


def hmc_eps(X, y, o, x, T, seed=3):
    """A step size for HMC from x, chosen on the float32 oracle (mean accept probability in (0.2, 1))."""
    v = np.random.RandomState(seed).randn(*x.shape).astype(np.float32)
    g = {"x_dim": x.shape[1], "T": T, "mask": np.zeros((T, x.shape[1]), dtype=np.float32)}
    return pc.choose_eps(lambda e: pc.oracle_dynamics(g, X, y, o, True, e), x, v)


# ---- 1. U and grad U --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 1000, 8192])
@pytest.mark.parametrize("d", [2, 5, 25, 50, 128])
def test_energy_and_gradient_within_the_bounds(n, d, monkeypatch):
    _energy_and_gradient_within_the_bounds(n, d, monkeypatch)


# d = 40, 65, 96: 3, 5 and 6 live feature tiles -- 3 of the 4 compiled ones of one state tile per wave, 5 and 6 of the 8 of two
# (the plan goes from one to two state tiles per wave between 4 and 5); above, d = 2 .. 128 has 1, 2, 4 and 8
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("d", [40, 65, 96])
def test_energy_and_gradient_within_the_bounds_at_partly_live_tile_counts(n, d, monkeypatch):
    _energy_and_gradient_within_the_bounds(n, d, monkeypatch)


def _energy_and_gradient_within_the_bounds(n, d, monkeypatch):
    W, X, y, o = pc.case(40, n, d)                                # 40 chains: the last tile is partial
    zero = np.zeros_like(o)
    runs = {}
    # n = 17: one live row in the second block -- the 15 padded rows would add 15 exp(0) to U if they were not masked
    for mode in ("planned", "streamed"):
        if mode == "streamed":
            monkeypatch.setenv("L2HMC_LOGISTIC_LDS", "0")
        for name, model, oo in (("offsets", PoissonRegression(X, y, offset=o, prior_var=S2), o),
                                ("zeros", PoissonRegression(X, y, offset=zero, prior_var=S2), zero),
                                ("none", PoissonRegression(X, y, prior_var=S2), zero)):
            U, G = model.get_energy_function(fused=True).evaluate(to_dev(W), want_grad=True)
            U, G = to_np(U), to_np(G)
            runs[mode, name] = (U, G)
            Ur, Gr = pc.energy(W, X, y, oo)
            sU, sg = pc.used(U, G, Ur, Gr, pc.bounds(W, X, y, oo))
            print("n=%d d=%d %s %s: uses %.3f of the U bound, %.3f of the grad U bound" % (n, d, mode, name, sU, sg))
            assert sU <= 1.0 and sg <= 1.0, (n, d, mode, name, sU, sg)
        for a, b in zip(runs[mode, "zeros"], runs[mode, "none"]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, d, mode)


# ---- 2. trajectories against the float32 oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,H", pc.TRAJ_CASES)
def test_trajectories_match_the_oracle(n, d, H):
    c = pc.traj_case(n, d, H)
    hmc, r, dist = c["hmc"], c["ref"], c["dist"]
    dyn = twin(c["g"], fused(c["X"], c["y"], c["o"]), hmc, max(H, 1), c["eps"])
    if H == 24:
        assert dyn._split                                          # nets wider than H = 15: the GEMM engine, grad U from l2hmc_energy
    xd, vd = to_dev(c["x"]), to_dev(c["v"])
    print("n=%d d=%d H=%d eps=%g oracle accept %.3f" % (n, d, H, c["eps"], float(r["forward"][3].mean())))
    for s in (0, 3):
        for key, got in (("fwd%d" % s, dyn._forward_step(xd, vd, s)), ("bwd%d" % s, dyn._backward_step(xd, vd, s))):
            errs = tuple(pc.rel_err(to_np(got[i]), r[key][i]) for i in range(3))
            tols = (pc.gate(pc.STATE_GATE, dist[key][0]), pc.gate(pc.STATE_GATE, dist[key][1]), pc.gate(pc.SCALAR_GATE, dist[key][2]))
            print("  %s: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (key, errs, dist[key], tols))
            assert all(e < t for e, t in zip(errs, tols)), (n, d, H, key, errs, tols)
    if not dyn._split:
        assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    X1, V1, lj = dyn.forward(xd, init_v=vd, log_jac=True)
    _, _, p = dyn.forward(xd, init_v=vd)
    rX, rV, rlj, rp = r["forward"]
    errs = (pc.rel_err(to_np(X1), rX), pc.rel_err(to_np(V1), rV), pc.rel_err(to_np(lj), rlj), pc.abs_err(to_np(p), rp))
    tols = tuple(pc.gate(b, dd) for b, dd in zip((pc.STATE_GATE, pc.STATE_GATE, pc.SCALAR_GATE, pc.SCALAR_GATE), dist["forward"]))
    print("  forward: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (errs, dist["forward"], tols))
    assert all(e < t for e, t in zip(errs, tols)), (n, d, H, errs, tols)
    assert 0.0 < float(to_np(p).mean()) <= 1.0


# ---- 3. overflow is a rejection ---------------------------------------------------------------------------------------------
def test_overflow_is_a_rejection_not_a_wrong_number():
    c = pc.overflow_case()
    bad, ok = c["nonfinite"], c["accepted"]
    assert bad.sum() >= pc.OVER_N // 8 and ok.sum() >= pc.OVER_N // 8
    dyn = Dynamics(5, fused(c["X"], c["y"], c["o"]), T=c["T"], eps=c["eps"], hmc=True)
    dyn.eps_override = c["eps"]
    xd, vd = to_dev(c["x"]), to_dev(c["v"])
    _, _, p = dyn.forward(xd, init_v=vd)
    p = to_np(p)
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    assert np.all(p[bad] == 0.0), p[bad]
    tol = pc.gate(pc.SCALAR_GATE, c["dist_p"])
    err = pc.abs_err(p[ok], c["p"][ok])
    print("overflow: %d non-finite, %d accepted; accept probability kernel-oracle %.3g, float32-float64 oracle %.3g" % (
        bad.sum(), ok.sum(), err, c["dist_p"]))
    assert err < tol and np.all(np.isfinite(p))
    xn, ps, _ = sample_chain(xd, dyn, 1, v=vd, u=to_dev(c["u"]))
    assert np.all(to_np(ps)[0][bad] == 0.0)
    assert np.array_equal(to_np(xn)[bad].view(np.uint32), c["x"][bad].view(np.uint32))
    assert np.all(np.isfinite(to_np(xn)))


# ---- 4. the persistent loop is a chain of single launches -----------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_persistent_loop_equals_single_launches_bit_for_bit(hmc):
    n, d, N, M = 500, 25, 64, 6
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=N, seed=1, eps=0.1)
    x, X, y, o = pc.case(N, n, d)
    v = np.random.RandomState(3).randn(N, d).astype(np.float32)
    # (half of the first proposal accepted: the loop's own draws and the states it reaches stay above the 0.2 asserted below)
    eps = pc.choose_eps(lambda e: pc.oracle_dynamics(g, X, y, o, hmc, e), x, v, lo=0.5)
    dyn = twin(g, fused(X, y, o), hmc, 10, eps)
    x0 = to_dev(x)
    xs, ps, hist = sample_chain(x0, dyn, M, seed=99, record=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    xc = x0
    for m in range(M):
        xc, p, _ = sample_chain(xc, dyn, 1, seed=99, proposal0=m)
        assert torch.equal(p[0], ps[m]) and torch.equal(xc, hist[m]), m
    assert torch.equal(xc, xs)
    assert 0.2 < float(ps.mean()) <= 1.0
    for variant in (16, 8, 32):                                    # the one-wave tile, LDS-resident-state and lane kernels
        dyn.variant = variant
        with pytest.raises(RuntimeError, match="general kernel only"):
            sample_chain(x0, dyn, 1, seed=99)


# ---- 5. temperature, the AIS bridge, ais_estimate ----------------------------------------------------------------------
def test_temperature_and_anneal_bridge():
    n, d = 300, 8
    W, X, y, o = pc.case(33, n, d)
    dyn = Dynamics(d, fused(X, y, o), T=5, eps=0.01, hmc=True)
    dyn.use_temperature, dyn.temperature = True, 2.5
    Ur, Gr, b = pc.scaled(W, X, y, o, temperature=2.5)
    sU, sg = pc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("T = 2.5: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0
    dyn.use_temperature, dyn.temperature = False, 1.0
    dyn.anneal_beta = 0.3
    Ur, Gr, b = pc.scaled(W, X, y, o, beta=0.3)
    sU, sg = pc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("beta = 0.3: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0


def test_ais_matches_a_float32_replay():
    n, d, N, K, T = 200, 6, 64, 5, 4
    rng = np.random.RandomState(6)
    x0 = rng.randn(N, d).astype(np.float32)
    draws = {"v0": rng.randn(N, d).astype(np.float32), "normals": rng.randn(K, N, d).astype(np.float32),
             "u": rng.uniform(size=(K, N)).astype(np.float32)}
    # the generator of `case` with the scale on X: max |x_i . x0| = 3 over the standard-normal starts of the anneal
    _, X, _, o = pc.case(N, n, d)
    X = (X * (3.0 / np.abs(x0.astype(np.float64) @ X.T.astype(np.float64)).max())).astype(np.float32)
    y = np.random.RandomState(7).poisson(np.exp(X.astype(np.float64) @ x0[0].astype(np.float64) + o)).astype(np.float32)
    eps = hmc_eps(X, y, o, x0, T)
    e = fused(X, y, o)
    init = D.Gaussian(np.zeros(d), np.eye(d)).get_energy_function()
    est, mean_alpha, st = ais_estimate(init, e, K, x0, step_size=eps, leapfrogs=T, x_dim=d, draws=draws, return_state=True)
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")

    def std_normal(z):
        return 0.5 * np.square(z).sum(1).astype(np.float32), z.astype(np.float32)
    rest, ralpha, rst = O.ais_estimate(std_normal, pc.oracle_energy(X, y, o), K, x0, draws["v0"], draws["normals"],
                                       draws["u"], step_size=eps, leapfrogs=T)
    print("ais: eps %g, mean alpha %.4f (oracle %.4f)" % (eps, float(mean_alpha), ralpha))
    assert pc.abs_err(to_np(st["w"]), rst["w"]) < 1e-4 * max(1.0, float(np.abs(rst["w"]).max()))
    assert abs(float(mean_alpha) - ralpha) < 1e-5
    assert pc.rel_err(to_np(st["x"]), rst["x"]) < 1e-4
    assert np.isfinite(float(est))


# ---- 6. parallel tempering ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_equal_rungs_are_the_scalar_path_bit_for_bit(hmc):
    n, d = 400, 12
    K, nl, R, M = 4, 32, 3, 2
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=K * nl, seed=2, eps=0.1)
    x, X, y, o = pc.case(K * nl, n, d)
    v = np.random.RandomState(3).randn(K * nl, d).astype(np.float32)
    eps = pc.choose_eps(lambda e: pc.oracle_dynamics(g, X, y, o, hmc, e, temperature=2.5), x, v)
    dyn = twin(g, fused(X, y, o), hmc, 10, eps, variant=100)
    x0 = to_dev(x)
    dyn.use_temperature, dyn.temperature = True, 2.5
    xs, ps, _ = sample_chain(x0, dyn, R * M, seed=11)
    dyn.use_temperature, dyn.temperature = False, 1.0
    pt = ParallelTempering(dyn, [2.5] * K, nl, seed=11)
    out = pt.run(x0, R, M, record_rungs=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_ladder_kernel<8, ")
    assert torch.equal(out["x"], xs) and torch.equal(out["p"], ps)
    assert torch.equal(out["swaps_accepted"], out["swaps_attempted"]) and int(out["swaps_attempted"].sum()) > 0
    assert float(ps.mean()) > 0.0


def test_swap_counters_and_round_trips_match_the_reference():
    n, d = 300, 4
    temps, nl, K, R, M = geometric_ladder(1.0, 8.0, 4), 32, 4, 24, 2
    x, X, y, o = pc.case(K * nl, n, d)
    eps = hmc_eps(X, y, o, x, 5)
    dyn = Dynamics(d, fused(X, y, o), T=5, eps=eps, hmc=True)
    dyn.eps_override = eps
    pt = ParallelTempering(dyn, temps, nl, seed=21)
    out = pt.run(to_dev(x), R, M, record_rungs=True, record_states=True)
    assert _ffi.last_kernel().startswith("traj_ladder_kernel<8, ")
    t32 = np.asarray(temps, np.float32).astype(np.float64)

    def U_of(xs):
        return to_np(dyn.energy(xs)).astype(np.float64)
    compared, acc, att, trips = ref.replay(pt, out, out["x_hist"], U_of, t32, R, M, None, 21, np.tile(np.arange(K), (nl, 1)), tol=1e-5)
    assert compared >= 0.95 * R * nl
    assert np.array_equal(att, to_np(out["swaps_attempted"]))
    assert np.abs(acc - to_np(out["swaps_accepted"])).sum() <= R * nl - compared
    assert np.array_equal(trips, to_np(out["round_trips"]))
    assert 0 < int(acc.sum()) < int(att.sum())


# ---- 7. warm-up ---------------------------------------------------------------------------------------------------------------
def test_warmup_adapts_the_step_size_on_the_fused_target():
    n, d, N, target = 300, 8, 256, 0.8
    x, X, y, o = pc.case(N, n, d)
    e = fused(X, y, o)

    def run():
        dyn = Dynamics(d, e, T=5, eps=1e-3, hmc=True)
        xw, info = warmup(to_dev(x), dyn, 60, target_accept=target, seed=4)
        return dyn, xw, info
    dyn, xw, info = run()
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    assert np.isfinite(info.eps) and 0.0 < info.eps < 1e3 and np.float32(info.log_eps) == dyn.alpha.item()
    _, p, _ = sample_chain(xw, dyn, 40, seed=4, proposal0=info.next_proposal0)
    acc = float(p.double().mean())
    print("warm-up: eps %.5f, accept %.4f over 40 further proposals (%d search + %d averaging updates)" % (
        info.eps, acc, info.n_search, info.n_averaged))
    assert abs(acc - target) <= 0.1
    dyn2, xw2, info2 = run()
    assert torch.equal(dyn2.alpha.view(torch.int32), dyn.alpha.view(torch.int32))
    assert torch.equal(xw2, xw) and torch.equal(info2.state.view(torch.int64), info.state.view(torch.int64))


# ---- 8. statistics ----------------------------------------------------------------------------------------------------------
def test_posterior_mean_matches_importance_sampling_and_the_history_feeds_loo():
    n, d, N, M = 2000, 5, 8192, 300
    _, X, y, o = pc.case(4, n, d)
    ref_mean, ref_se, mode, Lc = pc.laplace_is_mean(X, y, o)
    model = PoissonRegression(X, y, offset=o, prior_var=S2)
    # ten leapfrog steps across about two posterior standard deviations of the stiffest direction
    eps = 0.2 * float(np.sqrt(np.linalg.eigvalsh(Lc @ Lc.T).min()))
    dyn = Dynamics(d, model.get_energy_function(fused=True), T=10, eps=eps, hmc=True)
    dyn.eps_override = eps
    x0 = (mode + np.random.RandomState(3).randn(N, d) @ Lc.T).astype(np.float32)
    _, p, hist = sample_chain(to_dev(x0), dyn, M, seed=5, record=True)
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    h = to_np(hist[M // 2:]).astype(np.float64)                   # (M / 2, N, d)
    per_chain = h.mean(axis=0)
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(N)
    z = np.abs(mean - ref_mean) / np.sqrt(np.square(se) + np.square(ref_se))
    print("posterior mean z-scores", z, "accept", float(p.mean()), "eps", eps)
    assert float(p.mean()) > 0.5
    assert np.all(z < 5.0), (mean, ref_mean, se)
    draws = hist[M - 8:]                                          # the same device history, read where it lies (65536 draws)
    s, w = model.loo(draws), model.waic(draws)
    print("elpd_loo %.2f  elpd_waic %.2f" % (s.elpd_loo, w.elpd_waic))
    assert np.isfinite(s.elpd_loo) and np.isfinite(w.elpd_waic)


# ---- 9. training ----------------------------------------------------------------------------------------------------------------
def test_trainer_refuses_and_a_slow_path_state_dict_loads():
    from l2hmc_amd.training import Trainer
    n, d, N = 100, 5, 64
    x, X, y, o = pc.case(N, n, d)
    model = PoissonRegression(X, y, offset=o, prior_var=S2)
    torch.manual_seed(0)
    slow = Dynamics(d, model.get_energy_function(), T=4, eps=0.01, net_factory=layers.stq_network(10))
    fast = Dynamics(d, model.get_energy_function(fused=True), T=4, eps=0.02, net_factory=layers.stq_network(10))
    with pytest.raises(NotImplementedError, match=r"train on the slow path.*get_energy_function\(\).*load_state_dict"):
        Trainer(fast)
    fast.load_state_dict(slow.state_dict())
    for (k, a), (k2, b) in zip(slow.parameters(), fast.parameters()):
        assert k == k2 and torch.equal(a.detach(), b.detach()), k
    xs, ps, _ = sample_chain(to_dev(x), fast, 3, seed=1)
    assert _ffi.last_kernel().startswith("traj_kernel<8, ")
    assert torch.isfinite(xs).all() and torch.isfinite(ps).all() and float(ps.mean()) > 0.0
