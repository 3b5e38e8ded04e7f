"""GPU: binomial regression with the probit link on the fused trajectory kernels (L2HMC_ENERGY_PROBIT = 10), mirroring
tests/test_gpu_binomial_target.py.  U and grad U within the bounds of tests/probit_case.py on the LDS-staged and the streamed data
path; the EDGE rows (t to +-30); trajectories against the float32 oracle (HMC, fused nets, nets on the GEMM engine) at
tolerances computed from the oracle alone; the persistent loop against single launches bit for bit; equal ladder rungs against
the scalar path bit for bit; temperature and the AIS bridge; warm-up; the training refusal and the state_dict route; the posterior
mean of HMC chains against float64 importance sampling, with the model's own LOO and WAIC on that history."""
import numpy as np
import pytest
import torch

from l2hmc_amd import Dynamics, ParallelTempering, ProbitRegression, _ffi, layers, sample_chain, warmup
from oracle import l2hmc_oracle as O
from tests import poisson_target_case as pt
from tests import probit_case as pc
from tests.helpers import to_dev, to_np

pytestmark = pytest.mark.gpu

S2 = pc.PRIOR_VAR
_SHARES = {"U": 0.0, "g": 0.0}


def fused(c):
    return pc.model(c, prior_var=S2).get_energy_function(fused=True)


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


def _both_paths(c, monkeypatch, what):
    """U and grad U of the case's chains on the staged and on the streamed data path, each within the bounds."""
    Ur, Gr = pc.energy(c)
    b = pc.bounds(c)
    out = {}
    for mode in ("planned", "streamed"):
        if mode == "streamed":
            monkeypatch.setenv("L2HMC_LOGISTIC_LDS", "0")
        U, G = fused(c).evaluate(to_dev(c["W"]), want_grad=True)
        U, G = to_np(U), to_np(G)
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(G))
        sU, sg = pc.used(U, G, Ur, Gr, b)
        _SHARES["U"], _SHARES["g"] = max(_SHARES["U"], sU), max(_SHARES["g"], sg)
        print("%s %s: uses %.3f of the U bound, %.3f of the grad U bound (largest so far %.3f, %.3f)" % (
            what, mode, sU, sg, _SHARES["U"], _SHARES["g"]))
        assert sU <= 1.0 and sg <= 1.0, (what, mode, sU, sg)
        out[mode] = (U, G)
    return out


# ---- U and grad U -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 1000])
@pytest.mark.parametrize("d", [2, 25, 50, 128])
def test_energy_and_gradient_within_the_bounds(n, d, monkeypatch):
    # 40 chains: the last tile is partial.  n = 17: one live row in the second block -- its 15 padded rows carry weight 0
    # and are masked besides (log Phi(0) of a padded row would add log 2 per trial); trials mix 1, small and 50
    _both_paths(pc.case(40, n, d), monkeypatch, "probit n=%d d=%d" % (n, d))


# d = 40, 65, 96: 3, 5 and 6 live feature tiles of the compiled 4 / 8
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("d", [40, 65, 96])
def test_energy_and_gradient_within_the_bounds_at_partly_live_tile_counts(n, d, monkeypatch):
    _both_paths(pc.case(40, n, d), monkeypatch, "probit n=%d d=%d" % (n, d))


def test_edge_rows_are_finite_and_within_the_bounds(monkeypatch):
    """EDGE: rows at t near 0, +-5, +-9, +-15 and +-30 with y = 0, y = m and between: no inf or NaN in U or the gradient, both
    inside the bounds -- the tails where a log of 0.5 erfc returns -inf and 1 - Phi returns 0."""
    out = _both_paths(pc.EDGE, monkeypatch, "EDGE")
    assert np.array_equal(out["planned"][0], out["streamed"][0])


# ---- trajectories against the float32 oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,H", pc.TRAJ_CASES)
def test_trajectories_match_the_oracle(n, d, H):
    t = pc.traj_case(n, d, H)
    hmc, r, dist = t["hmc"], t["ref"], t["dist"]
    dyn = twin(t["g"], fused(t["c"]), hmc, max(H, 1), t["eps"])
    if H == 24:
        assert dyn._split                                          # nets wider than H = 15: the GEMM engine, grad U from l2hmc_energy
    xd, vd = to_dev(t["x"]), to_dev(t["v"])
    print("n=%d d=%d H=%d eps=%g oracle accept %.3f" % (n, d, H, t["eps"], float(r["forward"][3].mean())))
    for s in (0, 3):
        for key, got in (("fwd%d" % s, dyn._forward_step(xd, vd, s)), ("bwd%d" % s, dyn._backward_step(xd, vd, s))):
            errs = tuple(pt.rel_err(to_np(got[i]), r[key][i]) for i in range(3))
            tols = (pt.gate(pt.STATE_GATE, dist[key][0]), pt.gate(pt.STATE_GATE, dist[key][1]), pt.gate(pt.SCALAR_GATE, dist[key][2]))
            print("  %s: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (key, errs, dist[key], tols))
            assert all(e < tl for e, tl in zip(errs, tols)), (n, d, H, key, errs, tols)
    if not dyn._split:
        assert _ffi.last_kernel().startswith("traj_kernel<10, ")
    X1, V1, lj = dyn.forward(xd, init_v=vd, log_jac=True)
    _, _, p = dyn.forward(xd, init_v=vd)
    rX, rV, rlj, rp = r["forward"]
    errs = (pt.rel_err(to_np(X1), rX), pt.rel_err(to_np(V1), rV), pt.rel_err(to_np(lj), rlj), pt.abs_err(to_np(p), rp))
    tols = tuple(pt.gate(b, dd) for b, dd in zip((pt.STATE_GATE, pt.STATE_GATE, pt.SCALAR_GATE, pt.SCALAR_GATE), dist["forward"]))
    print("  forward: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (errs, dist["forward"], tols))
    assert all(e < tl for e, tl in zip(errs, tols)), (n, d, H, errs, tols)
    assert 0.0 < float(to_np(p).mean()) <= 1.0


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_persistent_loop_equals_single_launches_bit_for_bit(hmc):
    n, d, N, M = 500, 25, 64, 6
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=N, seed=1, eps=0.1)
    c = pc.case(N, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(N, d).astype(np.float32)
    eps = pt.choose_eps(lambda e: pc.oracle_dynamics(g, c, hmc, e), x, v, lo=0.5)
    dyn = twin(g, fused(c), hmc, 10, eps)
    x0 = to_dev(x)
    xs, ps, hist = sample_chain(x0, dyn, M, seed=99, record=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_kernel<10, ")
    xc = x0
    for m in range(M):
        xc, p, _ = sample_chain(xc, dyn, 1, seed=99, proposal0=m)
        assert torch.equal(p[0], ps[m]) and torch.equal(xc, hist[m]), m
    assert torch.equal(xc, xs)
    assert 0.2 < float(ps.mean()) <= 1.0
    for variant in (16, 8, 32):                                    # the one-wave tile, LDS-resident-state and lane kernels
        dyn.variant = variant
        with pytest.raises(RuntimeError, match="probit-regression target runs on the general kernel only"):
            sample_chain(x0, dyn, 1, seed=99)


@pytest.mark.parametrize("hmc", [True, False])
def test_equal_rungs_are_the_scalar_path_bit_for_bit(hmc):
    n, d = 400, 12
    K, nl, R, M = 4, 32, 3, 2
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=K * nl, seed=2, eps=0.1)
    c = pc.case(K * nl, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(K * nl, d).astype(np.float32)
    eps = pt.choose_eps(lambda e: pc.oracle_dynamics(g, c, hmc, e, temperature=2.5), x, v)
    dyn = twin(g, fused(c), hmc, 10, eps, variant=100)
    x0 = to_dev(x)
    dyn.use_temperature, dyn.temperature = True, 2.5
    xs, ps, _ = sample_chain(x0, dyn, R * M, seed=11)
    dyn.use_temperature, dyn.temperature = False, 1.0
    ptm = ParallelTempering(dyn, [2.5] * K, nl, seed=11)
    out = ptm.run(x0, R, M, record_rungs=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_ladder_kernel<10, ")
    assert torch.equal(out["x"], xs) and torch.equal(out["p"], ps)
    assert torch.equal(out["swaps_accepted"], out["swaps_attempted"]) and int(out["swaps_attempted"].sum()) > 0
    assert float(ps.mean()) > 0.0


def test_temperature_and_anneal_bridge():
    n, d = 300, 8
    c = pc.case(33, n, d)
    W = c["W"]
    dyn = Dynamics(d, fused(c), T=5, eps=0.01, hmc=True)
    dyn.use_temperature, dyn.temperature = True, 2.5
    Ur, Gr, b = pc.scaled(c, temperature=2.5)
    sU, sg = pc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("T = 2.5: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0
    dyn.use_temperature, dyn.temperature = False, 1.0
    dyn.anneal_beta = 0.3
    Ur, Gr, b = pc.scaled(c, beta=0.3)
    sU, sg = pc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("beta = 0.3: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0


def test_warmup_adapts_the_step_size_on_the_fused_target():
    n, d, N, target = 300, 8, 256, 0.8
    c = pc.case(N, n, d)
    e = fused(c)

    def run():
        dyn = Dynamics(d, e, T=5, eps=1e-3, hmc=True)
        xw, info = warmup(to_dev(c["W"]), dyn, 60, target_accept=target, seed=4)
        return dyn, xw, info
    dyn, xw, info = run()
    assert _ffi.last_kernel().startswith("traj_kernel<10, ")
    assert np.isfinite(info.eps) and 0.0 < info.eps < 1e3 and np.float32(info.log_eps) == dyn.alpha.item()
    _, p, _ = sample_chain(xw, dyn, 40, seed=4, proposal0=info.next_proposal0)
    acc = float(p.double().mean())
    print("warm-up: eps %.5f, accept %.4f over 40 further proposals (%d search + %d averaging updates)" % (
        info.eps, acc, info.n_search, info.n_averaged))
    assert abs(acc - target) <= 0.1                                # (the Poisson and binomial tests' margin)
    dyn2, xw2, info2 = run()
    assert torch.equal(dyn2.alpha.view(torch.int32), dyn.alpha.view(torch.int32))
    assert torch.equal(xw2, xw) and torch.equal(info2.state.view(torch.int64), info.state.view(torch.int64))


def test_trainer_refuses_and_a_slow_path_state_dict_loads():
    from l2hmc_amd.training import Trainer
    n, d, N = 100, 5, 64
    c = pc.case(N, n, d)
    model = pc.model(c, prior_var=S2)
    assert isinstance(model, ProbitRegression)
    torch.manual_seed(0)
    slow = Dynamics(d, model.get_energy_function(), T=4, eps=0.01, net_factory=layers.stq_network(10))
    fast = Dynamics(d, model.get_energy_function(fused=True), T=4, eps=0.02, net_factory=layers.stq_network(10))
    with pytest.raises(NotImplementedError, match=r"train on the slow path.*get_energy_function\(\).*load_state_dict"):
        Trainer(fast)
    # the slow path is the same posterior: its torch energy and gradient against the fused ones, within the float32 bounds
    # (twice: both are float32 evaluations of the definition; torch's log_ndtr has its own few ulps)
    xd = to_dev(c["W"])
    Us, Gs = slow._fn.evaluate(xd, want_grad=True)
    Uf, Gf = fast._fn.evaluate(xd, want_grad=True)
    b = pc.bounds(c)
    assert np.all(np.abs(to_np(Us) - to_np(Uf)) <= 2 * b["U"] + 1e-6 * np.abs(to_np(Uf)))
    assert np.all(np.abs(to_np(Gs) - to_np(Gf)) <= 2 * b["g"] + 1e-5 * np.abs(to_np(Gf)).max())
    fast.load_state_dict(slow.state_dict())
    for (k, a), (k2, b2) in zip(slow.parameters(), fast.parameters()):
        assert k == k2 and torch.equal(a.detach(), b2.detach()), k
    xs, ps, _ = sample_chain(xd, fast, 3, seed=1)
    assert _ffi.last_kernel().startswith("traj_kernel<10, ")
    assert torch.isfinite(xs).all() and torch.isfinite(ps).all() and float(ps.mean()) > 0.0


# ---- the posterior ------------------------------------------------------------------------------------------------------------
def test_posterior_mean_matches_importance_sampling_and_the_history_feeds_loo():
    """The posterior mean of HMC chains on a (200, 5) model against self-normalised importance sampling from a wide Gaussian
    (`probit_case.wide_is_mean`): z-scores under 5 with the two Monte Carlo standard errors combined -- the chains' from the
    spread of the per-chain means, the importance sampler's from its own weights.  The same device history feeds `loo` and
    `waic`."""
    n, d, N, M = 200, 5, 4096, 200
    c = pc.case(4, n, d)
    ref_mean, ref_se, mode, Lc = pc.wide_is_mean(c)
    model = pc.model(c, prior_var=S2)
    # ten leapfrog steps across about two posterior standard deviations of the stiffest direction
    eps = 0.2 * float(np.sqrt(np.linalg.eigvalsh(Lc @ Lc.T).min()))
    dyn = Dynamics(d, model.get_energy_function(fused=True), T=10, eps=eps, hmc=True)
    dyn.eps_override = eps
    x0 = (mode + np.random.RandomState(3).randn(N, d) @ Lc.T).astype(np.float32)
    _, p, hist = sample_chain(to_dev(x0), dyn, M, seed=5, record=True)
    assert _ffi.last_kernel().startswith("traj_kernel<10, ")
    h = to_np(hist[M // 2:]).astype(np.float64)                   # (M / 2, N, d)
    per_chain = h.mean(axis=0)
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(N)
    z = np.abs(mean - ref_mean) / np.sqrt(np.square(se) + np.square(ref_se))
    print("posterior mean z-scores", z, "accept", float(p.mean()), "eps", eps, "se", se, "importance se", ref_se)
    assert float(p.mean()) > 0.5
    assert np.all(ref_se < 0.05 * np.sqrt(np.diag(Lc @ Lc.T)))    # (the reference resolves the mean to 1/20 of a posterior sd)
    assert np.all(z < 5.0), (mean, ref_mean, se)
    draws = hist[M - 8:]                                          # the same device history, read where it lies (32768 draws)
    s, w = model.loo(draws), model.waic(draws)
    print("elpd_loo %.2f  elpd_waic %.2f  p_loo %.2f  k-hat above 0.7: %d" % (s.elpd_loo, w.elpd_waic, s.p_loo, s.n_bad))
    assert np.isfinite(s.elpd_loo) and np.isfinite(w.elpd_waic) and np.all(np.isfinite(s.elpd_loo_i))
