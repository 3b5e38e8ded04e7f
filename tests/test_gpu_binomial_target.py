"""GPU: binomial and negative-binomial regression on the fused trajectory kernels (L2HMC_ENERGY_BINOMIAL), mirroring
tests/test_gpu_poisson_target.py.  U and grad U within the bounds of tests/binomial_case.py on the LDS-staged and the streamed
data path; kind 9 with one trial and no offsets against kind 7; rows at |t| = 100; trajectories against the float32 oracle (HMC,
fused nets, nets on the GEMM engine) at tolerances computed from the oracle alone; the persistent loop against single launches
bit for bit; equal ladder rungs against the scalar path bit for bit; temperature and the AIS bridge; warm-up; the posterior
mean of HMC chains against float64 importance sampling, with the model's own LOO and WAIC on that history; the training refusal
and the state_dict route."""
import numpy as np
import pytest
import torch

from l2hmc_amd import BinomialRegression, Dynamics, LogisticRegression, ParallelTempering, _ffi, layers, sample_chain, warmup
from oracle import l2hmc_oracle as O
from tests import binomial_case as bc
from tests import poisson_target_case as pc
from tests.helpers import to_dev, to_np

pytestmark = pytest.mark.gpu

S2 = bc.PRIOR_VAR


def fused(c):
    return bc.model(c, prior_var=S2).get_energy_function(fused=True)


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
    Ur, Gr = bc.energy(c)
    b = bc.bounds(c)
    out = {}
    for mode in ("planned", "streamed"):
        if mode == "streamed":
            monkeypatch.setenv("L2HMC_LOGISTIC_LDS", "0")
        U, G = fused(c).evaluate(to_dev(c["W"]), want_grad=True)
        U, G = to_np(U), to_np(G)
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(G))
        sU, sg = bc.used(U, G, Ur, Gr, b)
        print("%s %s: uses %.3f of the U bound, %.3f of the grad U bound" % (what, mode, sU, sg))
        assert sU <= 1.0 and sg <= 1.0, (what, mode, sU, sg)
        out[mode] = (U, G)
    return out


# ---- 5. U and grad U --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 1000])
@pytest.mark.parametrize("d", [2, 25, 50, 128])
def test_binomial_energy_and_gradient_within_the_bounds(n, d, monkeypatch):
    # 40 chains: the last tile is partial.  n = 17: one live row in the second block -- its 15 padded rows carry weight 0
    # and are masked besides; trials mix 1, small and 50 with rows at y = 0 and y = m
    _both_paths(bc.case(40, n, d), monkeypatch, "binomial n=%d d=%d" % (n, d))


# d = 40, 65, 96: 3, 5 and 6 live feature tiles -- 3 of the 4 compiled ones of one state tile per wave, 5 and 6 of the 8 of two
# (the plan goes from one to two state tiles per wave between 4 and 5); above, d = 2 .. 128 has 1, 2, 4 and 8
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("d", [40, 65, 96])
def test_binomial_energy_and_gradient_within_the_bounds_at_partly_live_tile_counts(n, d, monkeypatch):
    _both_paths(bc.case(40, n, d), monkeypatch, "binomial n=%d d=%d" % (n, d))


@pytest.mark.parametrize("phi", bc.NB_PHIS)
@pytest.mark.parametrize("n,d", [(1000, 25), (17, 128), (17, 65)])
def test_negative_binomial_energy_and_gradient_within_the_bounds(n, d, phi, monkeypatch):
    _both_paths(bc.case(40, n, d, "negbinomial", phi), monkeypatch, "negbinomial phi=%g n=%d d=%d" % (phi, n, d))


@pytest.mark.parametrize("n,d", [(17, 5), (1000, 25)])
def test_one_trial_without_offsets_is_kind_7(n, d):
    """Kind 9 with trials = 1 and zero offsets against kind 7 on the same data: within the sum of their two bounds.  Kind 7's
    link forms e, the reciprocal and softplus by kind 9's expressions (compiled with the default contraction, which only
    removes roundings), so the bound of tests/binomial_case.py at m = 1, o = 0 bounds it too: the sum is twice that bound.  A
    weight or an offset read from the wrong slot (the 16 offsets and 16 weights of a block lie side by side) shows here."""
    c = bc.case(40, n, d)
    y = (c["y"] > 0.5 * c["trials"]).astype(np.float32)
    c = dict(c, y=y, trials=np.ones(n, dtype=np.float32), offset=np.zeros(n, dtype=np.float32))
    U9, G9 = fused(c).evaluate(to_dev(c["W"]), want_grad=True)
    U7, G7 = LogisticRegression(c["X"], y, prior_var=S2).get_energy_function().evaluate(to_dev(c["W"]), want_grad=True)
    assert _ffi.ENERGY_BINOMIAL == 9
    b = bc.bounds(c)
    dU, dG = np.abs(to_np(U9).astype(np.float64) - to_np(U7)), np.abs(to_np(G9).astype(np.float64) - to_np(G7))
    print("n=%d d=%d: |U9 - U7| / (2 bound) %.3g, |g9 - g7| / (2 bound) %.3g" % (n, d, np.max(dU / (2 * b["U"])), np.max(dG / (2 * b["g"]))))
    assert np.all(dU <= 2 * b["U"]) and np.all(dG <= 2 * b["g"])
    Ur, Gr = bc.energy(c)
    assert max(bc.used(to_np(U9), to_np(G9), Ur, Gr, b)) <= 1.0


def test_rows_at_a_linear_predictor_of_100(monkeypatch):
    """One row block with |t| = 100: softplus is t or e^-100, sigmoid 1 or 0; U and the residual (through grad U) are finite
    and within the bound."""
    _both_paths(bc.far_case(), monkeypatch, "|t| = 100")


# ---- 6. trajectories against the float32 oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,H", bc.TRAJ_CASES)
def test_trajectories_match_the_oracle(n, d, H):
    t = bc.traj_case(n, d, H)
    hmc, r, dist = t["hmc"], t["ref"], t["dist"]
    dyn = twin(t["g"], fused(t["c"]), hmc, max(H, 1), t["eps"])
    if H == 24:
        assert dyn._split                                          # nets wider than H = 15: the GEMM engine, grad U from l2hmc_energy
    xd, vd = to_dev(t["x"]), to_dev(t["v"])
    print("n=%d d=%d H=%d eps=%g oracle accept %.3f" % (n, d, H, t["eps"], float(r["forward"][3].mean())))
    for s in (0, 3):
        for key, got in (("fwd%d" % s, dyn._forward_step(xd, vd, s)), ("bwd%d" % s, dyn._backward_step(xd, vd, s))):
            errs = tuple(pc.rel_err(to_np(got[i]), r[key][i]) for i in range(3))
            tols = (pc.gate(pc.STATE_GATE, dist[key][0]), pc.gate(pc.STATE_GATE, dist[key][1]), pc.gate(pc.SCALAR_GATE, dist[key][2]))
            print("  %s: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (key, errs, dist[key], tols))
            assert all(e < tl for e, tl in zip(errs, tols)), (n, d, H, key, errs, tols)
    if not dyn._split:
        assert _ffi.last_kernel().startswith("traj_kernel<9, ")
    X1, V1, lj = dyn.forward(xd, init_v=vd, log_jac=True)
    _, _, p = dyn.forward(xd, init_v=vd)
    rX, rV, rlj, rp = r["forward"]
    errs = (pc.rel_err(to_np(X1), rX), pc.rel_err(to_np(V1), rV), pc.rel_err(to_np(lj), rlj), pc.abs_err(to_np(p), rp))
    tols = tuple(pc.gate(b, dd) for b, dd in zip((pc.STATE_GATE, pc.STATE_GATE, pc.SCALAR_GATE, pc.SCALAR_GATE), dist["forward"]))
    print("  forward: kernel-oracle %s, float32-float64 oracle %s, gates %s" % (errs, dist["forward"], tols))
    assert all(e < tl for e, tl in zip(errs, tols)), (n, d, H, errs, tols)
    assert 0.0 < float(to_np(p).mean()) <= 1.0


# ---- 7. plumbing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_persistent_loop_equals_single_launches_bit_for_bit(hmc):
    n, d, N, M = 500, 25, 64, 6
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=N, seed=1, eps=0.1)
    c = bc.case(N, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(N, d).astype(np.float32)
    # (half of the first proposal accepted: the loop's own draws and the states it reaches stay above the 0.2 asserted below)
    eps = pc.choose_eps(lambda e: bc.oracle_dynamics(g, c, hmc, e), x, v, lo=0.5)
    dyn = twin(g, fused(c), hmc, 10, eps)
    x0 = to_dev(x)
    xs, ps, hist = sample_chain(x0, dyn, M, seed=99, record=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_kernel<9, ")           # (`sample_chain` reports the kind-9 general kernel)
    xc = x0
    for m in range(M):
        xc, p, _ = sample_chain(xc, dyn, 1, seed=99, proposal0=m)
        assert torch.equal(p[0], ps[m]) and torch.equal(xc, hist[m]), m
    assert torch.equal(xc, xs)
    assert 0.2 < float(ps.mean()) <= 1.0
    for variant in (16, 8, 32):                                    # the one-wave tile, LDS-resident-state and lane kernels
        dyn.variant = variant
        with pytest.raises(RuntimeError, match="binomial-regression target runs on the general kernel only"):
            sample_chain(x0, dyn, 1, seed=99)


@pytest.mark.parametrize("hmc", [True, False])
def test_equal_rungs_are_the_scalar_path_bit_for_bit(hmc):
    n, d = 400, 12
    K, nl, R, M = 4, 32, 3, 2
    from tests import helpers
    g = helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=K * nl, seed=2, eps=0.1)
    c = bc.case(K * nl, n, d)
    x = c["W"]
    v = np.random.RandomState(3).randn(K * nl, d).astype(np.float32)
    eps = pc.choose_eps(lambda e: bc.oracle_dynamics(g, c, hmc, e, temperature=2.5), x, v)
    dyn = twin(g, fused(c), hmc, 10, eps, variant=100)
    x0 = to_dev(x)
    dyn.use_temperature, dyn.temperature = True, 2.5
    xs, ps, _ = sample_chain(x0, dyn, R * M, seed=11)
    dyn.use_temperature, dyn.temperature = False, 1.0
    pt = ParallelTempering(dyn, [2.5] * K, nl, seed=11)
    out = pt.run(x0, R, M, record_rungs=True)
    torch.cuda.synchronize()
    assert _ffi.last_kernel().startswith("traj_ladder_kernel<9, ")
    assert torch.equal(out["x"], xs) and torch.equal(out["p"], ps)
    assert torch.equal(out["swaps_accepted"], out["swaps_attempted"]) and int(out["swaps_attempted"].sum()) > 0
    assert float(ps.mean()) > 0.0


@pytest.mark.parametrize("kind,phi", [("binomial", None), ("negbinomial", 0.5)])
def test_temperature_and_anneal_bridge(kind, phi):
    n, d = 300, 8
    c = bc.case(33, n, d, kind, phi)
    W = c["W"]
    dyn = Dynamics(d, fused(c), T=5, eps=0.01, hmc=True)
    dyn.use_temperature, dyn.temperature = True, 2.5
    Ur, Gr, b = bc.scaled(c, temperature=2.5)
    sU, sg = bc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("T = 2.5: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0
    dyn.use_temperature, dyn.temperature = False, 1.0
    dyn.anneal_beta = 0.3
    Ur, Gr, b = bc.scaled(c, beta=0.3)
    sU, sg = bc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
    print("beta = 0.3: uses %.3f of the U bound, %.3f of the grad U bound" % (sU, sg))
    assert sU <= 1.0 and sg <= 1.0


def test_warmup_adapts_the_step_size_on_the_fused_target():
    n, d, N, target = 300, 8, 256, 0.8
    c = bc.case(N, n, d)
    e = fused(c)

    def run():
        dyn = Dynamics(d, e, T=5, eps=1e-3, hmc=True)
        xw, info = warmup(to_dev(c["W"]), dyn, 60, target_accept=target, seed=4)
        return dyn, xw, info
    dyn, xw, info = run()
    assert _ffi.last_kernel().startswith("traj_kernel<9, ")
    assert np.isfinite(info.eps) and 0.0 < info.eps < 1e3 and np.float32(info.log_eps) == dyn.alpha.item()
    _, p, _ = sample_chain(xw, dyn, 40, seed=4, proposal0=info.next_proposal0)
    acc = float(p.double().mean())
    print("warm-up: eps %.5f, accept %.4f over 40 further proposals (%d search + %d averaging updates)" % (
        info.eps, acc, info.n_search, info.n_averaged))
    assert abs(acc - target) <= 0.1                                # (the Poisson test's margin)
    dyn2, xw2, info2 = run()
    assert torch.equal(dyn2.alpha.view(torch.int32), dyn.alpha.view(torch.int32))
    assert torch.equal(xw2, xw) and torch.equal(info2.state.view(torch.int64), info.state.view(torch.int64))


def test_trainer_refuses_and_a_slow_path_state_dict_loads():
    from l2hmc_amd.training import Trainer
    n, d, N = 100, 5, 64
    c = bc.case(N, n, d)
    model = bc.model(c, prior_var=S2)
    assert isinstance(model, BinomialRegression)
    torch.manual_seed(0)
    slow = Dynamics(d, model.get_energy_function(), T=4, eps=0.01, net_factory=layers.stq_network(10))
    fast = Dynamics(d, model.get_energy_function(fused=True), T=4, eps=0.02, net_factory=layers.stq_network(10))
    with pytest.raises(NotImplementedError, match=r"train on the slow path.*get_energy_function\(\).*load_state_dict"):
        Trainer(fast)
    # the slow path is the same posterior: its torch energy against the fused one, within the float32 bounds (twice: both
    # are float32 evaluations of the definition)
    xd = to_dev(c["W"])
    Us, _ = slow._fn.evaluate(xd)
    Uf, _ = fast._fn.evaluate(xd)
    assert np.all(np.abs(to_np(Us) - to_np(Uf)) <= 2 * bc.bounds(c)["U"] + 1e-6 * np.abs(to_np(Uf)))
    fast.load_state_dict(slow.state_dict())
    for (k, a), (k2, b) in zip(slow.parameters(), fast.parameters()):
        assert k == k2 and torch.equal(a.detach(), b.detach()), k
    xs, ps, _ = sample_chain(xd, fast, 3, seed=1)
    assert _ffi.last_kernel().startswith("traj_kernel<9, ")
    assert torch.isfinite(xs).all() and torch.isfinite(ps).all() and float(ps.mean()) > 0.0


# ---- 8. the posterior ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,phi", [("binomial", None), ("negbinomial", 0.5)])
def test_posterior_mean_matches_importance_sampling_and_the_history_feeds_loo(kind, phi):
    n, d, N, M = 100, 5, 4096, 200
    c = bc.case(4, n, d, kind, phi)
    ref_mean, ref_se, mode, Lc = bc.laplace_is_mean(c)
    model = bc.model(c, prior_var=S2)
    # ten leapfrog steps across about two posterior standard deviations of the stiffest direction
    eps = 0.2 * float(np.sqrt(np.linalg.eigvalsh(Lc @ Lc.T).min()))
    dyn = Dynamics(d, model.get_energy_function(fused=True), T=10, eps=eps, hmc=True)
    dyn.eps_override = eps
    x0 = (mode + np.random.RandomState(3).randn(N, d) @ Lc.T).astype(np.float32)
    _, p, hist = sample_chain(to_dev(x0), dyn, M, seed=5, record=True)
    assert _ffi.last_kernel().startswith("traj_kernel<9, ")
    h = to_np(hist[M // 2:]).astype(np.float64)                   # (M / 2, N, d)
    per_chain = h.mean(axis=0)
    mean, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(N)
    z = np.abs(mean - ref_mean) / np.sqrt(np.square(se) + np.square(ref_se))
    print("posterior mean z-scores", z, "accept", float(p.mean()), "eps", eps)
    assert float(p.mean()) > 0.5
    assert np.all(z < 5.0), (mean, ref_mean, se)
    draws = hist[M - 8:]                                          # the same device history, read where it lies (32768 draws)
    s, w = model.loo(draws), model.waic(draws)
    print("elpd_loo %.2f  elpd_waic %.2f  p_loo %.2f  k-hat above 0.7: %d" % (s.elpd_loo, w.elpd_waic, s.p_loo, s.n_bad))
    assert np.isfinite(s.elpd_loo) and np.isfinite(w.elpd_waic) and np.all(np.isfinite(s.elpd_loo_i))
