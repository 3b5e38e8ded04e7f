"""GPU: `LogisticTrainer` -- the tile training kernel's logistic-regression form (`train_kernel<7>`) against the float64
oracle `training_loss_and_grad(g, np.float64, target=LogisticTarget(X, y, s2))` on identical injected draws; at a temperature;
against the same likelihood as a torch callable on the GEMM-engine trainer; bitwise reproducibility (two calls, two instruction
schedules); the sampler's proposal on the same draws; the checkpoint contract of `step`; the refusal beyond the LDS plan.

Gates: tests/logistic_train_case.py (the project's plain gates; a quantity's gate widens to 3 x the float32 numpy oracle's own
distance from the float64 one, never below the plain gate).  Every figure is printed before it is asserted."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from l2hmc_amd import Dynamics, LogisticRegression, LogisticTrainer, _ffi, layers, propose, sample_chain
from oracle import l2hmc_oracle as O
from tests import helpers
from tests import logistic_train_case as LC
from tests.helpers import abs_err, check_grads_per_tensor, net_grads, rel_err, to_dev, to_np

pytestmark = pytest.mark.gpu

KERNEL = "train_kernel<7>"


def _run(g, X, y, tau=None, rows=None):
    """one loss_and_grad call of a fresh LogisticTrainer on the first `rows` chains of the case"""
    if rows is not None:
        g = dict(g)
        for k in ("x", "z", "x.dir", "z.dir", "x.v_fwd", "x.v_bwd", "z.v_fwd", "z.v_bwd"):
            g[k] = g[k][:rows]
    dyn, tr = LC.hip_trainer(g, X, y, tau)
    loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=LC.draws_of(g))
    torch.cuda.synchronize()
    assert _ffi.last_kernel() == KERNEL, _ffi.last_kernel()
    return g, dyn, tr, loss, to_np(Lx), to_np(px)


# ---- 1. loss, Lx, px and every gradient tensor plus alpha against the float64 oracle -------------------------------------------
@pytest.mark.parametrize("n,d,eps,H", LC.CASES)
def test_gradient_matches_the_float64_oracle(n, d, eps, H):
    g, X, y = LC.make_case(n, d, eps, H)
    l64, r64, yard = LC.oracle_pair(g, X, y)
    _, dyn, tr, loss, Lx, px = _run(g, X, y)
    worst = LC.check_case("n=%d d=%d eps=%g H=%d" % (n, d, eps, H), loss, Lx, px, net_grads(dyn), l64, r64, yard)
    print("n=%d d=%d H=%d: worst ratio err / gate %.2f" % (n, d, H, worst))


def test_gradient_with_a_partial_last_tile():
    n, d, eps, H = 200, 25, 0.05, 10
    g, X, y = LC.make_case(n, d, eps, H)
    # a call launches the chains [x; z]: 20 + 20 = 40 chains end 8 rows into the third tile; 40 + 40 make the z rows start inside one
    g40, dyn, tr, loss, Lx, px = _run(g, X, y, rows=40)
    l64, r64, yard = LC.oracle_pair(g40, X, y)
    LC.check_case("n=200 d=25 40 chains", loss, Lx, px, net_grads(dyn), l64, r64, yard)
    g20, dyn, tr, loss, Lx, px = _run(g, X, y, rows=20)
    l64, r64, yard = LC.oracle_pair(g20, X, y)
    LC.check_case("n=200 d=25 20 chains", loss, Lx, px, net_grads(dyn), l64, r64, yard)


# ---- 2. at a temperature ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,eps,H", LC.CASES)
def test_tempered_gradient_matches_the_tempered_float64_oracle(n, d, eps, H):
    tau = 2.5
    g, X, y = LC.make_case(n, d, eps, H)
    l64, r64, yard = LC.oracle_pair(g, X, y, tau)
    _, dyn, tr, loss, Lx, px = _run(g, X, y, tau)
    got = net_grads(dyn)
    LC.check_case("n=%d d=%d H=%d tau=%g" % (n, d, H, tau), loss, Lx, px, got, l64, r64, yard)
    _, plain, _ = LC.oracle_pair(g, X, y)
    with pytest.raises(AssertionError):                              # the temperature really matters at this gate
        check_grads_per_tensor("untempered oracle", got, LC.grads_of(plain), yard=yard, yard_factor=3.0)


# ---- 3. two independent implementations: the same likelihood as a torch callable on the GEMM-engine trainer -------------------
@pytest.mark.parametrize("n,d,eps,H", [(17, 5, 0.1, 10), (200, 25, 0.05, 10)])
def test_fused_trainer_agrees_with_the_torch_callable_route(n, d, eps, H):
    from l2hmc_amd.training import SplitTrainer, Trainer
    g, X, y = LC.make_case(n, d, eps, H)
    l64, r64, yard = LC.oracle_pair(g, X, y)
    _, dyn, tr, loss, Lx, px = _run(g, X, y)
    Xd, yd = to_dev(X), to_dev(y)

    def fn(w):
        L = w @ Xd.t()
        return (torch.nn.functional.softplus(L) - yd * L).sum(1) + 0.5 * (w * w).sum(1) / LC.PRIOR_VAR
    cd = Dynamics(d, fn, T=int(g["T"]), eps=float(g["eps"]), net_factory=layers.stq_network(H))
    cd.mask = g["mask"]
    with torch.no_grad():
        cd.alpha.fill_(float(np.log(g["eps"])))
        for w, pre in ((cd._xw, "xnet."), (cd._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    tc = Trainer(cd)
    assert isinstance(tc, SplitTrainer) and tc.user
    lc, Lc, pc = tc.loss_and_grad(to_dev(g["x"]), draws=LC.draws_of(g))
    label = "n=%d d=%d fused vs torch callable" % (n, d)
    # the callable route against the oracle at the same gates, then the two against each other
    LC.check_case(label + " (callable vs oracle)", lc, to_np(Lc), to_np(pc), net_grads(cd), l64, r64, yard)
    worst = check_grads_per_tensor(label, net_grads(dyn), net_grads(cd), yard=yard, yard_factor=3.0)
    e_l, e_x, e_p = abs(float(loss) - float(lc)), rel_err(Lx, to_np(Lc)), abs_err(px, to_np(pc))
    print("%s: loss %.2e  Lx %.2e  px %.2e  worst tensor %s at %.2f of its gate" % (label, e_l, e_x, e_p, worst[1], worst[0]))
    assert e_l < max(1e-4 * max(1.0, abs(l64)), 3.0 * yard["loss"])
    assert e_x < max(1e-4, 3.0 * yard["Lx"]) and e_p < max(1e-4, 3.0 * yard["px"])


# ---- 4. bitwise reproducibility ----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_at_4096_chains():
    n, d, eps, H = 1000, 25, 0.02, 10
    g, X, y = LC.make_case(n, d, eps, H, N=4096)
    dyn, tr = LC.hip_trainer(g, X, y)
    l1, Lx1, px1 = tr.loss_and_grad(to_dev(g["x"]), draws=LC.draws_of(g))
    flat1 = tr.flat.clone()
    assert _ffi.last_kernel() == KERNEL
    l2, Lx2, px2 = tr.loss_and_grad(to_dev(g["x"]), draws=LC.draws_of(g))
    assert torch.equal(flat1, tr.flat) and torch.equal(Lx1, Lx2) and torch.equal(px1, px2) and float(l1) == float(l2)
    assert bool(torch.isfinite(flat1).all()) and float(flat1.abs().max()) > 0.0


def test_gradient_does_not_depend_on_the_instruction_schedule():
    """tests/test_gpu_round5.py's guard for the new kernel: the flat gradient, proposals and accept probabilities of one call from
    the default build and from the max-ILP build of the training unit are equal bit for bit."""
    ilp = os.path.join(helpers.ROOT, "l2hmc_amd", "csrc", "variants", "libl2hmc_hip_train_ilp.so")
    assert os.path.exists(ilp), "run `make -C l2hmc_amd/csrc variants` (builds the second schedule of train.hip)"
    with tempfile.TemporaryDirectory() as td:
        outs = []
        for tag, lib in (("default", None), ("ilp", ilp)):
            env = dict(os.environ)
            env.pop("L2HMC_DBG_LIB", None)
            if lib:
                env["L2HMC_DBG_LIB"] = lib
            out = os.path.join(td, tag + ".npz")
            r = subprocess.run([sys.executable, "-m", "tests.logistic_train_case", out, "300", "50", "0.03", "10", "48"],
                               cwd=helpers.ROOT, env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(np.load(out))
        a, b = outs
        assert str(a["kernel"]) == str(b["kernel"]) == KERNEL
        for k in ("flat", "Lx", "px"):
            assert a[k].size > 0 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert np.all(np.isfinite(a["flat"])) and float(a["loss"]) == float(b["loss"])


# ---- 5. the trainer's proposal is the sampler's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,eps,H,tau", [(200, 25, 0.05, 10, None), (1000, 25, 0.02, 10, None), (300, 50, 0.03, 10, 2.5)])
def test_trainer_proposal_agrees_with_the_sampler(n, d, eps, H, tau):
    g, X, y = LC.make_case(n, d, eps, H)
    _, dyn, tr, loss, Lx, px = _run(g, X, y, tau)
    dr = LC.draws_of(g)
    with torch.no_grad():
        sLx, _, spx, _ = propose(to_dev(g["x"]), dyn, direction=to_dev(g["x.dir"]), v=to_dev(dr["x_v"]))
    assert _ffi.last_kernel().startswith("traj_kernel<7, "), _ffi.last_kernel()
    e_x, e_p = rel_err(Lx, to_np(sLx)), abs_err(px, to_np(spx))
    print("n=%d d=%d tau=%s: trainer vs sampler  Lx %.2e  px %.2e" % (n, d, tau, e_x, e_p))
    assert e_x < 3e-5 and e_p < 1e-4


# ---- 6. step: the checkpoint contract, and a run that stays finite ---------------------------------------------------------------
def _fresh(seed_np, X, y, d):
    np.random.seed(seed_np)                  # masks come from numpy's global RNG like the reference's
    torch.manual_seed(seed_np)
    e = LogisticRegression(X, y, prior_var=LC.PRIOR_VAR).get_energy_function()
    dyn = Dynamics(d, e, T=10, eps=0.05, net_factory=layers.stq_network(10))
    return dyn, LogisticTrainer(dyn, seed=5)


def test_step_resumes_from_a_checkpoint_bit_for_bit():
    n, d = 200, 25
    X, y = LC.blr_data(n, d)
    x0 = (0.5 * torch.randn(256, d, generator=torch.Generator().manual_seed(1))).cuda()
    dyn_a, tr_a = _fresh(0, X, y, d)
    xs = x0.clone()
    for _ in range(50):
        _, _, xs, _ = tr_a.step(xs)
    assert _ffi.last_kernel() == KERNEL
    dyn_b, tr_b = _fresh(0, X, y, d)
    xb = x0.clone()
    for _ in range(25):
        _, _, xb, _ = tr_b.step(xb)
    buf = io.BytesIO()
    torch.save({"trainer": tr_b.state_dict(), "x": xb.cpu()}, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    dyn_c, tr_c = _fresh(123, X, y, d)       # different initial weights AND masks: everything must come from the file
    tr_c.load_state_dict(ck["trainer"])
    xc = ck["x"].cuda()
    for _ in range(25):
        _, _, xc, _ = tr_c.step(xc)
    assert torch.equal(tr_c.theta, tr_a.theta) and torch.equal(tr_c.m, tr_a.m) and torch.equal(tr_c.v, tr_a.v)
    assert torch.equal(xc, xs) and tr_c.global_step == 50 and torch.equal(dyn_c.mask, dyn_a.mask)
    assert not torch.equal(tr_a.theta, tr_b.theta)                  # (the second 25 steps moved the parameters)
    # the trained nets are the Dynamics' own: it samples as it is
    xf, ps = sample_chain(xs, dyn_a, 5, seed=3)[:2]
    assert _ffi.last_kernel().startswith("traj_kernel<7, ") and bool(torch.isfinite(xf).all()) and 0.0 < float(ps.mean()) <= 1.0


def test_a_200_step_run_keeps_a_finite_loss():
    n, d = 200, 25
    X, y = LC.blr_data(n, d)
    dyn, tr = _fresh(1, X, y, d)
    x = (0.5 * torch.randn(256, d, generator=torch.Generator().manual_seed(2))).cuda()
    losses = []
    for _ in range(200):
        loss, px, x, _ = tr.step(x)
        losses.append(loss)
    losses = torch.stack(losses).cpu().numpy()
    print("200 steps on (200, 25): loss %.4g -> %.4g, last mean accept %.3f" % (losses[0], losses[-1], float(px.mean())))
    assert np.all(np.isfinite(losses)) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(tr.theta).all())


# ---- 7. beyond the plan --------------------------------------------------------------------------------------------------------
def test_a_shape_beyond_the_plan_is_refused_and_nothing_is_launched():
    d = 128
    X, y = LC.blr_data(64, d)
    e = LogisticRegression(X, y, prior_var=LC.PRIOR_VAR).get_energy_function()
    dyn = Dynamics(d, e, T=10, eps=0.05, net_factory=layers.stq_network(10))
    x = to_dev((0.1 * np.random.RandomState(0).randn(16, d)).astype(np.float32))
    sample_chain(x, dyn, 1, seed=1)                                  # (the sampler holds this shape)
    before = _ffi.last_kernel()
    assert before.startswith("traj_kernel<7, ")
    with pytest.raises(NotImplementedError, match="torch callable") as ei:
        LogisticTrainer(dyn)
    msg = str(ei.value)
    need = _ffi.lib().l2hmc_train_logistic_lds_bytes(64, d, 10, 10)
    assert need == -2
    assert "d = 128" in msg and "H = 10" in msg and "bytes of LDS" in msg and "state_dict" in msg
    assert _ffi.last_kernel() == before                             # nothing was launched
    # ... and the C entry refuses the same shape by itself (a Trainer built around the guard)
    from l2hmc_amd.training import Trainer
    tr = object.__new__(LogisticTrainer)
    Trainer.__init__(tr, dyn)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        tr.loss_and_grad(x)
    assert _ffi.last_kernel() == before
