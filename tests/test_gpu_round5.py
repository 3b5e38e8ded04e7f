"""GPU tests added in round 5: the reference's DEFAULT Rough Well (distributions.py:84-97 with `easy=False`: cos(x / eps^2))
at eta = 1e-2 -- the form BASELINE config 4's second series is timed on -- through every kernel family.

What can and cannot be compared there.  The target's curvature is eta^-3 = 1e6: an error dx in a position comes back as
1e6 dx through grad U.  At the step sizes the bench's pilot tunes (7.8e-3 / 1.7e-3 / 3.6e-4 for d = 2 / 50 / 512) eps sqrt(1e6)
is 7.8 / 1.7 / 0.36 -- beyond the leapfrog stability limit for the first two -- so a T = 10 trajectory amplifies one ulp of x to
O(1): the float32 numpy oracle and the reference's own float32 run of the SAME op sequence disagree by 0.14 in x and 1.0 in
the accept probability there (measured, oracle/make_goldens.py `rough_ne_cases`).  No implementation -- the reference on another
machine included -- reproduces such a trajectory; what IS well defined, and what these tests pin:
  * grad U itself, recovered from each kernel family to float32 rounding (`test_gradient_probe_...`);
  * the reference-run fixtures rough{2,50,512}_ne at eps = 3e-4 (stable regime), through the generic tests of
    tests/test_gpu_parity.py at `stiff_tol` gates;
  * at the bench's own step sizes and full chain count: every ONE step the kernel takes, checked against the oracle's step
    from the kernel's own state (local parity along the kernel's trajectory), the T-fused launch bit-equal to that chain of
    one-step launches, and the accept probability consistent with the oracle's Hamiltonians at the kernel's own end points
    (`test_config4_default_rough_well_walk_at_full_chain_count`)."""
import numpy as np
import pytest

from oracle import l2hmc_oracle as O
from tests.helpers import (abs_err, hip_dynamics, load, oracle_dynamics, rel_err, stiffness, synthetic_case, to_dev, to_np)

pytestmark = pytest.mark.gpu

STEP_TOL, P_TOL = 3e-5, 1e-4


def _p_accept64(g, x0, v0, x1, v1, logjac):
    """dynamics.py:302-309 with the Rough Well's float32 arguments (the quotient x / den rounded to float32, as the reference
    and the kernels form it) but cosines and sums in float64: the accept probability a float32 implementation is allowed to
    miss only by its own summation rounding (H ~ d: 6e-5 per Hamiltonian at d = 512)."""
    from tests.helpers import rough_eta
    eta = rough_eta(g)
    den = np.float32(eta if bool(g["energy.easy"]) else eta * eta)

    def H(x, v):
        x, v = np.asarray(x, np.float32), np.asarray(v, np.float64)
        arg = (x / den).astype(np.float64)
        return 0.5 * np.sum(x.astype(np.float64) ** 2, 1) + np.float64(np.float32(eta)) * np.sum(np.cos(arg), 1) + 0.5 * np.sum(v * v, 1)
    with np.errstate(all="ignore"):
        val = H(x0, v0) - H(x1, v1) + np.asarray(logjac, np.float64)
        p = np.exp(np.minimum(val, 0.0))
    return np.where(np.isfinite(p), p, 0.0)


def _check_p(p, pref, d):
    """1e-4 (north_star) everywhere up to d = 64; wider states sum ~d/2-sized Hamiltonians in float32 (ulp 3e-5 at 512): 99 % of
    the chains within 1e-4, all within 3e-4."""
    e = np.abs(np.asarray(p, np.float64) - pref)
    if d <= 64:
        assert e.max() < P_TOL, float(e.max())
    else:
        assert np.quantile(e, 0.99) < P_TOL and e.max() < 3 * P_TOL, (float(np.quantile(e, 0.99)), float(e.max()))


def _zero_nets(g):
    g = dict(g)
    for net in ("xnet", "vnet"):
        for k in O.NET_KEYS:
            g[net + "." + k] = np.zeros_like(g[net + "." + k])
    return g


@pytest.mark.parametrize("d,variant", [(2, 0), (2, 100), (2, 32), (8, 0), (8, 100), (50, 1), (50, 4), (50, 16), (50, 104),
                                       (200, 0), (200, 8), (512, 0), (512, 4), (512, 104)])
def test_gradient_probe_of_the_default_rough_well_on_every_kernel_family(d, variant):
    """grad U of cos(x / eta^2), eta = 1e-2, as each trajectory kernel family computes it (each forms its own divisor and its
    own sin / cos: the Cody-Waite fast path below |arg| = 8192 pi/2, ocml's above, the switch wave-uniform).  With all net
    weights zero (S = T = Q = 0), v = 0 and eps = 1 one forward step is x' = x - grad U(x) / 2 exactly (dynamics.py:121-145), so
    grad U = 2 (x - x') to the rounding of x' (|x'| <= 54: 4e-6).  Chains 0..15 sit inside |x| < 1.25 (a whole tile below the
    switch), the next 16 straddle it, the rest are N(0, 1); the oracle's gradient is the fixture-pinned one (2e-7 of the
    reference's, tests/test_oracle_golden.py).  A wrong quadrant, divisor or branch is an error of O(100) here; the gate is
    3e-5 + 1e-6 |g|.  The accept probability of the same launch (nets zero: logdet = 0) is checked against the oracle's
    Hamiltonians at the kernel's own end point: that is each family's U (its cos)."""
    N = 64
    g = _zero_nets(synthetic_case("roughwell_ne", d, H=10, T=4, N=N, seed=500 + d, eps=1.0))
    x = g["x"].copy()
    x[:16] = np.clip(0.3 * x[:16], -1.25, 1.25)
    x[16:32] = np.clip(x[16:32], -1.35, 1.35) * 1.0
    x[16:32, 0] = 1.30                                  # |arg| = 13 000 > 12 867: this tile takes the ocml branch
    g["x"], g["v"] = x.astype(np.float32), np.zeros((N, d), np.float32)
    dyn = hip_dynamics(g, variant)
    od = oracle_dynamics(g)
    o = dyn.run(to_dev(g["x"]), to_dev(g["v"]), 0, 1, direction_all=1, want=("x", "v", "logjac"))
    xo, vo = to_np(o["x"]), to_np(o["v"])
    gref = od.grad_energy(g["x"])
    got = 2.0 * (g["x"].astype(np.float64) - xo.astype(np.float64))
    err = np.abs(got - gref) / (3e-5 + 1e-6 * np.abs(gref))
    assert err.max() < 1.0, (d, variant, float(np.abs(got - gref).max()))
    assert float(np.abs(to_np(o["logjac"])).max()) == 0.0
    # v' = -g(x)/2 - g(x')/2: the second gradient, at the kernel's own x' (|x'| ~ 50: arguments 5e5, ocml's branch)
    g2 = od.grad_energy(xo)
    assert np.abs(vo - (-0.5 * gref - 0.5 * g2)).max() < 1e-4, (d, variant)
    # U: a second launch that moves every argument by about a radian (eps = 1e-4, v ~ N(0, 1)): H0 - H1 is then made of the
    # cosine sums (0.01 per flipped dimension, 100x the gate) and the kinetic change; backward chains too
    dyn.eps_override = 1e-4
    v = np.random.RandomState(d).randn(N, d).astype(np.float32)
    direction = (np.arange(N) % 2).astype(np.uint8)
    o = dyn.run(to_dev(g["x"]), to_dev(v), 0, 1, direction=to_dev(direction), want=("x", "v", "logjac", "p"))
    p = to_np(o["p"])
    _check_p(p, _p_accept64(g, g["x"], v, to_np(o["x"]), to_np(o["v"]), np.zeros(N)), d)
    assert p.min() < 0.999 and p.max() > 0.5


@pytest.mark.parametrize("d,eps", [(2, 7.776e-3), (50, 1.68e-3), (512, 3.63e-4)])
def test_config4_default_rough_well_walk_at_full_chain_count(d, eps):
    """BASELINE.json config 4, second series, as the bench runs it: Rough Well eta = 1e-2 (non-easy), 16 384 chains, Lf = 10,
    the AUTOMATIC kernel choice, the step size bench.py's pilot settles on (profiles/r04_bench_steps20.json).  See the module
    docstring: the T-step map is chaotic at these step sizes, so the check is local --
      (i)   the fused T-step launch equals the chain of T one-step launches BIT FOR BIT (positions, momenta, log-Jacobian);
      (ii)  each of those one-step launches agrees with the float32 oracle's step FROM THE KERNEL'S OWN STATE: positions to
            3e-5 (the suite's single-step gate); momenta and log-det to the conditioning of one step,
            eps/2 * eta^-3 * (4 ulp of max|x|) relative to max(1, |v|) -- the last half-update reads grad U at the new x';
      (iii) the accept probability equals exp(min(H0 - H1 + logjac, 0)) at the kernel's own end point (`_check_p`)."""
    import torch
    from l2hmc_amd import _ffi
    N, T = 16384, 10
    g = synthetic_case("roughwell_ne", d, H=10, T=T, N=N, seed=600 + d, eps=eps, head_std=0.03)
    dyn = hip_dynamics(g, 0)
    od = oracle_dynamics(g)
    rng = np.random.RandomState(3)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    x0, v0, dr = to_dev(g["x"]), to_dev(g["v"]), to_dev(direction)
    fused = dyn.run(x0, v0, 0, T, direction=dr, want=("x", "v", "logjac", "p"))
    kernel = _ffi.last_kernel()
    kappa = stiffness(g)
    v_tol = max(STEP_TOL, 0.5 * eps * kappa * 4 * 2.0 ** -23 * float(np.abs(g["x"]).max() + 1.0))
    x, v = x0, v0
    lj = torch.zeros(N, device="cuda")
    worst = {"x": 0.0, "v": 0.0, "lj": 0.0}
    fwd = direction != 0
    for t in range(T):
        o = dyn.run(x, v, t, 1, direction=dr, want=("x", "v", "logjac"))
        xn, vn = to_np(x), to_np(v)
        with np.errstate(all="ignore"):
            fx, fv, fl = od.forward_step(xn, vn, np.float32(t))
            bx, bv, bl = od.backward_step(xn, vn, np.float32(T - 1 - t))
        rx, rv, rl = np.where(fwd[:, None], fx, bx), np.where(fwd[:, None], fv, bv), np.where(fwd, fl, bl)
        worst["x"] = max(worst["x"], rel_err(to_np(o["x"]), rx))
        worst["v"] = max(worst["v"], rel_err(to_np(o["v"]), rv))
        worst["lj"] = max(worst["lj"], rel_err(to_np(o["logjac"]), rl))
        x, v, lj = o["x"], o["v"], lj + o["logjac"]
    print("default rough well d=%d eps=%.3g %s: one-step err x %.1e v %.1e logdet %.1e (gates %.0e / %.1e); mean p %.3f"
          % (d, eps, kernel, worst["x"], worst["v"], worst["lj"], STEP_TOL, v_tol, float(fused["p"].mean())))
    assert worst["x"] < STEP_TOL and worst["v"] < v_tol and worst["lj"] < v_tol
    assert torch.equal(fused["x"], x) and torch.equal(fused["v"], v), "fused launch != chain of one-step launches"
    assert rel_err(to_np(fused["logjac"]), to_np(lj)) < 1e-5         # (summation order: T partial sums on the host here)
    _check_p(to_np(fused["p"]), _p_accept64(g, g["x"], g["v"], to_np(fused["x"]), to_np(fused["v"]), to_np(fused["logjac"])), d)
    assert 0.02 < float(fused["p"].mean()) < 0.98


@pytest.mark.parametrize("d,variant", [(200, 0), (200, 8), (512, 0)])
def test_wide_dims_default_rough_well_against_oracle(d, variant):
    """test_wide_dims_against_oracle's check for the non-easy form in the stable regime (eps = 3e-4: eps sqrt(curvature) = 0.3):
    direction-mixed proposal against the float32 oracle.  Gates: positions 1e-4; accept probability and momenta at the
    conditioning the reference-run fixture of the same shape shows (rough512_ne: the oracle itself is 2.2e-3 / 2.5e-3 from the
    reference) -- 1e-2; one step: positions 3e-5, momenta eps/2 * 1e6 * 4 ulp."""
    from l2hmc_amd import propose
    N = 48
    g = synthetic_case("roughwell_ne", d, N=N, seed=d, head_std=0.1, eps=3e-4)
    dyn = hip_dynamics(g, variant)
    od = oracle_dynamics(g)
    x, v = to_dev(g["x"]), to_dev(g["v"])
    rng = np.random.RandomState(1)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    Lx, _, px, outs = propose(x, dyn, do_mh_step=True, direction=to_dev(direction), v=v, u=to_dev(u))
    xo, vo, lj = dyn._forward_step(x, v, 3)
    rLx, _, rpx, _ = O.propose(g["x"], od, g["v"], g["v"], direction, u, both_directions=False)
    rxo, rvo, rlj = od.forward_step(g["x"], g["v"], np.float32(3))
    v_tol = 0.5 * 3e-4 * 1e6 * 4 * 2.0 ** -23 * float(np.abs(g["x"]).max() + 1.0)
    assert rel_err(to_np(xo), rxo) < STEP_TOL and rel_err(to_np(vo), rvo) < v_tol and rel_err(to_np(lj), rlj) < v_tol
    assert rel_err(to_np(Lx), rLx) < 1e-4
    assert abs_err(to_np(px), rpx) < 1e-2


@pytest.mark.parametrize("case", ["train_icg50", "train_tilted8", "train_rough6", "train_funnel3", "train_scg2d", "train_mog2d"])
def test_training_gradients_do_not_depend_on_the_instruction_schedule(case):
    """The per-workgroup gradient slots of one l2hmc_train_propose_grad launch (train_fast_kernel on four waves / one wave,
    dense / elementwise / funnel targets; train_small_kernel for d = 2) from TWO builds of the training translation unit --
    LLVM's default machine scheduler and `-mllvm -amdgpu-sched-strategy=max-ilp` (csrc/Makefile
    `variants/libl2hmc_hip_train_ilp.so`: another instruction order and another register allocation of every training kernel)
    -- are equal BIT FOR BIT, the NaN-prefilled entries nobody writes included.  Round 4 met a build of this kernel whose
    gradients changed with unrelated source lines; round 5 traced it to the register allocator placing a copy before a block's
    exec restore (tools/check_exec_prologue.py, which `make lint` runs over every translation unit) -- this is the dynamic
    side of the same guard: a result that moves with the schedule is a defect, whoever's."""
    import os
    import subprocess
    import sys
    import tempfile
    from tests.helpers import ROOT
    ilp = os.path.join(ROOT, "l2hmc_amd", "csrc", "variants", "libl2hmc_hip_train_ilp.so")
    assert os.path.exists(ilp), "run `make -C l2hmc_amd/csrc` (builds the second schedule of train.hip)"
    with tempfile.TemporaryDirectory() as td:
        outs = []
        for tag, lib in (("default", None), ("ilp", ilp)):
            env = dict(os.environ)
            env.pop("L2HMC_DBG_LIB", None)
            if lib:
                env["L2HMC_DBG_LIB"] = lib
            out = os.path.join(td, tag + ".npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_slots_dump.py"), "dump", case, out], cwd=ROOT,
                               env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(np.load(out))
        a, b = outs
        assert str(a["kernel"]) == str(b["kernel"])
        assert a["slots"].shape == b["slots"].shape and a["slots"].size > 0
        assert np.array_equal(a["slots"].view(np.uint32), b["slots"].view(np.uint32)), (case, str(a["kernel"]))
        assert np.array_equal(a["flat"].view(np.uint32), b["flat"].view(np.uint32)) and np.all(np.isfinite(a["flat"]))
        written = np.isfinite(a["slots"])
        assert written.mean() > 0.5           # (the dump really holds gradients: most slot entries are written)


def test_empty_shard_of_a_training_step_contributes_a_zero_gradient():
    """A rank that holds no chains (fewer chains than ranks) still takes part in the step's ONE all-reduce: its
    `l2hmc_train_step` must overwrite its gradient slice and loss terms with zeros (the reduction launch overwrites, nothing
    zeroes beforehand -- round 4 returned early and the rank re-sent the previous step's already-reduced gradient)."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd.training import Trainer
    g = load("train_icg50")
    dyn = hip_dynamics(g)
    dyn.eps_override = None
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
    tr = Trainer(dyn)
    d = int(g["x_dim"])
    tr._flat_ext.fill_(123.0)                                   # "last step's reduced gradient and tail"
    e2 = torch.empty((0, d), device="cuda")
    a, keep, _ = tr._train_args(e2, e2, torch.empty(0, dtype=torch.uint8, device="cuda"), 64)
    st = _ffi.L2hmcTrainStep()
    st.x_head, st.n_head = None, 0
    lt = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    st.loss = lt.data_ptr()
    st.terms = tr._flat_ext[tr.n_grad:].data_ptr()
    _ffi.check(_ffi.lib().l2hmc_train_step(a, st, _ffi.current_stream(dyn.device)))
    torch.cuda.synchronize()
    assert float(tr.flat.abs().max()) == 0.0
    assert float(tr._flat_ext[tr.n_grad:tr.n_grad + 6].abs().max()) == 0.0
    assert lt.cpu().tolist() == [0.0, 0.0, 0.0]
    # ... and an optimiser update on zero chains is refused
    st.theta, st.m, st.v = tr.theta.data_ptr(), tr.m.data_ptr(), tr.v.data_ptr()
    st.lr, st.beta1, st.beta2, st.epsilon, st.step = 1e-3, 0.9, 0.999, 1e-8, 1
    with pytest.raises(RuntimeError, match="at least one chain"):
        _ffi.check(_ffi.lib().l2hmc_train_step(a, st, _ffi.current_stream(dyn.device)))


# ---- net_factory in the reference's full generality (dynamics.py:69-79): ANY callable [a, b, tau, aux] -> [S, T, Q] ------------------
def _opaque(net):
    """the same function as `net`, with nothing for l2hmc_amd.layers.extract_stq to recognise"""
    return lambda inp: net(inp)


@pytest.mark.parametrize("case", ["tilted8", "icg50", "mog2d", "rough8"])
def test_arbitrary_net_callables_match_the_reference_fixtures(case):
    """The reference's `net_factory` returns any callable; here the fixture's OWN S/T/Q nets are handed over as opaque lambdas, so the
    Dynamics cannot fuse them and takes the general path (the caller's torch code between the library's launches,
    L2hmcSplitArgs.net_cb) -- which must then reproduce the reference-run fixture like the fused kernels do: single steps 3e-5,
    trajectories 1e-4 (2e-4 for the 25-step mixture, whose fused-path gate in test_gpu_train_split is the same), accept 1e-4,
    propose on the recorded draws incl. the MH select."""
    import torch
    from l2hmc_amd import Dynamics, layers, propose
    from tests.helpers import hip_energy
    g = load(case)
    d, H, T = int(g["x_dim"]), int(g["H"]), int(g["T"])
    fused = hip_dynamics(g)                               # builds the recognised nets with the fixture's weights ...
    nets = {"XNet": fused.XNet, "VNet": fused.VNet}
    dyn = Dynamics(d, hip_energy(g), T=T, eps=float(g["eps"]), net_factory=lambda x_dim, scope, factor: _opaque(nets[scope]))
    assert dyn._user_nets and dyn._split
    dyn.mask = g["mask"]
    dyn.eps_override = float(g["eps"])
    x, v = to_dev(g["x"]), to_dev(g["v"])
    traj = 2e-4 if T > 10 else 1e-4
    for s in g["steps"]:
        xo, vo, lj = dyn._forward_step(x, v, int(s))
        xb, vb, ljb = dyn._backward_step(x, v, int(s))
        for got, key in ((xo, "fstep%d.x"), (vo, "fstep%d.v"), (lj, "fstep%d.logdet"), (xb, "bstep%d.x"), (vb, "bstep%d.v"),
                         (ljb, "bstep%d.logdet")):
            assert rel_err(to_np(got), g[key % s]) < STEP_TOL, (case, key % s)
    for nm, fn in (("fwd", dyn.forward), ("bwd", dyn.backward)):
        X, V, lj = fn(x, init_v=v, log_jac=True)
        _, _, p = fn(x, init_v=v)
        assert rel_err(to_np(X), g[nm + ".x"]) < traj and rel_err(to_np(V), g[nm + ".v"]) < traj
        assert rel_err(to_np(lj), g[nm + ".logjac"]) < traj and abs_err(to_np(p), g[nm + ".p"]) < P_TOL
    Lx, Lv, px, outs = propose(x, dyn, do_mh_step=True, direction=to_dev(g["prop.dir"]),
                               v=(to_dev(g["prop.v_fwd"]), to_dev(g["prop.v_bwd"])), u=to_dev(g["prop.u"]))
    assert Lv is None
    assert rel_err(to_np(Lx), g["prop.Lx"]) < traj and abs_err(to_np(px), g["prop.px"]) < P_TOL
    from tests.helpers import check_x_next
    check_x_next(to_np(outs[0]), g["x"], g["prop.Lx"], g["prop.px"], g["prop.u"], P_TOL)
    # ... and the trainer says what it needs instead of crashing: these lambdas expose no variables (round 6 trains caller-supplied
    # nets that do -- tests/test_gpu_round6.py)
    from l2hmc_amd.training import Trainer
    with pytest.raises(ValueError, match="expose no parameters"):
        Trainer(dyn)


def test_a_net_outside_the_notebook_architecture_matches_the_oracle():
    """A structure the fused kernels do not have -- one tanh layer, S bounded by a sigmoid, Q identically zero (a Python float,
    like the reference's HMC lambdas, dynamics.py:73-76), the time input entering multiplicatively -- written twice, in torch for
    the product and in numpy for oracle/l2hmc_oracle.py's Dynamics (which takes callables), on a built-in Gaussian AND on the same
    target as a caller-supplied torch closure: direction-mixed propose + MH against the float32 oracle."""
    import torch
    from l2hmc_amd import Dynamics, distributions as D, propose
    d, N, T, eps = 6, 96, 7, 0.07
    rng = np.random.RandomState(5)
    W = {k: (0.4 * rng.randn(*shp)).astype(np.float32) for k, shp in
         (("A", (d, 12)), ("B", (d, 12)), ("C", (2, 12)), ("S", (12, d)), ("T", (12, d)))}
    Wt = {k: to_dev(v) for k, v in W.items()}

    def make_torch(scale):
        def net(inp):
            a, b, tau, aux = inp
            h = torch.tanh(a @ Wt["A"] + b @ Wt["B"]) * (1.0 + tau @ Wt["C"])
            return [scale * torch.sigmoid(h @ Wt["S"]) - 0.5 * scale, h @ Wt["T"], 0.0]
        return net

    def make_numpy(scale):
        def net(a, b, tau):
            h = np.tanh(a @ W["A"] + b @ W["B"]) * (np.float32(1.0) + tau @ W["C"])
            return (np.float32(scale) / (1 + np.exp(-(h @ W["S"]))) - np.float32(0.5 * scale), h @ W["T"], np.zeros_like(a))
        return net
    prec = np.diag(np.exp(np.linspace(-1, 1, d))).astype(np.float32)
    mu = (0.2 * rng.randn(d)).astype(np.float32)
    mask = O.init_mask(T, d, np.random.RandomState(2))
    x0 = rng.randn(N, d).astype(np.float32)
    v0 = rng.randn(N, d).astype(np.float32)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    gauss = D.Gaussian.__new__(D.Gaussian)
    gauss.mu, gauss.sigma, gauss.i_sigma = mu, None, prec
    mu_t, prec_t = to_dev(mu), to_dev(prec)

    def closure(x):                  # the same target as a plain torch callable: the caller's energy AND the caller's nets
        dx = x - mu_t
        return 0.5 * ((dx @ prec_t) * dx).sum(1)
    for energy, oracle_energy in ((gauss.get_energy_function(), O.Gaussian(mu, prec, np.float32)),
                                  (closure, O.Gaussian(mu, prec, np.float32))):
        dyn = Dynamics(d, energy, T=T, eps=eps, net_factory=lambda x_dim, scope, factor: make_torch(0.6 if scope == "XNet" else 0.3))
        assert dyn._user_nets
        dyn.mask = mask
        dyn.eps_override = eps
        od = O.Dynamics(d, oracle_energy, T, eps, mask, make_numpy(0.6), make_numpy(0.3))
        Lx, _, px, outs = propose(to_dev(x0), dyn, do_mh_step=True, direction=to_dev(direction), v=to_dev(v0), u=to_dev(u))
        rLx, _, rpx, rxn = O.propose(x0, od, v0, v0, direction, u, both_directions=False)
        assert rel_err(to_np(Lx), rLx) < 1e-4 and abs_err(to_np(px), rpx) < P_TOL
        from tests.helpers import check_x_next
        check_x_next(to_np(outs[0]), x0, rLx, rpx, u, P_TOL)
        assert 0.05 < float(px.mean()) < 0.999
    # a net that returns the wrong shape surfaces as a Python exception, not as a crash inside the library
    bad = Dynamics(d, gauss.get_energy_function(), T=T, eps=eps,
                   net_factory=lambda x_dim, scope, factor: (lambda inp: [inp[0][:, :2], inp[0], 0.0]))
    with pytest.raises(ValueError, match="must be"):
        bad.forward(to_dev(x0), init_v=to_dev(v0))


def test_training_on_presplit_planes_agrees_with_the_split_in_the_loop():
    """The GEMM-engine trainer at config 5's widths and 3072 chains (the chain count from which the decoder-sized products take the
    pre-split form, csrc/gemm_xl.hpp): round 5 puts the forward pass's and the Hessian-vector products' 1024-wide products on bf16
    planes (`vae_energy` with a DecPoint, `vae_hvp` of csrc/split.hip, train_split.hpp; activations split by the producing epilogue, weights once per
    call).  gemm_mode 2 keeps the split inside the k loop of every product: the same six bf16 products per block in the same order
    -- every product is bit-identical (tools/ubench_gemm_bf3.hip) -- but the BCE row sums of the energy are formed per 128-wide
    column tile instead of per 64-wide one: float32 partial sums of ~45 each (ulp 4e-6), 13 or 7 of them per chain, so U ~ 540
    differs by ~2e-5 and the accept probability with it (measured 2.8e-5; the suite's gate on p is 1e-4).  The proposals agree to
    2e-6, the loss to 1e-6, the gradient to 1.6e-7 of its scale (gate 1e-4: a tenth of the round-3 gate of gemm_mode 1 against
    the f32-MFMA form, which both modes also meet)."""
    import torch
    from l2hmc_amd import _ffi
    from l2hmc_amd.training import Trainer
    from tests.helpers import synthetic_vae_case
    N = 3072
    g = synthetic_vae_case(N=N, seed=7)
    rng = np.random.RandomState(4)
    dr = {"v": rng.randn(N, 50).astype(np.float32), "dir": rng.randint(0, 2, N).astype(np.uint8), "u": rng.rand(N).astype(np.float32)}
    ls = np.full((N, 50), -0.5, np.float32)
    res = {}
    for mode in (1, 2, 0):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        dyn.gemm_mode = mode
        tr = Trainer(dyn, decay_steps=0)
        loss, x_T, px = tr.sampler_loss_and_grad(to_dev(g["x"]), to_dev(g["aux"]), to_dev(ls), MH=1, draws=[dr])
        res[mode] = (float(loss), to_np(px).copy(), to_np(tr.flat).copy(), to_np(x_T).copy())
    a, b, c = res[1], res[2], res[0]
    scale = float(np.abs(c[2]).max())
    print("planes vs in-loop: loss %.9e / %.9e  |dp| %.1e  |dx| %.1e  |dgrad| / scale %.1e" % (
        a[0], b[0], np.abs(a[1] - b[1]).max(), np.abs(a[3] - b[3]).max(), np.abs(a[2] - b[2]).max() / scale))
    assert abs(a[0] - b[0]) < 1e-6 * max(1.0, abs(b[0])), (a[0], b[0])
    assert np.abs(a[1] - b[1]).max() < P_TOL, float(np.abs(a[1] - b[1]).max())
    assert rel_err(a[3], b[3]) < 2e-6, rel_err(a[3], b[3])
    assert np.abs(a[2] - b[2]).max() < 1e-4 * scale, float(np.abs(a[2] - b[2]).max() / scale)
    assert abs(a[0] - c[0]) < 1e-4 * max(1.0, abs(c[0])) and np.abs(a[1] - c[1]).max() < 5e-5
    assert np.abs(a[2] - c[2]).max() < 1e-3 * scale


@pytest.mark.parametrize("N", [3072, 8192, 8205])
def test_fused_net_launches_of_the_trainer_agree_with_the_three_products(N):
    """Round 5: the GEMM-engine trainer evaluates an S/T/Q net -- and its reverse -- in ONE launch each (`net_eval_kernel` with both
    hidden activations kept, `net_bwd_kernel`; csrc/gemm_f32.hpp) instead of three 64 x 64-tile products each.  Same contraction
    order (k ascending, four k per MFMA), same epilogues: the two forms are expected to agree to rounding, and are held to a
    hundredth of the gates of the suite.  3072 chains = 16 chains per workgroup, 8192 = 32 (the form config 5's bench runs), 8205 = the same with a last workgroup of 13
    chains (rows beyond the batch: clamped loads, no stores)."""
    import torch
    from l2hmc_amd.training import Trainer
    from tests.helpers import synthetic_vae_case
    g = synthetic_vae_case(N=N, seed=11)
    rng = np.random.RandomState(5)
    dr = {"v": rng.randn(N, 50).astype(np.float32), "dir": rng.randint(0, 2, N).astype(np.uint8), "u": rng.rand(N).astype(np.float32)}
    ls = np.full((N, 50), -0.5, np.float32)
    res = {}
    for mode in (0, 1):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        dyn.net_mode = mode
        tr = Trainer(dyn, decay_steps=0)
        loss, x_T, px = tr.sampler_loss_and_grad(to_dev(g["x"]), to_dev(g["aux"]), to_dev(ls), MH=1, draws=[dr])
        res[mode] = (float(loss), to_np(px).copy(), to_np(tr.flat).copy(), to_np(x_T).copy())
    a, b = res[0], res[1]
    scale = float(np.abs(b[2]).max())
    print("fused vs three products, %d chains: loss %.9e / %.9e  |dp| %.1e  |dx| %.1e  |dgrad| / scale %.1e  bitwise %s" % (
        N, a[0], b[0], np.abs(a[1] - b[1]).max(), np.abs(a[3] - b[3]).max(), np.abs(a[2] - b[2]).max() / scale,
        np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])))
    assert abs(a[0] - b[0]) < 1e-6 * max(1.0, abs(b[0])), (a[0], b[0])
    assert np.abs(a[1] - b[1]).max() < 1e-6 and rel_err(a[3], b[3]) < 2e-6
    assert np.abs(a[2] - b[2]).max() < 2e-6 * scale, float(np.abs(a[2] - b[2]).max() / scale)


@pytest.mark.parametrize("case", ["train_icg50_h32", "train_rough6_h20", "train_tilted8_h24"])
def test_fused_net_launches_on_ragged_widths(case):
    """The same A/B on the reference-graph fixtures of the wide-net trainer: 3 d = 18 / 24 / 150 and H = 20 / 24 / 32 are not
    multiples of 16 -- the zero padding of the weight copies and of the LDS tiles is what these exercise."""
    import torch
    from l2hmc_amd.training import SplitTrainer
    g = load(case)
    draws = {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
             "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
             "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}
    res = {}
    for mode in (0, 1):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        dyn.net_mode = mode
        tr = SplitTrainer(dyn)
        loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=draws)
        res[mode] = (float(loss), to_np(px).copy(), to_np(tr.flat).copy(), to_np(Lx).copy())
    a, b = res[0], res[1]
    scale = float(np.abs(b[2]).max())
    print("%s: |dgrad| / scale %.1e  |dp| %.1e" % (case, np.abs(a[2] - b[2]).max() / scale, np.abs(a[1] - b[1]).max()))
    assert abs(a[0] - b[0]) < 1e-6 * max(1.0, abs(b[0]))
    assert np.abs(a[1] - b[1]).max() < 1e-6 and rel_err(a[3], b[3]) < 2e-6
    assert np.abs(a[2] - b[2]).max() < 2e-6 * scale


@pytest.mark.parametrize("latent,dec_h,N", [(20, 256, 384), (50, 256, 384), (20, 1024, 6400)])
def test_split_k_latent_gradient_on_other_shapes(latent, dec_h, N):
    """`gemm_skinny_add_kernel` (the N = d <= 64, K = decoder width products: latent gradient of the decoder posterior) beyond
    config 5's own shape: d = 20 takes the two-column-block instantiation, a 256-wide decoder the 4-k-tile chunks, 6400 chains
    of a 1024-wide one the 32-row / eight-wave form with N <= 32.  Proposal against the float64 evaluation of the same map at
    the suite's gates."""
    from l2hmc_amd import propose
    from tests.helpers import check_x_next, synthetic_vae_case
    g = synthetic_vae_case(latent=latent, H=40, dec_h=dec_h, n_pix=96, enc_h=64, N=N, seed=3)
    dyn = hip_dynamics(g)
    rng = np.random.RandomState(6)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    Lx, _, px, outs = propose(to_dev(g["x"]), dyn, do_mh_step=True, direction=to_dev(direction), v=to_dev(g["v"]), u=to_dev(u),
                              aux=to_dev(g["aux"]))
    od64 = oracle_dynamics(g, np.float64)
    with np.errstate(all="ignore"):
        tLx, _, tpx, _ = O.propose(g["x"].astype(np.float64), od64, g["v"].astype(np.float64), g["v"].astype(np.float64),
                                   direction, u.astype(np.float64), both_directions=False)
    ex, ep = rel_err(to_np(Lx), tLx), abs_err(to_np(px), tpx)
    print("d %d, decoder %d, %d chains: mean p %.3f  max rel err x %.2e  |p - p64| %.2e" % (latent, dec_h, N, float(tpx.mean()), ex, ep))
    assert ex < 2e-4 and ep < 1e-4, (ex, ep)
    check_x_next(to_np(outs[0]), g["x"], tLx, tpx, u, 5e-4)


def test_pipelined_net_kernels_on_a_neighbouring_shape():
    """The software-pipelined instantiations `net_eval_kernel<2, 8, 7, 13>` / `net_bwd_kernel<2, 8, 10, 13>` are picked by the PADDED
    widths (ceil16(2 d) = 112, ceil16(H) = 208, ceil16(3 d) = 160), not by config 5's own d = 50, H = 200: d = 52, H = 204 lands on
    the same kernels with other pad columns (3 d = 156, four live columns in the last hidden block).  8192 chains (32 per
    workgroup); the sampler against the float64 evaluation of the same map at the suite's gates, the trainer's fused launches
    against its three-product form."""
    import torch
    from l2hmc_amd import propose
    from l2hmc_amd.training import Trainer
    from tests.helpers import check_x_next, synthetic_vae_case
    N, d = 8192, 52
    g = synthetic_vae_case(latent=d, H=204, dec_h=256, n_pix=96, enc_h=64, N=N, seed=8)
    dyn = hip_dynamics(g)
    rng = np.random.RandomState(9)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    Lx, _, px, outs = propose(to_dev(g["x"]), dyn, do_mh_step=True, direction=to_dev(direction), v=to_dev(g["v"]), u=to_dev(u),
                              aux=to_dev(g["aux"]))
    od64 = oracle_dynamics(g, np.float64)
    with np.errstate(all="ignore"):
        tLx, _, tpx, _ = O.propose(g["x"].astype(np.float64), od64, g["v"].astype(np.float64), g["v"].astype(np.float64),
                                   direction, u.astype(np.float64), both_directions=False)
    ex, ep = rel_err(to_np(Lx), tLx), abs_err(to_np(px), tpx)
    print("d 52, H 204, 8192 chains: mean p %.3f  max rel err x %.2e  |p - p64| %.2e" % (float(tpx.mean()), ex, ep))
    assert ex < 2e-4 and ep < 1e-4, (ex, ep)
    check_x_next(to_np(outs[0]), g["x"], tLx, tpx, u, 5e-4)
    dr = {"v": rng.randn(N, d).astype(np.float32), "dir": direction, "u": u}
    ls = np.full((N, d), -0.5, np.float32)
    res = {}
    for mode in (0, 1):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        dyn.net_mode = mode
        tr = Trainer(dyn, decay_steps=0)
        loss, x_T, pxt = tr.sampler_loss_and_grad(to_dev(g["x"]), to_dev(g["aux"]), to_dev(ls), MH=1, draws=[dr])
        res[mode] = (float(loss), to_np(pxt).copy(), to_np(tr.flat).copy(), to_np(x_T).copy())
    a, b = res[0], res[1]
    scale = float(np.abs(b[2]).max())
    print("trainer, fused vs three products: |dp| %.1e  |dgrad| / scale %.1e" % (np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max() / scale))
    assert abs(a[0] - b[0]) < 1e-6 * max(1.0, abs(b[0]))
    assert np.abs(a[1] - b[1]).max() < 1e-6 and rel_err(a[3], b[3]) < 2e-6
    assert np.abs(a[2] - b[2]).max() < 2e-6 * scale
