"""GPU, round 3: the parity holes the round-2 review named.

* `chain_operator` (utils/sampler.py:57-85) against the reference's OWN run of it (goldens' `chainop.*` keys), not only
  against the oracle;
* training gradients at chain counts that go through many workgroups and the two-level reduction (1024 and 4096 chains:
  128 / 512 workgroups) against the float64 reverse-mode oracle (itself pinned by the reference-graph fixtures);
* the tempered energy (`use_temperature`, dynamics.py:203-212) through trajectories, propose and the energy entry points
  (the generic per-case tests of test_gpu_parity.py pick `tilted8_temp` up as well; here the bigger-d kernels).
"""
import numpy as np
import pytest

from oracle import l2hmc_oracle as O
from tests.helpers import (CHAINOP_CASES, abs_err, aux_of, check_grads_per_tensor, check_x_next, fixture_grads, hip_dynamics,
                           load, net_grads, oracle_dynamics, rel_err, synthetic_case, to_dev, to_np)


def _oracle_grads(ref):
    """the float64 training oracle's output dict as name -> array ('xnet.W1', ..., 'alpha')"""
    return {k: ref[k] for k in ref if k.startswith(("xnet.", "vnet.")) or k == "alpha"}

pytestmark = pytest.mark.gpu

TRAJ_TOL, P_TOL = 1e-4, 1e-4


@pytest.mark.parametrize("case", CHAINOP_CASES)
def test_chain_operator_matches_the_reference_run(case):
    """HIP `chain_operator` on the draws the reference's chain_operator made (init_v = its first normal draw; per
    composed proposal the direction bits and BOTH momentum draws; the final MH uniform): final state, final momentum,
    accept probability and MH-selected state.  K composed trajectories => 3x the single-trajectory tolerances."""
    from l2hmc_amd import chain_operator
    g = load(case)
    dyn = hip_dynamics(g)
    K = int(g["chainop.K"])
    kw = {}
    if not int(g["hmc"]):
        kw = dict(directions=[to_dev(a) for a in g["chainop.dir"]],
                  vs=[(to_dev(a), to_dev(b)) for a, b in zip(g["chainop.v_fwd"], g["chainop.v_bwd"])])
    fx, fv, p, outs = chain_operator(to_dev(g["x"]), dyn, K, aux=aux_of(g), init_v=to_dev(g["chainop.init_v"]),
                                     do_mh_step=True, u=to_dev(g["chainop.u"]), **kw)
    rx, rv, rp, u = g["chainop.x"], g["chainop.v"], g["chainop.p"], g["chainop.u"]
    fin = np.all(np.isfinite(rx), axis=1) & (np.abs(rx).max(axis=1) < 1e3)
    assert fin.mean() > 0.9
    print("%s: chain_operator K=%d  x %.2e  v %.2e  p %.2e" % (case, K, rel_err(to_np(fx)[fin], rx[fin]),
                                                               rel_err(to_np(fv)[fin], rv[fin]), abs_err(to_np(p)[fin], rp[fin])))
    assert rel_err(to_np(fx)[fin], rx[fin]) < 3 * TRAJ_TOL
    assert rel_err(to_np(fv)[fin], rv[fin]) < 3 * TRAJ_TOL
    assert abs_err(to_np(p)[fin], rp[fin]) < 3 * P_TOL
    assert np.all(to_np(p)[~fin] == 0)
    check_x_next(to_np(outs[0])[fin], g["x"][fin], rx[fin], rp[fin], u[fin], 3 * P_TOL)


def _train_case(N, T, seed):
    """ICG-50 weights/target of the `train_icg50` fixture with N chains in the typical set and fresh draws."""
    g = dict(load("train_icg50"))
    rng = np.random.RandomState(seed)
    d = int(g["x_dim"])
    var = 1.0 / np.diagonal(g["energy.i_sigma"])
    g["x"] = (rng.randn(N, d) * np.sqrt(var)).astype(np.float32)
    g["z"] = rng.randn(N, d).astype(np.float32)
    g["T"], g["N"] = T, N
    g["mask"] = O.init_mask(T, d, rng)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    return g


@pytest.mark.parametrize("N,T,variant", [(1024, 4, 0), (1024, 4, 100), (4096, 10, 0)])
def test_training_gradient_at_scale_matches_the_float64_oracle(N, T, variant):
    """2N chain-trajectories ([x; z]) = 128 / 512 sixteen-chain workgroups through the per-workgroup gradient slots and
    the second-level reduction, against oracle/l2hmc_train_oracle.py in float64 (the fixtures stop at 64 chains).  The
    4096-chain, Lf = 10 case is the training step `profiles/*_train_timing.txt` times."""
    import torch
    from oracle import l2hmc_train_oracle as TO
    from l2hmc_amd.training import Trainer
    g = _train_case(N, T, 17)
    ref_loss, ref = TO.training_loss_and_grad(g, np.float64)
    dyn = hip_dynamics(g)
    dyn.eps_override = None
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
    tr = Trainer(dyn)
    tr.variant = variant
    draws = {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
             "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
             "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}
    loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=draws)
    assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert rel_err(to_np(Lx), ref["Lx"]) < TRAJ_TOL and abs_err(to_np(px), ref["px"]) < P_TOL
    # per tensor (round 6): 2e-4 of the tensor's own max + 1e-6 of the scale
    worst = check_grads_per_tensor("N=%d T=%d v%d" % (N, T, variant), net_grads(dyn), _oracle_grads(ref))
    print("N=%d T=%d variant %d: loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate"
          % (N, T, variant, float(loss), ref_loss, worst[1], worst[0]))
    # bitwise reproducible at this size too (fixed-order slot reduction, no atomics)
    flat1 = tr.flat.clone()
    tr.loss_and_grad(to_dev(g["x"]), draws=draws)
    assert torch.equal(flat1, tr.flat)


@pytest.mark.parametrize("kind,d,N,T", [("roughwell_easy", 128, 48, 3), ("roughwell_easy", 300, 33, 2), ("gauss_diag", 96, 40, 3)])
def test_training_beyond_the_fused_kernels_runs_on_the_gemm_engine(kind, d, N, T):
    """Shapes no fused training kernel holds (d > 64 with H = 10: l2hmc_train_fused_lds_bytes says UNSUPPORTED) --
    `Trainer(dynamics)` hands them to the GEMM-engine trainer by itself; its gradient against the float64 oracle."""
    import torch
    from oracle import l2hmc_train_oracle as TO
    from l2hmc_amd import _ffi
    from l2hmc_amd.training import SplitTrainer, Trainer
    from tests.helpers import synthetic_case
    g = synthetic_case(kind, d, H=10, T=T, N=N, seed=d, head_std=0.1)
    rng = np.random.RandomState(9)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    ref_loss, ref = TO.training_loss_and_grad(g, np.float64)
    dyn = hip_dynamics(g)
    assert _ffi.lib().l2hmc_train_fused_lds_bytes(int(dyn._fn.kind), 1, d, 10, T) == -2
    dyn.eps_override = None
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
    tr = Trainer(dyn)
    assert isinstance(tr, SplitTrainer)
    draws = {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
             "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
             "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}
    loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=draws)
    assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert rel_err(to_np(Lx), ref["Lx"]) < TRAJ_TOL and abs_err(to_np(px), ref["px"]) < P_TOL
    worst = check_grads_per_tensor("float64 oracle", net_grads(dyn), _oracle_grads(ref))     # per tensor (round 6)
    print("loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate" % (float(loss), ref_loss, worst[1], worst[0]))
    # and a few optimiser steps run (sampling on the fused wide-state kernels, gradient on the engine)
    x = to_dev(g["x"])
    for _ in range(3):
        out = tr.step(x)
        x = out[2]
    assert torch.isfinite(x).all()


@pytest.mark.parametrize("kind,d,N,T", [("gmm4", 2, 1024, 5), ("gmm2", 2, 200, 10), ("gmm8", 4, 333, 3)])
def test_gmm_training_gradient_on_the_d4_kernel_matches_the_float64_oracle(kind, d, N, T):
    """Mixture-of-Gaussians targets (config 3's energy, distributions.py:104-134) on the one-dimension-per-lane trainer
    (`train_small_kernel`: responsibilities and Hessian-vector product through the chain's four lanes) against
    oracle/l2hmc_train_oracle.py in float64, and against the general tile kernel."""
    import torch
    from oracle import l2hmc_train_oracle as TO
    from l2hmc_amd.training import Trainer
    from tests.helpers import synthetic_case
    g = synthetic_case(kind, d, H=10, T=T, N=N, seed=41 + d, head_std=0.2)
    rng = np.random.RandomState(5)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    ref_loss, ref = TO.training_loss_and_grad(g, np.float64)
    draws = {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
             "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
             "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}
    flats = {}
    for variant in (0, 100):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        tr = Trainer(dyn)
        tr.variant = variant
        loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=draws)
        assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (variant, float(loss), ref_loss)
        assert rel_err(to_np(Lx), ref["Lx"]) < TRAJ_TOL and abs_err(to_np(px), ref["px"]) < P_TOL
        worst = check_grads_per_tensor("float64 oracle", net_grads(dyn), _oracle_grads(ref))     # per tensor (round 6)
        print("loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate" % (float(loss), ref_loss, worst[1], worst[0]))
        flats[variant] = tr.flat.clone()
        tr.loss_and_grad(to_dev(g["x"]), draws=draws)
        assert torch.equal(flats[variant], tr.flat)             # fixed-order slot reduction: bitwise reproducible


@pytest.mark.parametrize("kind,d,variant", [("gauss_diag", 50, 0), ("gauss_diag", 50, 4), ("gauss_dense", 24, 0),
                                            ("roughwell_easy", 40, 0), ("gauss_diag", 200, 0), ("gauss_diag", 2, 0),
                                            ("gauss_dense", 200, 0)])
def test_tempered_energy_on_every_kernel_family(kind, d, variant):
    """use_temperature=True, T = 2.5 (dynamics.py:203-212: U and grad U divided by the fed temperature) -- the fast /
    tile / dense / wide / lane kernels must either honour it or hand over to a kernel that does: propose vs the oracle,
    energy and gradient entry points vs the oracle."""
    from l2hmc_amd import propose
    N = 96
    g = synthetic_case(kind, d, H=10, T=5, N=N, seed=d)
    g["temperature"] = np.float32(2.5)
    rng = np.random.RandomState(4)
    dr, u = rng.randint(0, 2, N).astype(np.uint8), rng.rand(N).astype(np.float32)
    dyn, od = hip_dynamics(g, variant), oracle_dynamics(g)
    assert dyn.use_temperature and dyn.temperature == 2.5
    Lx, _, px, o = propose(to_dev(g["x"]), dyn, do_mh_step=True, direction=to_dev(dr), v=to_dev(g["v"]), u=to_dev(u))
    with np.errstate(all="ignore"):
        rLx, _, rpx, _ = O.propose(g["x"], od, g["v"], g["v"], dr, u, both_directions=False)
        cold = O.propose(g["x"], oracle_dynamics({k: v for k, v in g.items() if k != "temperature"}), g["v"], g["v"],
                         dr, u, both_directions=False)
    assert rel_err(cold[0], rLx) > 1e-2          # the temperature really changes the trajectory
    assert rel_err(to_np(Lx), rLx) < TRAJ_TOL and abs_err(to_np(px), rpx) < P_TOL, (kind, d, variant)
    check_x_next(to_np(o[0]), g["x"], rLx, rpx, u, P_TOL)
    assert rel_err(to_np(dyn.energy(to_dev(g["x"]))), od.energy(g["x"])) < 1e-5
    assert rel_err(to_np(dyn.grad_energy(to_dev(g["x"]))), od.grad_energy(g["x"])) < 1e-5
    if d == 50 and variant == 0:
        # a kernel that has no tempered form refuses loudly when forced ...
        with pytest.raises(RuntimeError, match="variant 16"):
            propose(to_dev(g["x"]), hip_dynamics(g, 16), direction=to_dev(dr), v=to_dev(g["v"]))
        # ... and is not what the automatic choice takes at its chain count (16 384: the one-wave-per-tile kernel's range)
        big = np.tile(g["x"], (171, 1))[:16384]
        bv, bd = np.tile(g["v"], (171, 1))[:16384], np.tile(dr, 171)[:16384]
        bLx, _, bpx, _ = propose(to_dev(big), dyn, direction=to_dev(bd), v=to_dev(bv))
        assert rel_err(to_np(bLx)[:N], rLx) < TRAJ_TOL and abs_err(to_np(bpx)[:N], rpx) < P_TOL


@pytest.mark.timeout(600)
def test_bench_launches_its_own_ranks_the_way_the_driver_calls_it():
    """`python bench.py --gpus 2` with NO torchrun and no WORLD_SIZE (the driver's plain invocation): bench.py becomes the
    launcher, two ranks start through torch.distributed.run, rank 0 prints ONE JSON line.  Rehearsed on the 1-GPU box with
    both ranks on cuda:0 over gloo (`--one-device --backend gloo`; on the 8-GPU node the same path runs one rank per GPU
    over RCCL).  Checks the weak-scaling headline and, with `--full`, the `strong65536` key (65 536 chains in total over
    the ranks) and the `dist` key (sharded ESS + flat-gradient all-reduce)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--one-device", "--backend", "gloo",
                        "--steps", "20", "--warmup", "5", "--full"], capture_output=True, text=True, timeout=560, env=env)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["steps"] == 20 and out["warmup"] == 5
    assert out["config"]["chains_per_gpu"] == 4096 and out["config"]["chains_total"] == 8192
    assert out["config"]["state_finite"] and out["value"] > 1e8
    s = out["strong65536"]
    assert s["chains_per_gpu"] == 32768 and s["scaling"] == "strong" and s["state_finite"] and s["value"] > 1e8
    assert 0.0 < s["rank0_frac"] < 1.0 and 0.01 < s["mean_accept_prob"] <= 1.0
    d = out["dist"]
    assert d["ranks"] == 2 and d["backend"] == "gloo" and d["sharded_training"]["parameters_identical_across_ranks"]
    assert 4e-3 < d["sharded_ess"]["ess_per_mh_step"] < 8e-3
    # a mismatching --gpus / WORLD_SIZE is a clear error, not an assert deep inside
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                        timeout=120, env=env2)
    assert r2.returncode != 0 and "WORLD_SIZE" in (r2.stderr + r2.stdout)


# ---- caller-supplied energies (the slow path: U / grad U from the caller's torch code between launches) --------------
def _banana_np(x, b=0.3, s=2.0):
    """U(x) = x0^2 / (2 s^2) + 1/2 sum_{k>=1} (x_k + b x0^2 - s^2 b)^2 and its gradient (numpy; dtype of x)."""
    t = x[:, 1:] + b * x[:, :1] ** 2 - s * s * b
    U = 0.5 * x[:, 0] ** 2 / (s * s) + 0.5 * np.sum(t * t, axis=1)
    g = np.empty_like(x)
    g[:, 0] = x[:, 0] / (s * s) + 2 * b * x[:, 0] * np.sum(t, axis=1)
    g[:, 1:] = t
    return U, g


def _banana_torch(x, b=0.3, s=2.0):
    t = x[:, 1:] + b * x[:, :1] ** 2 - s * s * b
    return 0.5 * x[:, 0] ** 2 / (s * s) + 0.5 * (t * t).sum(1)


class _BananaTarget:
    """The banana density above with its Hessian-vector product, for oracle/l2hmc_train_oracle.py (dtype of the inputs)."""

    def __init__(self, b=0.3, s=2.0):
        self.b, self.s = b, s

    def energy(self, x):
        return _banana_np(x, self.b, self.s)[0]

    def grad(self, x):
        return _banana_np(x, self.b, self.s)[1]

    def hessvec(self, x, u):
        b, s = self.b, self.s
        t = x[:, 1:] + b * x[:, :1] ** 2 - s * s * b
        out = np.empty_like(x)
        h00 = 1.0 / (s * s) + 2 * b * np.sum(t, axis=1) + 4 * b * b * x[:, 0] ** 2 * (x.shape[1] - 1)
        out[:, 0] = u[:, 0] * h00 + 2 * b * x[:, 0] * np.sum(u[:, 1:], axis=1)
        out[:, 1:] = 2 * b * x[:, :1] * u[:, :1] + u[:, 1:]
        return out


@pytest.mark.parametrize("H,explicit_grad", [(10, False), (24, True)])
def test_training_on_a_user_energy_matches_the_float64_oracle(H, explicit_grad):
    """The notebook loss on a target that is NOT in utils/distributions.py, given as a plain torch callable: `Trainer`
    runs on the GEMM engine, U / grad U / Hessian-vector products come from autograd through the caller's code
    (double backward, or one backward through the caller's own gradient function) -- loss, proposals and every
    parameter gradient against oracle/l2hmc_train_oracle.py with the same density in numpy float64; then a few
    optimiser steps."""
    import torch
    from oracle import l2hmc_train_oracle as TO
    from l2hmc_amd import Dynamics, layers
    from l2hmc_amd.training import SplitTrainer, Trainer
    d, T, N = 5, 4, 52
    g = synthetic_case("roughwell_easy", d, H=H, T=T, N=N, seed=7 + H, head_std=0.2)
    rng = np.random.RandomState(11)
    g["x"] = (rng.randn(N, d) * np.array([2.0] + [1.0] * (d - 1))).astype(np.float32)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    ref_loss, ref = TO.training_loss_and_grad(g, np.float64, target=_BananaTarget())
    grad_fn = None
    if explicit_grad:
        def grad_fn(x):
            t = x[:, 1:] + 0.3 * x[:, :1] ** 2 - 4 * 0.3
            return torch.cat([x[:, :1] / 4 + 0.6 * x[:, :1] * t.sum(1, keepdim=True), t], dim=1)
    dyn = Dynamics(d, _banana_torch, T=T, eps=float(g["eps"]), net_factory=layers.stq_network(H), grad_energy=grad_fn)
    dyn.mask = g["mask"]
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
        for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    tr = Trainer(dyn)
    assert isinstance(tr, SplitTrainer) and tr.user
    draws = {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
             "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
             "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}
    loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=draws)
    assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert rel_err(to_np(Lx), ref["Lx"]) < TRAJ_TOL and abs_err(to_np(px), ref["px"]) < P_TOL
    worst = check_grads_per_tensor("float64 oracle", net_grads(dyn), _oracle_grads(ref))     # per tensor (round 6)
    print("loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate" % (float(loss), ref_loss, worst[1], worst[0]))
    x = to_dev(g["x"])
    for _ in range(3):
        x = tr.step(x)[2]
    assert torch.isfinite(x).all()

    # an exception inside the caller's code surfaces as itself, not as a crash in the C frame
    def bad(x):
        raise ValueError("boom in the user's energy")
    dyn2 = Dynamics(d, bad, T=T, eps=0.1, net_factory=layers.stq_network(H))
    with pytest.raises(ValueError, match="boom"):
        Trainer(dyn2).loss_and_grad(to_dev(g["x"]), draws=draws)


@pytest.mark.parametrize("H,hmc,explicit_grad", [(10, False, False), (24, False, True), (10, True, False)])
def test_user_energy_banana_matches_the_oracle(H, hmc, explicit_grad):
    """A target that is NOT in utils/distributions.py (a banana density), given to `Dynamics` as a plain torch callable:
    propose + MH, single steps, energy / grad_energy / p_accept against `O.Dynamics` with the same density in numpy --
    nets and half-updates on the HIP kernels, U / grad U from autograd (or the caller's own gradient function)."""
    import torch
    from l2hmc_amd import Dynamics, layers, propose, sample_chain
    from tests.helpers import golden_nets
    d, T, N = 6, 5, 80
    g = synthetic_case("roughwell_easy", d, H=H, T=T, N=N, seed=H, head_std=0.3)
    rng = np.random.RandomState(5)
    x0 = (rng.randn(N, d) * np.array([2.0] + [1.0] * (d - 1))).astype(np.float32)
    v0 = rng.randn(N, d).astype(np.float32)
    dr, u = rng.randint(0, 2, N).astype(np.uint8), rng.rand(N).astype(np.float32)
    grad_fn = None
    if explicit_grad:
        def grad_fn(x):
            t = x[:, 1:] + 0.3 * x[:, :1] ** 2 - 4 * 0.3
            return torch.cat([x[:, :1] / 4 + 0.6 * x[:, :1] * t.sum(1, keepdim=True), t], dim=1)
    dyn = Dynamics(d, _banana_torch, T=T, eps=float(g["eps"]), hmc=hmc,
                   net_factory=None if hmc else layers.stq_network(H), grad_energy=grad_fn)
    dyn.mask = g["mask"]
    dyn.eps_override = float(g["eps"])
    xn = vn = None
    if not hmc:
        xn, vn = golden_nets(g)
        with torch.no_grad():
            for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
                for k in O.NET_KEYS:
                    w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    od = O.Dynamics(d, _banana_np, T, g["eps"], g["mask"], xn, vn)
    od64 = O.Dynamics(d, _banana_np, T, g["eps"], g["mask"], xn, vn, dtype=np.float64)
    # energy / gradient entry points
    assert rel_err(to_np(dyn.energy(to_dev(x0))), od.energy(x0)) < 1e-5
    assert rel_err(to_np(dyn.grad_energy(to_dev(x0))), od.grad_energy(x0)) < 1e-5
    # one step in each direction, a whole proposal with MH
    for name, hip, orc in (("fwd", dyn._forward_step, od.forward_step), ("bwd", dyn._backward_step, od.backward_step)):
        hx, hv, hl = hip(to_dev(x0), to_dev(v0), 2)
        rx, rv, rl = orc(x0, v0, 2)
        assert rel_err(to_np(hx), rx) < 3e-5 and rel_err(to_np(hv), rv) < 3e-5 and rel_err(to_np(hl), rl) < 3e-5, name
    if hmc:
        Lx, Lv, px, outs = propose(to_dev(x0), dyn, init_v=to_dev(v0), do_mh_step=True, u=to_dev(u))
        rLx, rLv, rpx, _ = O.propose(x0, od, v0, u=u)
        tLx, _, tpx, _ = O.propose(x0.astype(np.float64), od64, v0.astype(np.float64), u=u.astype(np.float64))
    else:
        Lx, Lv, px, outs = propose(to_dev(x0), dyn, init_v=to_dev(v0), do_mh_step=True, direction=to_dev(dr),
                                   v=to_dev(v0), u=to_dev(u))
        rLx, rLv, rpx, _ = O.propose(x0, od, v0, v0, dr, u, both_directions=False)
        tLx, _, tpx, _ = O.propose(x0.astype(np.float64), od64, v0.astype(np.float64), v0.astype(np.float64), dr,
                                   u.astype(np.float64), both_directions=False)
    print("banana H=%d hmc=%d: x %.2e v %.2e p %.2e (vs fp64: x %.2e p %.2e)"
          % (H, hmc, rel_err(to_np(Lx), rLx), rel_err(to_np(Lv), rLv), abs_err(to_np(px), rpx),
             rel_err(to_np(Lx), tLx), abs_err(to_np(px), tpx)))
    assert rel_err(to_np(Lx), rLx) < TRAJ_TOL and rel_err(to_np(Lv), rLv) < TRAJ_TOL
    assert abs_err(to_np(px), rpx) < P_TOL and abs_err(to_np(px), tpx) < P_TOL
    check_x_next(to_np(outs[0]), x0, rLx, rpx, u, P_TOL)
    # p_accept on arbitrary end points; the sampler loop with the library's Philox stream == the same draws injected
    pa = dyn.p_accept(to_dev(x0), to_dev(v0), Lx, Lv, torch.zeros(N, device="cuda"))
    assert abs_err(to_np(pa), od.p_accept(x0, v0, to_np(Lx), to_np(Lv), np.zeros(N, np.float32))) < P_TOL
    xf, p3, _ = sample_chain(to_dev(x0), dyn, 3, seed=9)
    from l2hmc_amd.sampler import philox_draws
    pv, pd, pu = philox_draws(9, N, d, 3)
    xi, pi, _ = sample_chain(to_dev(x0), dyn, 3, v=pv, u=pu, direction=None if hmc else pd)
    assert torch.equal(xf, xi) and torch.equal(p3, pi)
    assert bool(torch.isfinite(xf).all()) and 0.0 < float(p3.mean()) <= 1.0


def test_user_energy_errors_surface_as_python_exceptions():
    """An exception inside the caller's energy (here: a wrong output shape) aborts the trajectory and is re-raised."""
    from l2hmc_amd import Dynamics, propose
    dyn = Dynamics(3, lambda x: (x * x).sum(), T=2, eps=0.1, hmc=True)          # returns a scalar, not (N,)
    with pytest.raises(ValueError, match="shape"):
        propose(to_dev(np.zeros((8, 3), np.float32)), dyn)

    def boom(x):
        raise KeyError("inside the callback")
    dyn2 = Dynamics(3, lambda x: (x * x).sum(1), T=2, eps=0.1, hmc=True, grad_energy=boom)
    with pytest.raises(KeyError, match="inside the callback"):
        propose(to_dev(np.zeros((8, 3), np.float32)), dyn2)


def test_the_vae_posterior_as_a_plain_closure_matches_the_reference_golden():
    """mnist_vae.py:122-126's `energy(z, aux)` written as the reference writes it -- a closure over a decoder built from
    the layer kit, BCE-with-logits + prior in torch ops -- handed to `Dynamics` unchanged, with the image-conditioned
    nets of :134-167: trajectories, the log-Jacobian, accept probabilities and `propose` against the fixture the
    reference's own graph produced (`vae_small`), and against the built-in decoder-posterior path."""
    import torch
    import torch.nn.functional as F
    from l2hmc_amd import Dynamics, propose, vae
    from tests.helpers import _load_mlp
    g = load("vae_small")
    d, H = int(g["x_dim"]), int(g["H"])
    dec = vae.make_decoder(d, g["dec.W1"].shape[1], g["dec.W3"].shape[1])
    enc = vae.make_encoder_sampler(g["enc.W1"].shape[0], g["enc.W1"].shape[1], H)
    _load_mlp(dec, g, "dec.")
    _load_mlp(enc, g, "enc.")

    def energy(z, aux=None):                                        # mnist_vae.py:122-126
        logits = dec(z)
        log_posterior = -F.binary_cross_entropy_with_logits(logits, aux, reduction="none").sum(1)
        log_prior = -0.5 * (z * z).sum(1)
        return -log_posterior - log_prior

    dyn = Dynamics(d, energy, T=int(g["T"]), eps=float(g["eps"]), net_factory=vae.sampler_net_factory(d, enc, H, H))
    dyn.mask = g["mask"]
    dyn.eps_override = float(g["eps"])
    with torch.no_grad():
        for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    aux = to_dev(g["aux"])
    x, v = to_dev(g["x"]), to_dev(g["v"])
    assert rel_err(to_np(dyn.energy(x, aux=aux)), g["energy"]) < 1e-5
    assert rel_err(to_np(dyn.grad_energy(x, aux=aux)), g["grad_energy"]) < 1e-5
    for nm, fn in (("fwd", dyn.forward), ("bwd", dyn.backward)):
        X, V, lj = fn(x, init_v=v, aux=aux, log_jac=True)
        _, _, p = fn(x, init_v=v, aux=aux)
        assert rel_err(to_np(X), g[nm + ".x"]) < TRAJ_TOL and rel_err(to_np(V), g[nm + ".v"]) < TRAJ_TOL, nm
        assert rel_err(to_np(lj), g[nm + ".logjac"]) < TRAJ_TOL and abs_err(to_np(p), g[nm + ".p"]) < P_TOL, nm
    Lx, _, px, outs = propose(x, dyn, aux=aux, do_mh_step=True, direction=to_dev(g["prop.dir"]),
                              v=(to_dev(g["prop.v_fwd"]), to_dev(g["prop.v_bwd"])), u=to_dev(g["prop.u"]))
    assert rel_err(to_np(Lx), g["prop.Lx"]) < TRAJ_TOL and abs_err(to_np(px), g["prop.px"]) < P_TOL
    check_x_next(to_np(outs[0]), g["x"], g["prop.Lx"], g["prop.px"], g["prop.u"], P_TOL)
    # ... and the built-in (GEMM-engine) decoder posterior gives the same proposal
    bd = hip_dynamics(g)
    bLx, _, bpx, _ = propose(x, bd, aux=aux, do_mh_step=True, direction=to_dev(g["prop.dir"]),
                             v=(to_dev(g["prop.v_fwd"]), to_dev(g["prop.v_bwd"])), u=to_dev(g["prop.u"]))
    assert rel_err(to_np(Lx), to_np(bLx)) < 5e-5 and abs_err(to_np(px), to_np(bpx)) < 5e-5
    with pytest.raises(ValueError, match="aux"):
        propose(x, dyn)


def test_training_the_vae_sampler_on_a_plain_closure_matches_the_reference_graph():
    """mnist_vae.py:185-226's sampler objective with the model handed over as the reference hands it over -- the closure
    energy(z, aux) of :122-126 over a decoder from the layer kit, no bespoke energy class: loss, proposal, accept
    probability and the gradient of every sampler variable (image branch and alpha included) against `tf.gradients` of
    the reference's own graph (fixture `train_vae_small`); U, grad U and the Hessian-vector products come from autograd
    through the closure."""
    import torch
    import torch.nn.functional as F
    from l2hmc_amd import Dynamics, vae
    from l2hmc_amd.training import SplitTrainer, Trainer
    from tests.helpers import _load_mlp
    g = load("train_vae_small")
    d, H = int(g["x_dim"]), int(g["H"])
    dec = vae.make_decoder(d, g["dec.W1"].shape[1], g["dec.W3"].shape[1])
    enc = vae.make_encoder_sampler(g["enc.W1"].shape[0], g["enc.W1"].shape[1], H)
    _load_mlp(dec, g, "dec.")
    _load_mlp(enc, g, "enc.")

    def energy(z, aux=None):                                        # mnist_vae.py:122-126
        logits = dec(z)
        return F.binary_cross_entropy_with_logits(logits, aux, reduction="none").sum(1) + 0.5 * (z * z).sum(1)

    dyn = Dynamics(d, energy, T=int(g["T"]), eps=float(g["eps"]), net_factory=vae.sampler_net_factory(d, enc, H, H))
    dyn.mask = g["mask"]
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
        for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    tr = Trainer(dyn)
    assert isinstance(tr, SplitTrainer) and tr.user and tr.image_sampler and not tr.vae
    draws = {"v": np.where(g["prop.dir"][:, None] != 0, g["prop.v_fwd"], g["prop.v_bwd"]), "dir": g["prop.dir"], "u": g["prop.u"]}
    loss, x_T, px = tr.sampler_loss_and_grad(to_dev(g["x"]), to_dev(g["aux"]), to_dev(g["log_sigma"]), MH=1, draws=[draws])
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    assert abs_err(to_np(px), g["px"]) < P_TOL and rel_err(to_np(x_T), g["x_next"]) < TRAJ_TOL
    e = dyn._xw["aux_encoder"]
    got = net_grads(dyn, extra={"enc." + k: e[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")})
    worst = check_grads_per_tensor("closure-trained VAE sampler", got, fixture_grads(g))      # per tensor incl. the image branch
    print("closure-trained VAE sampler: loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate" % (float(loss), float(g["loss"]), worst[1], worst[0]))


@pytest.mark.parametrize("gemm_mode", [0, 1, 3])
def test_config5_at_a_chain_count_that_takes_the_big_gemm_tiles(gemm_mode):
    """Config 5's widths (decoder 50 -> 1024 -> 1024 -> 784, H = 200 nets + image branch, Lf = 5) at 3072 chains -- the
    smallest batch whose decoder products take the big workgroup tiles, i.e. the kernels the 8192-chain numbers are quoted on
    (`test_config5_full_size_against_oracle`, 192 chains, only reaches the 64 x 64 form).  Both arithmetic modes of those
    products: 0 = f32-input MFMA on 128 x 128 / 128 x 112 tiles (gemm_nt_kernel), 1 = bf16x3 (exact three-way bf16 split of every
    fp32 operand, six products on the bf16 MFMA, fp32 accumulation) -- since round 4 on PRE-SPLIT planes and 256 x 128 tiles
    (gemm_xlp_kernel; the in-loop split of round 3 stays in the training path, test below), 3 = f16x2 planes (round 6: exact
    two-way f16 split, THREE f16 MFMAs per block pair on the same plane layout; what Dynamics asks for).  SAME tolerances for all, against
    the float64 evaluation of the same map: positions 2e-4 relative, accept probability 1e-4 absolute (north_star)."""
    from l2hmc_amd import propose
    from tests.helpers import synthetic_vae_case
    N = 3072
    g = synthetic_vae_case(N=N, seed=5)
    dyn = hip_dynamics(g)
    dyn.gemm_mode = gemm_mode
    rng = np.random.RandomState(2)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    aux = aux_of(g)
    Lx, _, px, outs = propose(to_dev(g["x"]), dyn, do_mh_step=True, direction=to_dev(direction), v=to_dev(g["v"]),
                              u=to_dev(u), aux=aux)
    from l2hmc_amd import _ffi
    assert _ffi.last_kernel() == ("gemm_xlp_kernel" if gemm_mode in (1, 3) else "gemm_nt_kernel")
    od64 = oracle_dynamics(g, np.float64)
    with np.errstate(all="ignore"):
        tLx, _, tpx, _ = O.propose(g["x"].astype(np.float64), od64, g["v"].astype(np.float64), g["v"].astype(np.float64),
                                   direction, u.astype(np.float64), both_directions=False)
    ex, ep = rel_err(to_np(Lx), tLx), abs_err(to_np(px), tpx)
    print("config 5 @ %d chains, gemm_mode %d: mean p %.3f  max rel err x %.2e  |p - p64| max %.2e  99.9%% %.2e"
          % (N, gemm_mode, float(tpx.mean()), ex, ep, np.quantile(np.abs(to_np(px) - tpx), 0.999)))
    assert ex < 2e-4 and ep < 1e-4, (gemm_mode, ex, ep)
    check_x_next(to_np(outs[0]), g["x"], tLx, tpx, u, 5e-4)


def test_bf16x3_training_gradient_agrees_with_the_f32_mfma_one_at_big_tile_sizes():
    """(and, since round 6, gemm_mode 3: forward evaluations on f16x2 planes)  The sampler-training gradient (l2hmc_train_split_grad: forward with everything kept, reverse sweep, decoder
    Hessian-vector products) at 3072 chains of config 5's widths, decoder-sized products as bf16x3 vs as f32-input MFMA:
    loss, accept probabilities and the whole flat gradient [XNet | VNet | eps | image branch] agree to fp32 rounding level
    (the f32 form is pinned against the reference graph / the float64 autograd oracle at fixture sizes)."""
    import torch
    from l2hmc_amd.training import Trainer
    from tests.helpers import synthetic_vae_case
    N = 3072
    g = synthetic_vae_case(N=N, seed=7)
    rng = np.random.RandomState(4)
    dr = {"v": rng.randn(N, 50).astype(np.float32), "dir": rng.randint(0, 2, N).astype(np.uint8), "u": rng.rand(N).astype(np.float32)}
    ls = np.full((N, 50), -0.5, np.float32)
    res = {}
    for mode in (0, 1, 3):
        dyn = hip_dynamics(g)
        dyn.eps_override = None
        with torch.no_grad():
            dyn.alpha.fill_(float(np.log(g["eps"])))
        dyn.gemm_mode = mode
        tr = Trainer(dyn, decay_steps=0)
        loss, x_T, px = tr.sampler_loss_and_grad(to_dev(g["x"]), to_dev(g["aux"]), to_dev(ls), MH=1, draws=[dr])
        res[mode] = (float(loss), to_np(px), to_np(tr.flat).copy())
    a, b = res[0], res[1]
    scale = float(np.abs(a[2]).max())
    print("loss %.6e vs %.6e   |dp| %.2e   |dgrad| %.2e (scale %.2e)" % (a[0], b[0], np.abs(a[1] - b[1]).max(),
                                                                         np.abs(a[2] - b[2]).max(), scale))
    assert abs(a[0] - b[0]) < 1e-4 * max(1.0, abs(a[0]))
    assert np.abs(a[1] - b[1]).max() < 5e-5
    # (1 / v^2 weights of a few chains with v ~ 1e-4 amplify the 2e-5 difference in p that either arithmetic has against
    #  float64: the gate is the size of that conditioning, a wrong product would be off by O(scale))
    assert np.abs(a[2] - b[2]).max() < 1e-3 * scale
    # gemm_mode 3 (round 6): the FORWARD evaluations on f16x2 planes, the reverse sweep's tangent / adjoint planes bf16x3 -- same gates
    c = res[3]
    print("mode 3: loss %.6e   |dp| %.2e   |dgrad| %.2e" % (c[0], np.abs(a[1] - c[1]).max(), np.abs(a[2] - c[2]).max()))
    assert abs(a[0] - c[0]) < 1e-4 * max(1.0, abs(a[0]))
    assert np.abs(a[1] - c[1]).max() < 5e-5
    assert np.abs(a[2] - c[2]).max() < 1e-3 * scale


@pytest.mark.parametrize("d", [2, 8, 32, 128, 512])
def test_config4_rough_well_sweep_at_full_chain_count(d):
    """BASELINE.json config 4 as the bench runs it: Rough Well (easy, eta = 0.1), 16 384 chains, Lf = 10, the AUTOMATIC kernel
    choice at every d of the sweep (d <= 4 form, 1 / 4 waves per tile, one wave per tile, LDS-resident state) -- direction-
    mixed propose + MH against the fp32 oracle, bracketed by the float64 one like the other full-size checks, and the
    two-half-batches bit-equality (sharding invariance).  The bounded-argument sin / cos of round 3 is on this path."""
    import torch
    from l2hmc_amd import propose
    N = 16384
    g = synthetic_case("roughwell_easy", d, H=10, T=10, N=N, seed=100 + d, head_std=0.3 if d < 100 else 0.1)
    rng = np.random.RandomState(9)
    direction = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.rand(N).astype(np.float32)
    dyn = hip_dynamics(g, 0)
    x, v = to_dev(g["x"]), to_dev(g["v"])
    Lx, _, px, outs = propose(x, dyn, do_mh_step=True, direction=to_dev(direction), v=v, u=to_dev(u))
    with np.errstate(all="ignore"):
        rLx, _, rpx, _ = O.propose(g["x"], oracle_dynamics(g), g["v"], g["v"], direction, u, both_directions=False)
        tLx, _, tpx, _ = O.propose(g["x"].astype(np.float64), oracle_dynamics(g, np.float64), g["v"].astype(np.float64),
                                   g["v"].astype(np.float64), direction, u.astype(np.float64), both_directions=False)
    fin = np.all(np.isfinite(tLx), axis=1) & (np.abs(tLx).max(axis=1) < 1e4)
    assert fin.mean() > 0.95
    scale = np.maximum(1.0, np.abs(tLx).max(axis=1))
    e_hip = np.abs(to_np(Lx) - tLx).max(axis=1) / scale
    e_o32 = np.abs(rLx - tLx).max(axis=1) / scale
    ep_hip, ep_o32 = np.abs(to_np(px) - tpx)[fin], np.abs(rpx - tpx)[fin]
    print("rough well d=%d N=%d: x err vs fp64 hip 99%% %.1e max %.1e | oracle32 max %.1e ; p err hip max %.1e | oracle32 %.1e ; mean p %.3f"
          % (d, N, np.quantile(e_hip[fin], 0.99), e_hip[fin].max(), e_o32[fin].max(), ep_hip.max(), ep_o32.max(), float(tpx.mean())))
    assert np.quantile(e_hip[fin], 0.99) < TRAJ_TOL and e_hip[fin].max() < 3 * e_o32[fin].max() + TRAJ_TOL
    assert np.quantile(ep_hip, 0.99) < P_TOL and ep_hip.max() < 3 * ep_o32.max() + P_TOL
    check_x_next(to_np(outs[0])[fin], g["x"][fin], tLx[fin], tpx[fin], u[fin], 5 * P_TOL)
    # half batches: d <= 4 switches kernels at chain-count thresholds, so pin the variant the full batch took only where
    # both halves take the same automatic choice (8192 chains: 4-wave tile for d >= 33, same small / wide kernels otherwise)
    if d != 32:
        h = N // 2
        for lo, hi in ((0, h), (h, N)):
            Lx_h, _, px_h, _ = propose(x[lo:hi].contiguous(), dyn, do_mh_step=True, direction=to_dev(direction[lo:hi]),
                                       v=v[lo:hi].contiguous(), u=to_dev(u[lo:hi]))
            if d in (2, 8, 128, 512):
                assert torch.equal(Lx_h, Lx[lo:hi]) and torch.equal(px_h, px[lo:hi]), d
