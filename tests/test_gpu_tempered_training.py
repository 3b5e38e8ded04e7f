"""Training at a temperature on the GPU: every trainer differentiates the notebook loss (and the VAE sampler objective) of the
dynamics on U / temperature -- the reference's graph with its `temperature` placeholder fed (dynamics.py:203-212) -- against the
float64 oracle on the tempered target (`_Tempered`), and stays consistent with the sampler at the same temperature."""
import numpy as np
import pytest

from oracle import l2hmc_oracle as O
from tests.helpers import (abs_err, check_grads_per_tensor, hip_dynamics, load, net_grads, rel_err, synthetic_case, to_dev,
                           to_np)
from tests.test_tempered_training_cpu import _Tempered

pytestmark = pytest.mark.gpu

TRAJ_TOL, P_TOL = 1e-4, 1e-4


def _draws(g):
    return {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
            "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
            "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}


def _oracle_grads(ref):
    return {k: ref[k] for k in ref if k.startswith(("xnet.", "vnet.")) or k == "alpha"}


def _tempered_dyn(g, tau):
    import torch
    dyn = hip_dynamics(g)
    dyn.eps_override = None
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
    dyn.use_temperature = True
    dyn.temperature = tau
    return dyn


def _against_oracle(g, tau, label, variant=0, force_split=False, target=None, dyn=None):
    """loss / Lx / px / every tensor against the float64 oracle on U / tau; the untempered oracle lies outside the gate"""
    from oracle import l2hmc_train_oracle as TO
    from l2hmc_amd.training import SplitTrainer, Trainer
    base = target if target is not None else TO.target_of(g, np.float64)
    ref_loss, ref = TO.training_loss_and_grad(g, np.float64, target=_Tempered(base, tau))
    dyn = dyn if dyn is not None else _tempered_dyn(g, tau)
    tr = SplitTrainer(dyn) if force_split else Trainer(dyn)
    tr.variant = variant
    loss, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss)), (label, float(loss), ref_loss)
    assert rel_err(to_np(Lx), ref["Lx"]) < TRAJ_TOL and abs_err(to_np(px), ref["px"]) < P_TOL, label
    got = net_grads(dyn)
    worst = check_grads_per_tensor(label, got, _oracle_grads(ref))
    _, plain = TO.training_loss_and_grad(g, np.float64, target=base)
    with pytest.raises(AssertionError):          # the temperature really matters at this gate
        check_grads_per_tensor(label + " (untempered oracle)", got, _oracle_grads(plain))
    print("%s: loss %.6e (ref %.6e)  worst tensor %s at %.2f of its gate" % (label, float(loss), ref_loss, worst[1], worst[0]))
    return dyn, tr


# variant 0: the register-resident / d <= 4 kernels; 100: the general tile kernel (it has no funnel Hessian-vector product)
@pytest.mark.parametrize("case,tau,variant", [(c, 2.5, v) for c in ("train_scg2d", "train_tilted8", "train_icg50", "train_mog2d",
                                                                    "train_rough6") for v in (0, 100)]
                         + [("train_funnel3", 2.5, 0), ("train_mog2d", 0.5, 0), ("train_mog2d", 0.5, 100)])
def test_tempered_training_gradient_matches_the_tempered_float64_oracle(case, tau, variant):
    _against_oracle(load(case), tau, "%s tau=%g v%d" % (case, tau, variant), variant=variant)


def test_tempered_training_at_scale_is_exact_and_reproducible():
    import torch
    from tests.test_gpu_round3 import _train_case
    g = _train_case(4096, 10, 17)
    dyn, tr = _against_oracle(g, 2.5, "icg50 N=4096 T=10 tau=2.5")
    flat1 = tr.flat.clone()
    tr.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    assert torch.equal(flat1, tr.flat)


@pytest.mark.parametrize("case", ["train_icg50_h32", "train_rough6_h20", "train_mog3d_h20"])
def test_tempered_training_on_the_gemm_engine(case):
    from l2hmc_amd.training import SplitTrainer
    dyn, tr = _against_oracle(load(case), 2.5, case + " tau=2.5")
    assert isinstance(tr, SplitTrainer)


def test_tempered_training_on_the_gemm_engine_beyond_the_fused_kernels():
    g = synthetic_case("roughwell_easy", 128, H=10, T=3, N=48, seed=1)
    rng = np.random.RandomState(3)
    N, d = 48, 128
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    from l2hmc_amd.training import SplitTrainer
    _, tr = _against_oracle(g, 2.5, "roughwell_easy d=128 tau=2.5")
    assert isinstance(tr, SplitTrainer)


def test_tempered_training_on_a_user_energy():
    import torch
    from l2hmc_amd import Dynamics, layers
    from tests.test_gpu_round3 import _BananaTarget, _banana_torch
    d, T, N, H = 5, 4, 52, 10
    g = synthetic_case("roughwell_easy", d, H=H, T=T, N=N, seed=7 + H, head_std=0.2)
    rng = np.random.RandomState(11)
    g["x"] = (rng.randn(N, d) * np.array([2.0] + [1.0] * (d - 1))).astype(np.float32)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    dyn = Dynamics(d, _banana_torch, T=T, eps=float(g["eps"]), net_factory=layers.stq_network(H), use_temperature=True)
    dyn.temperature = 2.5
    dyn.mask = g["mask"]
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
        for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    _, tr = _against_oracle(g, 2.5, "banana tau=2.5", target=_BananaTarget(), dyn=dyn)
    assert tr.user


def _vae_pair(tau):
    """the built-in decoder posterior at temperature tau, and the same decoder handed over as the closure U / tau at 1"""
    import torch
    import torch.nn.functional as F
    from l2hmc_amd import Dynamics, vae
    from tests.helpers import _load_mlp, synthetic_vae_case
    N, d, H = 64, 10, 24
    g = synthetic_vae_case(latent=d, H=H, dec_h=48, n_pix=40, enc_h=32, T=4, N=N, seed=2)
    g["dec.W3"] = (g["dec.W3"] * 30.0).astype(np.float32)
    bd = hip_dynamics(g)
    bd.eps_override = None
    bd.use_temperature, bd.temperature = True, tau
    dec = vae.make_decoder(d, 48, 40)
    enc = vae.make_encoder_sampler(40, 32, H)
    _load_mlp(dec, g, "dec.")
    _load_mlp(enc, g, "enc.")

    def energy(z, aux=None):
        logits = dec(z)
        return (F.binary_cross_entropy_with_logits(logits, aux, reduction="none").sum(1) + 0.5 * (z * z).sum(1)) / tau

    cd = Dynamics(d, energy, T=4, eps=float(g["eps"]), net_factory=vae.sampler_net_factory(d, enc, H, H))
    cd.mask = g["mask"]
    with torch.no_grad():
        cd.alpha.copy_(bd.alpha)
        for wc, wb in ((cd._xw, bd._xw), (cd._vw, bd._vw)):
            for k in O.NET_KEYS:
                wc[k].copy_(wb[k].reshape(wc[k].shape))
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            cd._xw["aux_encoder"][k].copy_(bd._xw["aux_encoder"][k].reshape(cd._xw["aux_encoder"][k].shape))
    rng = np.random.RandomState(4)
    draws = {"v": rng.randn(N, d).astype(np.float32), "dir": rng.randint(0, 2, N).astype(np.uint8),
             "u": rng.rand(N).astype(np.float32)}
    x = (0.7 * rng.randn(N, d)).astype(np.float32)
    log_sigma = np.full((N, d), -0.3, dtype=np.float32)
    return g, bd, cd, x, log_sigma, draws


def test_tempered_decoder_posterior_matches_the_closure_of_u_over_tau():
    from l2hmc_amd.training import Trainer
    tau = 2.0
    g, bd, cd, x, log_sigma, draws = _vae_pair(tau)
    aux = to_dev(g["aux"])
    tb, tc = Trainer(bd), Trainer(cd)
    assert tb.vae and tc.user and tc.image_sampler
    lb, xb, pb = tb.sampler_loss_and_grad(to_dev(x), aux, to_dev(log_sigma), MH=1, draws=[draws])
    lc, xc, pc = tc.sampler_loss_and_grad(to_dev(x), aux, to_dev(log_sigma), MH=1, draws=[draws])
    assert abs(float(lb) - float(lc)) < 1e-4 * max(1.0, abs(float(lc)))
    assert rel_err(to_np(xb), to_np(xc)) < TRAJ_TOL and abs_err(to_np(pb), to_np(pc)) < P_TOL

    def grads(dyn):
        e = dyn._xw["aux_encoder"]
        return net_grads(dyn, extra={"enc." + k: e[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")})
    worst = check_grads_per_tensor("decoder posterior tau=2 vs closure U/2", grads(bd), grads(cd))
    print("decoder posterior tau=%g: loss %.6e vs closure %.6e, worst tensor %s at %.2f of its gate"
          % (tau, float(lb), float(lc), worst[1], worst[0]))


def test_tempered_decoder_posterior_energy_term_is_of_the_plain_energy():
    """energy_scale > 0 (mnist_vae.py:209-224): built from the plain closure energy(final_x, aux), not from the tempered one --
    the chains do not move, the loss moves by exactly es * mean(1 / ed - ed), ed = (U(Lx) - U(x))^2 p + 1e-4 of the PLAIN U."""
    import torch
    from l2hmc_amd.training import Trainer
    tau, es = 2.0, 0.3
    g, bd, _, x, log_sigma, draws = _vae_pair(tau)
    draws = dict(draws, u=np.zeros_like(draws["u"]))        # every proposal accepted: x_T is the proposal Lx
    aux = to_dev(g["aux"])
    tb = Trainer(bd)
    l0, x0, p0 = tb.sampler_loss_and_grad(to_dev(x), aux, to_dev(log_sigma), MH=1, draws=[draws])
    l1, x1, p1 = tb.sampler_loss_and_grad(to_dev(x), aux, to_dev(log_sigma), MH=1, draws=[draws], energy_scale=es)
    assert torch.equal(x0, x1) and torch.equal(p0, p1)
    U0 = bd.energy(to_dev(x), aux=aux).double()             # (the decoder posterior's own energy: untempered)
    U1 = bd.energy(x1, aux=aux).double()
    p = p1.double()
    ed = (U1 - U0) ** 2 * p + 1e-4
    want = es * float((1.0 / ed - ed).mean())
    got = float(l1) - float(l0)
    edt = ((U1 - U0) / tau) ** 2 * p + 1e-4
    tempered = es * float((1.0 / edt - edt).mean())
    print("energy term: %.6e (plain U %.6e, tempered U would give %.6e)" % (got, want, tempered))
    assert abs(got - want) < 2e-3 * max(1.0, abs(want))
    assert abs(tempered - want) > 1e-2 * max(1.0, abs(want))


def _gauss_dyn(var, tau, seed=0):
    import torch
    from l2hmc_amd import Dynamics, distributions as D, layers
    d = var.shape[0]
    torch.manual_seed(seed)
    np.random.seed(seed)
    dyn = Dynamics(d, D.Gaussian(np.zeros(d), np.diag(var)).get_energy_function(), T=10, eps=0.1,
                   net_factory=layers.stq_network(10), use_temperature=tau is not None)
    if tau is not None:
        dyn.temperature = tau
    return dyn


def test_fused_step_at_a_temperature_is_the_step_on_the_widened_gaussian():
    """One Trainer.step (gradient, in-launch Metropolis select and Adam) on N(0, diag var) at tau = 2.5 against the step on
    N(0, diag(2.5 var)) at tau = 1: same seed, same weights."""
    import torch
    from l2hmc_amd.training import Trainer
    d, N, tau = 50, 4096, 2.5
    # variances whose precisions P and P / tau are both exact float32 numbers
    rng = np.random.RandomState(1)
    prec_w = rng.randint(1, 64, d) / 32.0
    var_w = 1.0 / prec_w
    var = var_w / tau
    a, b = _gauss_dyn(var, tau), _gauss_dyn(var_w, None)
    with torch.no_grad():
        for wa, wb in ((a._xw, b._xw), (a._vw, b._vw)):
            for k in O.NET_KEYS:
                wb[k].copy_(wa[k])
        b.alpha.copy_(a.alpha)
    b.mask = a.mask
    ta, tb = Trainer(a, seed=5), Trainer(b, seed=5)
    x = torch.as_tensor((rng.randn(N, d) * np.sqrt(var_w)).astype(np.float32), device="cuda")
    u = rng.rand(N).astype(np.float32)
    la, pa, xa, _ = ta.step(x, u=to_dev(u))
    lb, pb, xb, _ = tb.step(x, u=to_dev(u))
    assert abs(float(la) - float(lb)) < 1e-4 * max(1.0, abs(float(lb)))
    assert abs_err(to_np(pa), to_np(pb)) < P_TOL
    clear = np.abs(to_np(pb) - u) > 10 * P_TOL                  # chains whose select the accept probability's rounding cannot flip
    assert clear.mean() > 0.9 and rel_err(to_np(xa)[clear], to_np(xb)[clear]) < TRAJ_TOL
    # the flat gradient the in-launch Adam consumed, tensor by tensor
    def per_tensor(tr):
        f = to_np(tr.flat)
        out = {"t%02d" % i: f[off:off + n] for i, (_, off, n) in enumerate(tr.slots)}
        out["alpha"] = f[-1:]
        return out
    check_grads_per_tensor("fused step tau=2.5 vs widened Gaussian", per_tensor(ta), per_tensor(tb))


def test_trainer_proposal_agrees_with_the_sampler_at_the_same_temperature():
    import torch
    from l2hmc_amd import propose
    from l2hmc_amd.training import Trainer
    g = load("train_icg50")
    dyn = _tempered_dyn(g, 2.5)
    tr = Trainer(dyn)
    dr = _draws(g)
    _, Lx, px = tr.loss_and_grad(to_dev(g["x"]), draws=dr)
    with torch.no_grad():
        sLx, _, spx, _ = propose(to_dev(g["x"]), dyn, direction=to_dev(g["x.dir"]), v=to_dev(dr["x_v"]))
    assert rel_err(to_np(Lx), to_np(sLx)) < TRAJ_TOL and abs_err(to_np(px), to_np(spx)) < P_TOL


def test_temperature_is_read_at_every_call():
    import torch
    from l2hmc_amd.training import Trainer
    g = load("train_mog2d")
    dyn = _tempered_dyn(g, 3.0)
    tr = Trainer(dyn)
    dyn.temperature = 3.0
    tr.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    dyn.temperature = 1.5
    l1, L1, p1 = tr.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    f1 = tr.flat.clone()
    fresh = _tempered_dyn(g, 1.5)
    tf = Trainer(fresh)
    l2, L2, p2 = tf.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    assert torch.equal(f1, tf.flat) and torch.equal(L1, L2) and torch.equal(p1, p2) and float(l1) == float(l2)
    # use_temperature=False: the plain Dynamics, bit for bit, whatever `temperature` holds
    off = _tempered_dyn(g, 2.5)
    off.use_temperature = False
    plain = hip_dynamics(g)
    plain.eps_override = None
    with torch.no_grad():
        plain.alpha.fill_(float(np.log(g["eps"])))
    to, tp = Trainer(off), Trainer(plain)
    lo, Lo, po = to.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    lp, Lp, pp = tp.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
    assert torch.equal(to.flat, tp.flat) and torch.equal(Lo, Lp) and torch.equal(po, pp) and float(lo) == float(lp)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        dyn.temperature = bad
        with pytest.raises(ValueError, match="temperature"):
            tr.loss_and_grad(to_dev(g["x"]), draws=_draws(g))
        with pytest.raises(ValueError, match="temperature"):
            tr.step(to_dev(g["x"]))
