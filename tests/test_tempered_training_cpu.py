"""Training at a temperature without a GPU: the trainers accept a tempered Dynamics (U / temperature, the reference's
dynamics.py:203-212 with temperature fed on every sess.run), keep refusing the AIS bridge, and the float64 yardstick the GPU
tests hold them to is itself pinned."""
import numpy as np
import pytest

from l2hmc_amd import distributions as D


class _Tempered(object):
    """U / tau of an oracle target (oracle/l2hmc_train_oracle.py: energy / grad / hessvec), delegating in call order so that a
    target that caches its last point (the mixture's hessvec reads the gradient of the last grad call) still works."""

    def __init__(self, target, tau):
        self.t, self.tau = target, float(tau)

    def energy(self, x):
        return self.t.energy(x) / self.tau

    def grad(self, x):
        return self.t.grad(x) / self.tau

    def hessvec(self, x, v):
        return self.t.hessvec(x, v) / self.tau


def _dyn(d, tau=2.5, H=10, beta=0.0):
    from l2hmc_amd import Dynamics, layers
    e = D.RoughWell(d, 0.1, easy=True).get_energy_function()
    dyn = Dynamics(d, e, T=5, eps=0.1, net_factory=layers.stq_network(H), device="cpu", use_temperature=True)
    dyn.temperature = tau
    dyn.anneal_beta = beta
    return dyn


def test_trainers_build_on_a_tempered_dynamics():
    from l2hmc_amd.training import SplitTrainer, Trainer
    assert type(Trainer(_dyn(50))) is Trainer
    assert isinstance(Trainer(_dyn(128)), SplitTrainer)


def test_annealed_dynamics_is_still_refused():
    from l2hmc_amd.training import Trainer
    for d in (50, 128):
        with pytest.raises(NotImplementedError, match="anneal_beta"):
            Trainer(_dyn(d, tau=2.5, beta=0.5))
        with pytest.raises(NotImplementedError, match="anneal_beta"):
            Trainer(_dyn(d, tau=1.0, beta=0.5))


@pytest.mark.parametrize("tau", [0.0, -1.0, float("inf"), float("nan")])
def test_bad_temperature_is_an_argument_error(tau):
    from l2hmc_amd.training import Trainer, train_temperature
    dyn = _dyn(50, tau=tau)
    with pytest.raises(ValueError, match="temperature"):
        train_temperature(dyn)
    with pytest.raises(ValueError, match="temperature"):
        Trainer(dyn)


def test_temperature_follows_the_reference_rule():
    from l2hmc_amd.training import train_temperature
    dyn = _dyn(4, tau=2.5)
    assert train_temperature(dyn) == 2.5
    dyn.temperature = 0.75                     # read at every call: a schedule is the caller setting it before each step
    assert train_temperature(dyn) == 0.75
    dyn.use_temperature = False
    assert train_temperature(dyn) == 1.0
    dyn.temperature = float("nan")             # (not used, not checked: use_temperature=False trains on the plain U)
    assert train_temperature(dyn) == 1.0


def test_tempered_yardstick_is_the_gaussian_of_scaled_variance():
    """The float64 oracle on `_Tempered(Gaussian, tau)` is the oracle on the Gaussian whose variances are tau times larger."""
    from oracle import l2hmc_train_oracle as TO
    from tests.helpers import synthetic_case
    tau, d = 2.5, 6
    N = 12
    g = synthetic_case("gauss_diag", d, H=8, T=3, N=N, seed=3)
    rng = np.random.RandomState(5)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    # (precisions of a few bits, so that P and P / tau are both exact in float32: the two targets differ by the factor alone)
    prec_t = (rng.randint(1, 32, d) / 16.0).astype(np.float32)
    prec = (prec_t.astype(np.float64) * tau).astype(np.float32)
    assert np.array_equal(prec.astype(np.float64) / tau, prec_t.astype(np.float64))
    mu = rng.randn(d).astype(np.float32)
    plain = TO.GaussianTarget(mu, np.diag(prec), np.float64)
    wide = TO.GaussianTarget(mu, np.diag(prec_t), np.float64)
    l1, r1 = TO.training_loss_and_grad(g, np.float64, target=_Tempered(plain, tau))
    l2, r2 = TO.training_loss_and_grad(g, np.float64, target=wide)
    assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
    for k in r2:
        a, b = np.asarray(r1[k], np.float64), np.asarray(r2[k], np.float64)
        assert np.abs(a - b).max() <= 1e-12 * max(1e-300, np.abs(b).max()), k
    # ... and the temperature matters
    l0, _ = TO.training_loss_and_grad(g, np.float64, target=plain)
    assert abs(l0 - l2) > 1e-6 * max(1.0, abs(l2))


def test_tempered_mixture_yardstick_keeps_the_cached_point():
    """GMM's hessvec reads the gradient of the last grad call: the wrapper delegates in order, so its Hessian-vector product
    is exactly the plain one / tau (not / tau^2)."""
    from oracle import l2hmc_train_oracle as TO
    rng = np.random.RandomState(0)
    d = 3
    mus = rng.randn(2, d)
    S = np.stack([np.eye(d) * 2.0, np.eye(d) * 0.5])
    t = TO.GMMTarget(mus, S, [0.3, 0.7], np.float64)
    w = _Tempered(TO.GMMTarget(mus, S, [0.3, 0.7], np.float64), 2.5)
    x, v = rng.randn(7, d), rng.randn(7, d)
    g0 = t.grad(x)
    h0 = t.hessvec(x, v)
    g1 = w.grad(x)
    h1 = w.hessvec(x, v)
    assert np.allclose(g1 * 2.5, g0, rtol=1e-14, atol=0) and np.allclose(h1 * 2.5, h0, rtol=1e-14, atol=0)
