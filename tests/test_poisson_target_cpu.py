"""CPU: the fused Poisson-regression target (L2HMC_ENERGY_POISSON = 8) as far as it goes without a GPU -- the ABI number, the
two forms of `PoissonRegression.get_energy_function`, the argument checks of the library (nothing is launched: every call is
refused before it touches a device), the training refusals, and the bounds of tests/poisson_target_case.py held against a float32
numpy restatement of U and grad U.  The inputs of the GPU test's overflow case are checked here too: its two classes of chains
are properties of the float32 oracle alone."""
import os
import re

import numpy as np
import pytest

from l2hmc_amd import PoissonRegression, _ffi
from l2hmc_amd import distributions as D
from tests import poisson_target_case as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096              # a non-NULL "device pointer" for calls that are refused before anything reads it


def test_energy_kind_is_8_in_the_binding_and_the_header():
    assert _ffi.ENERGY_POISSON == 8
    header = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    m = re.search(r"L2HMC_ENERGY_POISSON\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _ffi.ENERGY_POISSON
    assert re.search(r"#define\s+L2HMC_ABI_VERSION\s+6\b", header) and _ffi.ABI_VERSION == 6
    assert "l2hmc_poisson_offset_floats" in header and "l2hmc_poisson_offset_floats" in _ffi.SYMBOLS
    import ctypes
    assert ctypes.sizeof(_ffi.L2hmcEnergy) == 56


def test_both_forms_of_the_energy_function():
    _, X, y, o = pc.case(4, 37, 3)
    model = PoissonRegression(X, y, offset=o, prior_var=2.5)
    slow = model.get_energy_function()
    assert type(slow) is D.UserEnergy and slow.kind == D.ENERGY_USER
    assert type(model.get_energy_function(fused=False)) is D.UserEnergy
    e = model.get_energy_function(fused=True)
    assert type(e) is D.PoissonEnergy and isinstance(e, D.EnergyFunction)
    assert e.kind == _ffi.ENERGY_POISSON == 8 and e.n_comp == 37 and e.eta == 2.5 and e.x_dim == 3
    e0 = PoissonRegression(X, y, prior_var=2.5).get_energy_function(fused=True)        # offset=None: zeros
    assert np.array_equal(e0._host["offset"], np.zeros(37, dtype=np.float32))


def _energy(kind=8, n=100, mu=FAKE, prec=FAKE, eta=2.0):
    return _ffi.L2hmcEnergy(kind, n, mu, prec, None, eta, 0, 1.0, 0.0, 0.0, 0)


def _traj(e, d):
    a = _ffi.L2hmcTrajectoryArgs()
    a.energy = e
    a.n_chains, a.d, a.T, a.n_steps, a.eps_host = 16, d, 5, 5, 0.1
    a.x = a.v = a.masks = a.trig = FAKE
    return a


@pytest.mark.parametrize("kw,d,msg", [
    ({"prec": None}, 5, b"Poisson regression needs the offsets (prec: l2hmc_poisson_offset_floats(n_data) floats, zeros for none)"),
    ({"mu": None}, 5, b"Poisson regression needs the packed data (mu, l2hmc_pack_logistic with the counts as labels)"),
    ({}, 129, b"Poisson regression supports d <= 128 (got 129)"),
    ({"eta": 0.0}, 5, b"Poisson regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"eta": float("inf")}, 5, b"Poisson regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"n": 0}, 5, b"Poisson regression needs 1 <= n_comp = n_data <= 1048576 (got 0)"),
    ({"n": (1 << 20) + 1}, 5, b"Poisson regression needs 1 <= n_comp = n_data <= 1048576 (got 1048577)"),
])
def test_energy_and_trajectory_refuse_bad_arguments_without_a_gpu(kw, d, msg):
    L = _ffi.lib()
    e = _energy(**kw)
    assert L.l2hmc_energy(e, FAKE, 16, d, None, None, None) == -1
    assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()
    assert L.l2hmc_trajectory(_traj(e, d), None) == -1
    assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()


def test_offset_size_query():
    L = _ffi.lib()
    assert [L.l2hmc_poisson_offset_floats(n) for n in (1, 16, 17, 1000, 1 << 20)] == [16, 16, 32, 1008, 1 << 20]
    assert L.l2hmc_poisson_offset_floats(0) == -1 and b"Poisson regression" in L.l2hmc_last_error()
    assert L.l2hmc_poisson_offset_floats((1 << 20) + 1) == -1


def test_training_entry_points_name_the_other_route():
    L = _ffi.lib()
    route = b"train on the same likelihood as a caller-supplied energy"
    assert L.l2hmc_train_fused_lds_bytes(8, 100, 5, 10, 5) == -2
    assert b"Poisson-regression target" in L.l2hmc_last_error() and route in L.l2hmc_last_error()
    a = _ffi.L2hmcTrainArgs()
    a.energy = _energy()
    a.n_chains, a.d, a.H, a.T, a.eps_host, a.scale, a.inv_n = 16, 5, 10, 5, 0.1, 0.1, 1.0 / 16
    net = _ffi.L2hmcNet(*([FAKE] * 16))
    import ctypes
    a.xnet = a.vnet = ctypes.pointer(net)
    for k in ("masks", "trig", "x", "v", "Lx", "p", "v1", "grad", "workspace"):
        setattr(a, k, FAKE)
    assert L.l2hmc_train_propose_grad(a, None) == -2
    assert b"Poisson-regression target" in L.l2hmc_last_error() and route in L.l2hmc_last_error()


def test_trainer_refuses_the_fused_energy_and_names_the_slow_path():
    from l2hmc_amd.training import LogisticTrainer, SplitTrainer, Trainer

    class Dyn(object):                      # what Trainer.__new__ reads before anything else
        pass
    dyn = Dyn()
    _, X, y, o = pc.case(4, 37, 3)
    dyn._fn = PoissonRegression(X, y, offset=o).get_energy_function(fused=True)
    for cls in (Trainer, SplitTrainer, LogisticTrainer):
        with pytest.raises(NotImplementedError, match=r"get_energy_function\(\)") as ei:
            cls(dyn)
        assert "load_state_dict" in str(ei.value) and "slow path" in str(ei.value)


@pytest.mark.parametrize("n,d", [(17, 5), (1000, 25)])
def test_bounds_hold_for_a_float32_restatement(n, d):
    for zero in (False, True):
        W, X, y, o = pc.case(40, n, d, zero_offset=zero)
        U, G = pc.energy(W, X, y, o)
        U32, G32 = pc.energy(W, X, y, o, dtype=np.float32)
        b = pc.bounds(W, X, y, o)
        sU, sg = pc.used(U32, G32, U, G, b)
        print("n=%d d=%d zero_offset=%s: float32 numpy uses %.3f of the U bound, %.3f of the grad U bound" % (n, d, zero, sU, sg))
        assert sU <= 1.0 and sg <= 1.0
        assert np.all(b["U"] < 1e-3 * np.abs(U).max()) and np.all(b["g"] < 1e-3 * np.abs(G).max() + 1e-3)     # (they bind)
        for T, beta in ((2.5, 1.0), (1.0, 0.3)):
            Us, Gs, bs = pc.scaled(W, X, y, o, temperature=T, beta=beta)
            q = np.float32(0.5) * (W * W).sum(axis=1)
            Ub = (np.float32(1 - beta) * q + np.float32(beta) * U32) / np.float32(T)
            Gb = (np.float32(1 - beta) * W + np.float32(beta) * G32) / np.float32(T)
            sU, sg = pc.used(Ub, Gb, Us, Gs, bs)
            assert sU <= 1.0 and sg <= 1.0, (T, beta, sU, sg)


def test_the_bounds_see_a_wrong_link():
    """a float32 energy that drops the offsets' rounding is inside; one that adds exp(0) for a padded row, or uses mu - y in U, is not"""
    W, X, y, o = pc.case(40, 17, 5)
    U, G = pc.energy(W, X, y, o)
    b = pc.bounds(W, X, y, o)
    assert pc.used(U + 1.0, G, U, G, b)[0] > 1.0                           # one unmasked padded row: exp(0) = 1 more
    assert pc.used(U, G + 1e-4 * np.abs(G).max(), U, G, b)[1] > 1.0


def test_trajectory_step_sizes_come_from_the_oracle():
    for n, d, H in [(17, 5, 0), (200, 25, 10)]:
        c = pc.traj_case(n, d, H)
        p = c["ref"]["forward"][3]
        assert 0.2 < float(p.mean()) < 1.0 and np.all(np.isfinite(c["ref"]["forward"][0]))
        print("n=%d d=%d H=%d: eps %g, oracle accept %.3f, float32-float64 distances %s" % (n, d, H, c["eps"], p.mean(), c["dist"]["forward"]))


def test_overflow_case_has_its_two_classes():
    c = pc.overflow_case()
    assert c["nonfinite"].sum() >= pc.OVER_N // 8 and c["accepted"].sum() >= pc.OVER_N // 8
    assert not np.any(c["nonfinite"] & c["accepted"]) and np.all(c["p"][c["nonfinite"]] == 0.0)
    U0 = pc.energy(c["x"], c["X"], c["y"], c["o"], dtype=np.float32)[0]
    assert np.all(np.isfinite(U0)) and np.all(c["u"] > 0.0)               # every chain starts at a finite energy
    print("overflow case: %d non-finite, %d accepted of %d" % (c["nonfinite"].sum(), c["accepted"].sum(), pc.OVER_N))
