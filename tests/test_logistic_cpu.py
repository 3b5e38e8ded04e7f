"""CPU: the Bayesian logistic-regression target's ABI (kind 7, the pack functions), its host-side argument checks, the Python
validation of LogisticRegression and the Trainer's refusal -- no GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest

from l2hmc_amd import LogisticRegression, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_kind_7_and_the_pack_functions():
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    assert int(re.search(r"L2HMC_ENERGY_LOGISTIC = (\d+)", hdr).group(1)) == 7 == _ffi.ENERGY_LOGISTIC
    assert int(re.search(r"#define L2HMC_ABI_VERSION (\d+)", hdr).group(1)) == 6
    for name in ("l2hmc_packed_logistic_floats", "l2hmc_pack_logistic"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    L = _ffi.lib()
    assert L.l2hmc_struct_bytes(1) == 56 == ctypes.sizeof(_ffi.L2hmcEnergy)


def test_packed_size_and_pack_argument_errors():
    L = _ffi.lib()
    # per 16-row block: two fragment orders of NT = ceil(d / 16) groups (256 floats each) and 16 labels
    assert L.l2hmc_packed_logistic_floats(1000, 25) == 63 * (512 * 2 + 16)
    assert L.l2hmc_packed_logistic_floats(17, 5) == 2 * (512 + 16)
    assert L.l2hmc_packed_logistic_floats(8192, 128) == 512 * (512 * 8 + 16)
    for n, d in ((0, 5), (5, 0), (5, 129), (1 << 20 | 1, 5)):
        assert L.l2hmc_packed_logistic_floats(n, d) == -1, (n, d)
    assert L.l2hmc_pack_logistic(None, None, 16, 5, None, None) == -1
    assert b"NULL" in L.l2hmc_last_error()
    assert L.l2hmc_pack_logistic(None, None, 16, 200, None, None) == -1
    assert b"d <= 128" in L.l2hmc_last_error() or b"1 <= d <= 128" in L.l2hmc_last_error()


def test_energy_argument_errors_on_the_host():
    L = _ffi.lib()
    fake = 0x1000                                                   # never dereferenced: the checks come first
    x = ctypes.c_void_p(fake)

    def energy(**kw):
        e = dict(kind=_ffi.ENERGY_LOGISTIC, n_comp=100, mu=fake, prec=None, logc=None, eta=1.0, easy=0, temperature=1.0,
                 anneal_beta=0.0, den=0.0, reserved_=0)
        e.update(kw)
        return _ffi.L2hmcEnergy(**e)
    for bad, d, msg in ((energy(eta=0.0), 5, b"eta"), (energy(eta=-1.0), 5, b"eta"), (energy(mu=None), 5, b"packed data"),
                        (energy(n_comp=0), 5, b"n_comp"), (energy(), 129, b"d <= 128")):
        assert L.l2hmc_energy(bad, x, 16, d, x, x, None) == -1
        assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()
        assert L.l2hmc_p_accept(bad, x, x, x, x, x, 16, d, x, None) == -1
    a = _ffi.L2hmcTrajectoryArgs()
    a.energy = energy(eta=0.0)
    a.n_chains, a.d, a.T, a.n_steps = 16, 5, 4, 4
    a.x = a.v = a.masks = a.trig = fake
    a.eps_host = 0.1
    assert L.l2hmc_trajectory(a, None) == -1 and b"eta" in L.l2hmc_last_error()
    # the trainers have no logistic-regression kernel
    assert L.l2hmc_train_fused_lds_bytes(_ffi.ENERGY_LOGISTIC, 100, 5, 10, 10) == -2


def test_python_validation():
    X = np.random.RandomState(0).randn(20, 3)
    y = (np.arange(20) % 2).astype(np.float32)
    m = LogisticRegression(X, y, prior_var=0.5)
    assert m.dim == 3 and m.X.dtype == np.float32 and m.prior_var == 0.5
    e = m.get_energy_function()
    assert e.kind == _ffi.ENERGY_LOGISTIC and e.x_dim == 3 and e.n_comp == 20 and e.eta == 0.5
    with pytest.raises(ValueError, match="0 or 1"):
        LogisticRegression(X, np.where(y > 0, 2.0, 0.0))
    with pytest.raises(ValueError, match="0 or 1"):
        LogisticRegression(X, y - 0.5)
    with pytest.raises(ValueError, match="y must be"):
        LogisticRegression(X, y[:10])
    with pytest.raises(ValueError, match="X must be"):
        LogisticRegression(X[:, 0], y)
    with pytest.raises(ValueError, match="d <= 128"):
        LogisticRegression(np.zeros((4, 129)), np.zeros(4))
    with pytest.raises(ValueError, match="finite"):
        LogisticRegression(np.full((20, 3), np.nan), y)
    for pv in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="prior_var"):
            LogisticRegression(X, y, prior_var=pv)
    # the unnormalised log density is -U
    W = np.random.RandomState(1).randn(4, 3)
    L_ = W @ X.T
    want = -((np.logaddexp(0, L_) - y * L_).sum(1) + 0.5 * np.square(W).sum(1) / 0.5)
    assert np.allclose(m.log_density(W), want, rtol=1e-6)


def test_trainer_refuses_with_the_working_route():
    from l2hmc_amd.training import Trainer

    class FakeDynamics(object):                                     # the fields Trainer reads before any GPU work
        _user_nets = _user = _split = False
        hmc, anneal_beta, x_dim, H, T = False, 0.0, 3, 10, 10
        _fn = LogisticRegression(np.eye(3), np.array([0.0, 1.0, 1.0])).get_energy_function()
    with pytest.raises(NotImplementedError, match="torch callable") as ei:
        Trainer(FakeDynamics())
    assert "state_dict" in str(ei.value)
