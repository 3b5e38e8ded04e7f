"""CPU: training on the fused logistic-regression target -- the new query's ABI and values, the host-side argument checks of
the training entry for kind 7, `LogisticTrainer`'s export and refusals, the new kernel's resources, and the oracle target the
GPU tests compare against (its Hessian-vector product and gradient pinned by central finite differences).  No GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest

import l2hmc_amd
from l2hmc_amd import LogisticRegression, _ffi
from tests.logistic_train_case import PRIOR_VAR, LogisticTarget, blr_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = "l2hmc_train_logistic_lds_bytes"


def test_the_query_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    assert re.search(r"int64_t\s+%s\s*\(\s*int32_t n_data, int32_t d, int32_t H, int32_t T\)" % QUERY, hdr)
    assert _ffi.SYMBOLS[QUERY] == (ctypes.c_int64, [ctypes.c_int32] * 4)
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), QUERY)
    assert int(re.search(r"#define L2HMC_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _ffi.lib().l2hmc_abi_version()
    assert _ffi.lib().l2hmc_struct_bytes(1) == 56                    # additive: no struct changed


def plan_bytes(d, H, T):
    """csrc/train.hip train_layout(d, H, T, 7, 1, data_global = true) restated: two weight and two gradient images of the
    flat net parameters, masks / trig / exponent tables, 20 (16, ldd) and 8 (16, ldh) matrices, per-chain scalars; no mean /
    precision area (the data streams from L2) and no partial-sum matrices (the waves' partial sums reuse idle ones)."""
    def up4(n):
        return (n + 3) // 4 * 4

    def pitch(n):
        p = up4(n)
        return p + 4 if (p // 4) % 2 == 0 else p
    P = 5 * d * H + H * H + 6 * H + 5 * d
    floats = (4 * up4(P) + 4 + up4(T * d) + up4(2 * T) + 4 + 4 * up4(d) + 20 * 16 * pitch(d) + 8 * 16 * pitch(H)
              + 2 * 16 * 8 + 16 * 16)
    return 4 * floats


def test_query_values_refusal_and_bad_arguments():
    L = _ffi.lib()
    fn = getattr(L, QUERY)
    for n, d, H, T in ((1, 2, 10, 6), (17, 5, 10, 6), (1000, 25, 10, 10), (300, 50, 10, 10), (200, 25, 15, 6), (300, 50, 15, 10),
                       (300, 64, 10, 10), (1 << 20, 25, 10, 10)):
        want = plan_bytes(d, H, T)
        assert want <= 160 * 1024
        assert fn(n, d, H, T) == want, (n, d, H, T)
    assert fn(300, 50, 10, 10) == fn(5, 50, 10, 10)                 # the data is not staged: the row count does not enter
    # beyond the plan: refused with the bytes
    for d, H, T in ((128, 10, 10), (100, 10, 10)):
        want = plan_bytes(d, H, T)
        assert want > 160 * 1024
        assert fn(300, d, H, T) == -2
        assert str(want).encode() in L.l2hmc_last_error() and b"LDS" in L.l2hmc_last_error(), L.l2hmc_last_error()
    for bad in ((0, 5, 10, 10), (-1, 5, 10, 10), ((1 << 20) + 1, 5, 10, 10), (100, 0, 10, 10), (100, 129, 10, 10),
                (100, 5, 0, 10), (100, 5, 10, 0)):
        assert fn(*bad) == -1, bad
    # the general query keeps refusing kind 7 (tests/test_logistic_cpu.py pins it too)
    assert L.l2hmc_train_fused_lds_bytes(_ffi.ENERGY_LOGISTIC, 100, 5, 10, 10) == -2


def test_training_entry_argument_errors_on_the_host():
    L = _ffi.lib()
    fake = 0x1000                                                   # never dereferenced: the checks come first

    def args(d=5, **kw):
        e = dict(kind=_ffi.ENERGY_LOGISTIC, n_comp=100, mu=fake, prec=None, logc=None, eta=1.0, easy=0, temperature=1.0,
                 anneal_beta=0.0, den=0.0, reserved_=0)
        e.update(kw)
        a = _ffi.L2hmcTrainArgs()
        net = _ffi.L2hmcNet(*[fake] * len(_ffi.NET_FIELDS))
        a.xnet, a.vnet = ctypes.pointer(net), ctypes.pointer(net)
        a.energy = _ffi.L2hmcEnergy(**e)
        a.masks = a.trig = a.x = a.v = a.Lx = a.p = a.v1 = a.grad = a.workspace = fake
        a.alpha, a.eps_host = None, 0.1
        a.n_chains, a.d, a.H, a.T = 16, d, 10, 4
        a.direction, a.direction_all = None, 1
        a.scale, a.inv_n = 0.1, 1.0 / 16
        return a, net
    for (a, keep), msg in ((args(eta=0.0), b"eta"), (args(eta=-1.0), b"eta"), (args(eta=float("inf")), b"eta"),
                           (args(mu=None), b"packed data"), (args(n_comp=0), b"n_comp"), (args(n_comp=(1 << 20) + 1), b"n_comp"),
                           (args(d=129), b"d <= 128")):
        assert L.l2hmc_train_propose_grad(a, None) == -1, msg
        assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()
    st = _ffi.L2hmcTrainStep()
    a, keep = args(eta=0.0)
    assert L.l2hmc_train_step(a, st, None) == -1 and b"eta" in L.l2hmc_last_error()
    # a shape beyond the plan: refused with the bytes before anything is launched
    a, keep = args(d=128)
    a.T = 10
    assert L.l2hmc_train_propose_grad(a, None) == -2
    assert str(plan_bytes(128, 10, 10)).encode() in L.l2hmc_last_error()
    # the temperature / anneal_beta rules of the other kinds hold for this one
    a, keep = args(temperature=0.0)
    assert L.l2hmc_train_propose_grad(a, None) == -1 and b"temperature" in L.l2hmc_last_error()
    a, keep = args(anneal_beta=0.5)
    assert L.l2hmc_train_propose_grad(a, None) == -2 and b"annealed" in L.l2hmc_last_error()


class _FakeDynamics(object):                                        # the fields the trainers read before any GPU work
    _user_nets = _user = _split = False
    hmc, anneal_beta, x_dim, H, T = False, 0.0, 3, 10, 10
    use_temperature, temperature = False, 1.0


def _logistic_fn(d=3):
    return LogisticRegression(np.eye(d), (np.arange(d) % 2).astype(np.float64)).get_energy_function()


def test_logistic_trainer_is_exported_and_refuses_what_it_does_not_train():
    from l2hmc_amd import distributions as D
    from l2hmc_amd.training import LogisticTrainer, Trainer
    assert l2hmc_amd.LogisticTrainer is LogisticTrainer and "LogisticTrainer" in l2hmc_amd.__all__
    assert issubclass(LogisticTrainer, Trainer)

    class Rough(_FakeDynamics):
        _fn = D.RoughWell(3, 0.1, easy=True).get_energy_function()
    with pytest.raises(NotImplementedError, match="LogisticRegression"):
        LogisticTrainer(Rough())

    class Hmc(_FakeDynamics):
        hmc = True
        _fn = _logistic_fn()
    with pytest.raises(ValueError, match="nothing to train"):
        LogisticTrainer(Hmc())

    class Annealed(_FakeDynamics):
        anneal_beta = 0.5
        _fn = _logistic_fn()
    with pytest.raises(NotImplementedError, match="anneal"):
        LogisticTrainer(Annealed())

    class Wide(_FakeDynamics):                                      # nets wider than H = 15 run on the GEMM engine
        _split, H = True, 24
        _fn = _logistic_fn()
    with pytest.raises(NotImplementedError, match="H <= 15"):
        LogisticTrainer(Wide())

    class Big(_FakeDynamics):                                       # beyond the LDS plan: shape, bytes and the other route
        x_dim = 128
        _fn = _logistic_fn(128)
    with pytest.raises(NotImplementedError, match="torch callable") as ei:
        LogisticTrainer(Big())
    msg = str(ei.value)
    assert "d = 128" in msg and "H = 10" in msg and "T = 10" in msg and str(plan_bytes(128, 10, 10)) in msg and "state_dict" in msg


def test_trainer_names_the_logistic_trainer_first():
    from l2hmc_amd.training import SplitTrainer, Trainer

    class Dyn(_FakeDynamics):
        _fn = _logistic_fn()
    for cls in (Trainer, SplitTrainer):
        with pytest.raises(NotImplementedError, match="torch callable") as ei:
            cls(Dyn())
        msg = str(ei.value)
        assert "state_dict" in msg and "LogisticTrainer" in msg and msg.index("LogisticTrainer") < msg.index("torch callable")


def test_the_logistic_training_kernel_uses_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources.resources()
    if "train.s" not in res:
        pytest.skip("no listings (l2hmc_amd/csrc/build/asm): run `make -C l2hmc_amd/csrc`")
    for f in ("train.s", "train_ilp.s"):
        if f not in res:
            continue
        rows = {k: (vg, sc) for k, vg, sc, _ in res[f]}
        for name in ("train_kernel<false, true>", "train_kernel<true, true>"):      # <TEMP, LOGI>
            assert name in rows, (f, sorted(k for k in rows if k.startswith("train_kernel")))
            assert rows[name][1] == 0 and rows[name][0] <= 512, (f, name, rows[name])
        # (the general kernel's own instantiations are still there, without scratch)
        for name in ("train_kernel<false, false>", "train_kernel<true, false>"):
            assert rows[name][1] == 0, (f, name, rows[name])


# ---- the oracle target ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 2), (17, 5), (200, 25)])
def test_oracle_target_derivatives_by_central_differences(n, d):
    X, y = blr_data(n, d)
    t = LogisticTarget(X, y, PRIOR_VAR, np.float64)
    rng = np.random.RandomState(n + d)
    w, u = 0.7 * rng.randn(6, d), rng.randn(6, d)
    h = 1e-5
    # grad by central differences of energy, one coordinate at a time
    g = t.grad(w)
    fd = np.zeros_like(w)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        fd[:, k] = (t.energy(w + e) - t.energy(w - e)) / (2 * h)
    assert np.abs(fd - g).max() < 1e-7 * max(1.0, np.abs(g).max())
    # hessvec by central differences of grad along u (error O(h^2 |u|^3 |U'''|))
    hv = t.hessvec(w, u)
    fd = (t.grad(w + h * u) - t.grad(w - h * u)) / (2 * h)
    assert np.abs(fd - hv).max() < 1e-7 * max(1.0, np.abs(hv).max())
    # and the closed forms the kernel implements
    L_ = w @ X.astype(np.float64).T
    s = 1.0 / (1.0 + np.exp(-L_))
    assert np.allclose(hv, (s * (1 - s) * (u @ X.T.astype(np.float64))) @ X + u / PRIOR_VAR, rtol=1e-12, atol=1e-12)
    assert np.allclose(t.energy(w), -LogisticRegression(X, y, PRIOR_VAR).log_density(w), rtol=1e-12)
    # float32 instance: the yardstick of the GPU gates is this arithmetic
    t32 = LogisticTarget(X, y, PRIOR_VAR, np.float32)
    assert t32.grad(w.astype(np.float32)).dtype == np.float32 and t32.hessvec(w.astype(np.float32), u.astype(np.float32)).dtype == np.float32
    assert np.abs(t32.hessvec(w.astype(np.float32), u.astype(np.float32)) - hv).max() < 1e-5 * max(1.0, np.abs(hv).max())
