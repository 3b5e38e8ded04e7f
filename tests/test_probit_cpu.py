"""CPU: binomial regression with the probit link (`ProbitRegression`; L2HMC_ENERGY_PROBIT = 10, L2HMC_GLM_PROBIT = 6) as far as it
goes without a GPU -- the definitions on the float64 host route, the slow-path energy with its gradient and Hessian-vector
product, the ABI numbers and every refusal of the library (nothing is launched: every call is refused before it touches a
device), the recorded constants of tests/probit_case.py against fresh measurements, its bounds held against the float32 numpy
restatement of the device sequence, and the registers of the new kernels from the compiler's listing."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from l2hmc_amd import BinomialRegression, ProbitRegression, _ffi, glm
from l2hmc_amd import distributions as D
from tests import glm_case as gc
from tests import probit_case as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096              # a non-NULL "device pointer" for calls that are refused before anything reads it


# ---- 1. definitions, float64 host route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 37])
def test_log_lik_sums_to_one_over_the_responses(m):
    rng = np.random.RandomState(m)
    x = rng.randn(3)
    X, y = np.tile(x, (m + 1, 1)), np.arange(m + 1.0)
    model = ProbitRegression(X, y, m, offset=np.full(m + 1, 0.3))
    W = rng.randn(6, 3)
    ll = model.log_lik(W)
    assert ll.dtype == np.float64 and ll.shape == (6, m + 1)
    assert np.max(np.abs(np.exp(ll).sum(axis=1) - 1.0)) < 1e-12
    p = pc.Phi((W @ x.astype(np.float32).astype(np.float64)) + np.float32(0.3).astype(np.float64))
    assert np.max(np.abs(model.predict_mean(W) - m * p.mean())) < 1e-12 * m


def test_host_route_is_the_restatement():
    """`log_density`, `log_lik`, `predict_mean`, `waic` and `loo` on numpy draws (torch.special.log_ndtr in float64) against the
    scipy restatement of tests/probit_case.py; binary probit is trials = 1, the default."""
    from l2hmc_amd import psis
    c = pc.case(70, 33, 17)
    model = pc.model(c, prior_var=pc.PRIOR_VAR)
    assert isinstance(model._glm.lik, glm.Probit) and model._glm.family == _ffi.GLM_PROBIT == 6 and model._glm.consts.shape == (4, 33)
    ll64, t = pc.log_lik(c)
    assert np.max(np.abs(model.log_lik(c["W"]) - ll64)) < 1e-12 * np.max(np.abs(ll64))
    assert np.max(np.abs(model.log_lik(c["W"], rows=(17, 33)) - ll64[:, 17:])) < 1e-12 * np.max(np.abs(ll64))
    U, _ = pc.energy(c)
    assert np.max(np.abs(-model.log_density(c["W"]) - U)) < 1e-12 * np.max(np.abs(U))
    ref = pc.restatement(c)
    assert np.max(np.abs(model.predict_mean(c["W"]) - ref["mean_mu"])) < 1e-12 * ref["mean_mu"].max()
    w = model.waic(c["W"])
    assert np.max(np.abs(w.lppd_i - ref["lppd_i"])) < 1e-10 and np.max(np.abs(w.p_waic_i - ref["p_waic_i"])) < 1e-10
    got, want = model.loo(c["W"]), psis.loo_from_log_lik(ll64)
    assert np.max(np.abs(got.elpd_loo_i - want.elpd_loo_i)) < 1e-9 and np.allclose(got.khat, want.khat, atol=1e-7, equal_nan=True)
    # the row constants are the binomial's, rounded once, in the rows the header names
    o, m, k = pc.terms(c)
    for row, v in enumerate((o, m, pc.saturated(c), k)):
        assert np.array_equal(model._glm.consts[row], v.astype(np.float32)), row
    assert np.array_equal(model._glm.consts, BinomialRegression(c["X"], c["y"], c["trials"], offset=c["offset"])._glm.consts)
    sat = pc.saturated(c)
    assert np.all(ll64 <= sat + 1e-12 * np.abs(sat))
    b1 = ProbitRegression(c["X"], (c["y"] > 0).astype(np.float32))
    assert np.array_equal(b1.trials, np.ones(33, dtype=np.float32))


def test_host_route_keeps_both_tails():
    """EDGE on the host: the float64 restatement and the library's host route are finite at t = +-30 (a log of 0.5 erfc is -inf
    from t = -38 in float64 and from t = -14 in float32; 1 - Phi is 0 from t = 8.3), and they agree."""
    c = pc.EDGE
    ll64, t = pc.log_lik(c)
    assert np.all(np.isfinite(ll64)) and np.abs(t).max() > 29.5 and ll64.min() < -22000.0
    got = pc.model(c).log_lik(c["W"])
    assert np.all(np.isfinite(got)) and np.max(np.abs(got - ll64) / np.maximum(np.abs(ll64), 1e-300)) < 1e-11


def test_arguments_are_checked():
    X, y = np.zeros((4, 2)), np.array([0.0, 1.0, 2.0, 3.0])
    for bad in (0, 2, 2.5, (1 << 24) + 1, [3, 3, 3], np.nan):
        with pytest.raises(ValueError, match="trials"):
            ProbitRegression(X, y, bad)
    with pytest.raises(ValueError, match="successes y"):
        ProbitRegression(X, y)                                   # trials = 1: y must be 0 or 1
    assert np.array_equal(ProbitRegression(X, y, 3).trials, np.full(4, 3.0, dtype=np.float32))
    with pytest.raises(ValueError, match="ProbitRegression supports d <= 128"):
        ProbitRegression(np.zeros((4, 129)), y, 3)
    with pytest.raises(ValueError, match="offset"):
        ProbitRegression(X, y, 3, offset=np.zeros(3))
    with pytest.raises(ValueError, match="prior_var"):
        ProbitRegression(X, y, 3, prior_var=0.0)


def test_slow_path_energy_gradient_and_hessian_vector_product():
    """The torch energy against the definition, its analytic gradient against autograd and the definition, and the
    Hessian-vector product (autograd through the analytic gradient, what a trainer takes) against a central difference of the
    gradient, float64."""
    import torch
    c = pc.case(8, 37, 3)
    model = pc.model(c, prior_var=pc.PRIOR_VAR)
    x = torch.as_tensor(c["W"].astype(np.float64))
    U, G = pc.energy(c)
    assert np.max(np.abs(model.energy(x).numpy() - U)) < 1e-12 * np.max(np.abs(U))
    assert np.max(np.abs(model.grad_energy(x).numpy() - G)) < 1e-12 * np.max(np.abs(G))
    xr = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(model.energy(xr).sum(), xr)
    assert np.max(np.abs(g.numpy() - G)) < 1e-10 * np.max(np.abs(G))
    u = torch.as_tensor(np.random.RandomState(1).randn(*x.shape))
    xr = x.clone().requires_grad_(True)
    hv, = torch.autograd.grad((model.grad_energy(xr) * u).sum(), xr)
    h = 1e-5
    fd = (model.grad_energy(x + h * u) - model.grad_energy(x - h * u)) / (2 * h)
    assert np.max(np.abs(hv.numpy() - fd.numpy())) < 1e-7 * np.max(np.abs(fd.numpy()))
    # ... and in the tails (EDGE): finite, and the gradient is the definition's
    e = pc.EDGE
    me = pc.model(e, prior_var=pc.PRIOR_VAR)
    xe = torch.as_tensor(e["W"][:5].astype(np.float64))
    Ue, Ge = pc.energy(e, e["W"][:5])
    assert np.max(np.abs(me.energy(xe).numpy() - Ue)) < 1e-11 * np.max(np.abs(Ue))
    assert np.max(np.abs(me.grad_energy(xe).numpy() - Ge)) < 1e-11 * np.max(np.abs(Ge))
    # float32, as the slow path runs: finite in the tails
    x32 = torch.as_tensor(e["W"][:5])
    assert torch.isfinite(me.energy(x32)).all() and torch.isfinite(me.grad_energy(x32)).all()
    Uf, Gf = me.energy(x32).numpy(), me.grad_energy(x32).numpy()
    assert np.max(np.abs(Uf - Ue)) < 1e-5 * np.max(np.abs(Ue)) and np.max(np.abs(Gf - Ge)) < 1e-4 * np.max(np.abs(Ge))
    slow = me.get_energy_function()
    assert slow.fn == me.energy and slow.grad_fn == me.grad_energy


# ---- 2. the ABI without a GPU ------------------------------------------------------------------------------------------------
def test_numbers_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    for name, value in (("L2HMC_ENERGY_PROBIT", _ffi.ENERGY_PROBIT), ("L2HMC_GLM_PROBIT", _ffi.GLM_PROBIT)):
        m = re.search(r"%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (_ffi.ENERGY_PROBIT, _ffi.GLM_PROBIT) == (10, 6)
    assert re.search(r"#define\s+L2HMC_ABI_VERSION\s+6\b", header) and _ffi.ABI_VERSION == 6
    assert ctypes.sizeof(_ffi.L2hmcEnergy) == 56


def test_both_forms_of_the_energy_function():
    c = pc.case(4, 37, 3)
    model = pc.model(c, prior_var=2.5)
    slow = model.get_energy_function()
    assert type(slow) is D.UserEnergy and slow.kind == D.ENERGY_USER
    e = model.get_energy_function(fused=True)
    assert type(e) is D.ProbitEnergy and isinstance(e, D.BinomialEnergy)
    assert e.kind == _ffi.ENERGY_PROBIT == 10 and e.n_comp == 37 and e.eta == 2.5 and e.x_dim == 3
    o, m, _ = pc.terms(c)
    assert np.array_equal(e._host["offset"], o.astype(np.float32)) and np.array_equal(e._host["weight"], m.astype(np.float32))
    # the binomial keeps its kind
    b = BinomialRegression(c["X"], c["y"], c["trials"]).get_energy_function(fused=True)
    assert type(b) is D.BinomialEnergy and b.kind == _ffi.ENERGY_BINOMIAL == 9


def _energy(kind=10, n=100, mu=FAKE, prec=FAKE, eta=2.0):
    return _ffi.L2hmcEnergy(kind, n, mu, prec, None, eta, 0, 1.0, 0.0, 0.0, 0)


def _traj(e, d):
    a = _ffi.L2hmcTrajectoryArgs()
    a.energy = e
    a.n_chains, a.d, a.T, a.n_steps, a.eps_host = 16, d, 5, 5, 0.1
    a.x = a.v = a.masks = a.trig = FAKE
    return a


@pytest.mark.parametrize("kw,d,msg", [
    ({"prec": None}, 5, b"probit regression needs the offsets and trials (prec: l2hmc_binomial_aux_floats(n_data) floats"),
    ({"mu": None}, 5, b"probit regression needs the packed data (mu, l2hmc_pack_logistic with the successes as labels)"),
    ({}, 129, b"probit regression supports d <= 128 (got 129)"),
    ({"eta": 0.0}, 5, b"probit regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"eta": float("inf")}, 5, b"probit regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"eta": float("nan")}, 5, b"probit regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"n": 0}, 5, b"probit regression needs 1 <= n_comp = n_data <= 1048576 (got 0)"),
    ({"n": (1 << 20) + 1}, 5, b"probit regression needs 1 <= n_comp = n_data <= 1048576 (got 1048577)"),
])
def test_energy_and_trajectory_refuse_bad_arguments_without_a_gpu(kw, d, msg):
    L = _ffi.lib()
    e = _energy(**kw)
    assert L.l2hmc_energy(e, FAKE, 16, d, None, None, None) == -1
    assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()
    assert L.l2hmc_trajectory(_traj(e, d), None) == -1
    assert msg in L.l2hmc_last_error(), L.l2hmc_last_error()


def test_training_entry_points_name_the_other_route():
    L = _ffi.lib()
    route = (b"train on the slow path", b"load_state_dict")
    assert L.l2hmc_train_fused_lds_bytes(10, 100, 5, 10, 5) == -2
    assert b"probit-regression target" in L.l2hmc_last_error() and all(r in L.l2hmc_last_error() for r in route)
    a = _ffi.L2hmcTrainArgs()
    a.energy = _energy()
    a.n_chains, a.d, a.H, a.T, a.eps_host, a.scale, a.inv_n = 16, 5, 10, 5, 0.1, 0.1, 1.0 / 16
    net = _ffi.L2hmcNet(*([FAKE] * 16))
    a.xnet = a.vnet = ctypes.pointer(net)
    for k in ("masks", "trig", "x", "v", "Lx", "p", "v1", "grad", "workspace"):
        setattr(a, k, FAKE)
    assert L.l2hmc_train_propose_grad(a, None) == -2
    assert b"probit-regression target" in L.l2hmc_last_error() and all(r in L.l2hmc_last_error() for r in route)
    s = _ffi.L2hmcTrainSplitArgs()
    e = _energy()
    s.energy = ctypes.pointer(e)
    s.n_chains, s.d, s.T, s.H = 16, 5, 5, 10
    rc = L.l2hmc_train_split_grad(s, None)
    assert rc == -2, (rc, L.l2hmc_last_error())
    assert b"probit-regression target" in L.l2hmc_last_error() and all(r in L.l2hmc_last_error() for r in route)


def test_trainers_refuse_the_fused_energy_and_name_the_slow_path():
    from l2hmc_amd.training import LogisticTrainer, SplitTrainer, Trainer

    class Dyn(object):                      # what Trainer.__new__ reads before anything else
        pass
    dyn = Dyn()
    dyn._fn = pc.model(pc.case(4, 37, 3)).get_energy_function(fused=True)
    for cls in (Trainer, SplitTrainer, LogisticTrainer):
        with pytest.raises(NotImplementedError, match=r"probit.*get_energy_function\(\)") as ei:
            cls(dyn)
        assert "load_state_dict" in str(ei.value) and "slow path" in str(ei.value)


def test_glm_entries_take_the_probit_family():
    L = _ffi.lib()
    ok = 1 << 12

    def loglik(S=100, d=3, n=10, fam=6):
        return L.l2hmc_glm_log_lik(ok, S, d, ok, ok, n, fam, ok, None)

    def predict(S=100, d=3, n=10, fam=6):
        return L.l2hmc_glm_predict(ok, S, d, ok, ok, n, fam, ok, ok, None)

    def tails(S=100, d=3, n=10, fam=6):
        return L.l2hmc_glm_loo_tails(ok, S, d, ok, ok, n, fam, None, 10, ok, ok, ok, ok, ok, ok, None)

    for fn in (loglik, predict, tails):
        assert fn(d=129) == -1 and b"<= d <= 128" in L.l2hmc_last_error(), (fn.__name__, L.l2hmc_last_error())
        assert fn(S=1) == -1 and b"n_draws >= 2" in L.l2hmc_last_error()
        for fam in (5, 7, 8):
            assert fn(fam=fam) == -1 and b"unknown family" in L.l2hmc_last_error() and b"L2HMC_GLM_PROBIT = 6" in L.l2hmc_last_error()


# ---- 3. the recorded constants ---------------------------------------------------------------------------------------------------
def test_recorded_erfcx_error_covers_a_fresh_measurement():
    """ERFCX_ULPS against the float32 sequence re-measured on a coarser grid than the one that set it (1 000 003 points of
    [0, 64], the reciprocal correctly rounded and one ulp either way), and on a logarithmic grid to 1e19; the coefficients are
    the ones ProbitLink holds."""
    from scipy.special import erfcx
    lo, hi, points = pc.ERFCX_GRID
    assert (lo, hi) == (0.0, 64.0) and points > 1000003
    src = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "l2hmc_kernels.hpp")).read()
    body = src[src.index("struct ProbitLink"):]
    body = body[body.index("float p = fmaf("):body.index("E = __fmul_rn(p, u)")]
    lits = [np.float32(v) for line in body.splitlines() for v in re.findall(r"(-?\d[\d.]*(?:e[+-]?\d+)?)f\b", line.split("//")[0])]
    assert lits == [np.float32(v) for v in pc.ERFCX_COEF], lits
    worst = 0.0
    for xs in (np.linspace(lo, hi, 1000003).astype(np.float32), np.logspace(np.log10(64.0), 19.0, 100001).astype(np.float32)):
        ref = erfcx(xs.astype(np.float64))
        for nudge in (0, -1, 1):
            worst = max(worst, float(np.max(np.abs(pc.erfcx32(xs, nudge).astype(np.float64) - ref) / ref)) / pc.EPS)
    print("erfcx: worst relative error %.3f u (recorded %.1f)" % (worst, pc.ERFCX_ULPS))
    assert worst <= pc.ERFCX_ULPS


def test_recorded_gates_are_four_times_the_measured_sensitivities():
    """The K_* of tests/probit_case.py against a fresh measurement on the two cheapest cases that set them (the whole table is
    tools/probit_accuracy.py's)."""
    assert pc.SHAPES == gc.SHAPES[:7] and pc.GEOM_SHAPES == gc.SHAPES[7:]
    for S, n, d in ((25, 1, 1), (70, 33, 17)):
        k = pc.sensitivity(pc.case(S, n, d))
        for got, K in zip(k, (pc.K_KHAT, pc.K_ELPD, pc.K_NEFF, pc.K_MCSE)):
            assert 4.0 * got <= K * (1 + 1e-9), (S, n, d, k)


# ---- 4. bounds -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(17, 5), (1000, 25)])
def test_bounds_hold_for_the_float32_restatement(n, d):
    c = pc.case(40, n, d)
    W = c["W"]
    U, G = pc.energy(c)
    U32, G32 = pc.energy(c, dtype=np.float32)
    b = pc.bounds(c)
    sU, sg = pc.used(U32, G32, U, G, b)
    ll, lb = pc.log_lik(c)[0], pc.ll_bounds(c)
    sl = float(np.max(np.abs(pc.log_lik32(c).astype(np.float64) - ll) / lb["B"]))
    print("n=%d d=%d: float32 numpy uses %.3f of the U bound, %.3f of the grad U bound, %.3f of the ll bound" % (n, d, sU, sg, sl))
    assert sU <= 1.0 and sg <= 1.0 and sl <= 1.0
    assert np.all(b["U"] < 1e-3 * np.abs(U).max()) and np.all(b["g"] < 1e-3 * np.abs(G).max() + 1e-3)     # (they bind)
    assert np.all(lb["B"] < 1e-3 * max(1.0, np.abs(ll).max()))
    for T, beta in ((2.5, 1.0), (1.0, 0.3)):
        Us, Gs, bs = pc.scaled(c, temperature=T, beta=beta)
        q = np.float32(0.5) * (W * W).sum(axis=1)
        Ub = (np.float32(1 - beta) * q + np.float32(beta) * U32) / np.float32(T)
        Gb = (np.float32(1 - beta) * W + np.float32(beta) * G32) / np.float32(T)
        sU, sg = pc.used(Ub, Gb, Us, Gs, bs)
        assert sU <= 1.0 and sg <= 1.0, (T, beta, sU, sg)
        assert np.all(bs["U"] < 1e-3 * np.abs(Us).max())


@pytest.mark.parametrize("S,n,d", pc.SHAPES + pc.GEOM_SHAPES + pc.LONG)
def test_statistics_cases_are_bound(S, n, d):
    """Every shape of the statistics and geometry tests: the float32 restatement is inside B and Bmean element by element, and
    exp(ll - sat) sums to more than 0 in every row."""
    c = pc.case(S, n, d)
    ll, t = pc.log_lik(c)
    b = pc.ll_bounds(c)
    share = float(np.max(np.abs(pc.log_lik32(c).astype(np.float64) - ll) / b["B"]))
    o, m, _ = pc.terms(c)
    t32 = (c["W"] @ c["X"].T + o.astype(np.float32)).astype(np.float32)
    mean32 = (m.astype(np.float32) * pc.link32(t32, c["y"], m)["Phi"]).astype(np.float32)
    sm = float(np.max(np.abs(mean32.astype(np.float64) - pc.mean_of(c, t)) / b["Bmean"]))
    print("(%d, %d, %d): float32 numpy uses %.3g of the ll bound, %.3g of the mean bound" % (S, n, d, share, sm))
    assert share <= 1.0 and sm <= 1.0
    assert np.all(np.exp(ll - pc.saturated(c)).sum(axis=0) > 0.0)


def test_the_bounds_see_a_wrong_link():
    """an energy that counts one padded row (log Phi(0) at a weight of 1), reads the trials of the next row, drops the offsets,
    or loses one ulp-sized part in 1e4 of log Phi is outside the bounds"""
    c = pc.case(40, 17, 5)
    U, G = pc.energy(c)
    b = pc.bounds(c)
    assert pc.used(U + np.log(2.0), G, U, G, b)[0] > 1.0
    wrong = dict(c)
    wrong["trials"] = np.roll(c["trials"], 1)
    wrong["y"] = np.minimum(c["y"], wrong["trials"])
    Uw, Gw = pc.energy(wrong)
    assert min(pc.used(Uw, Gw, U, G, b)) > 1.0
    wrong = dict(c)
    wrong["offset"] = np.zeros_like(c["offset"])
    Uw, Gw = pc.energy(wrong)
    assert min(pc.used(Uw, Gw, U, G, b)) > 1.0
    assert pc.used(U * (1 + 1e-4), G * (1 + 1e-4), U, G, b) > (1.0, 1.0)


def test_edge_rows_are_finite_and_bound():
    """EDGE: t near 0, +-5, +-9, +-15, +-30 with y = 0, y = m and 0 < y < m at m = 50.  The float64 restatement is finite; the
    bounds stay below 1e-3 of |ll| (of 1e-32 where |ll| is below the float32 range: t = 15 and 30 on the sure side), of |U| and
    of the gradient's scale; the float32 restatement is finite and inside them; a log of 0.5 erfc would not be."""
    from scipy.special import erfc
    c = pc.EDGE
    ll, t = pc.log_lik(c)
    assert c["X"].shape == (27, 3) and np.all(c["trials"] == 50.0)
    for j, tau in enumerate(pc.EDGE_TAUS):
        assert np.all(np.abs(t[:, 3 * j:3 * j + 3] - tau) < 0.31) and c["y"][3 * j:3 * j + 3].tolist() == [0.0, 50.0, 23.0]
    assert np.all(np.isfinite(ll))
    b = pc.ll_bounds(c)
    assert np.all(b["B"] < 1e-3 * np.maximum(np.abs(ll), 1e-32))
    ll32 = pc.log_lik32(c)
    assert np.all(np.isfinite(ll32))
    share = float(np.max(np.abs(ll32.astype(np.float64) - ll) / b["B"]))
    U, G = pc.energy(c)
    U32, G32 = pc.energy(c, dtype=np.float32)
    bu = pc.bounds(c)
    sU, sg = pc.used(U32, G32, U, G, bu)
    print("EDGE: float32 numpy uses %.3f of the ll bound, %.3f of the U bound, %.3f of the grad U bound" % (share, sU, sg))
    assert share <= 1.0 and sU <= 1.0 and sg <= 1.0 and np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
    assert np.all(bu["U"] < 1e-3 * np.abs(U)) and np.all(bu["g"] < 1e-3 * np.abs(G).max())
    with np.errstate(all="ignore"):
        naive = np.log(np.float32(0.5) * erfc(-t.astype(np.float32) / np.float32(np.sqrt(2.0))).astype(np.float32))
    assert np.isneginf(naive).any()


def test_trajectory_step_sizes_come_from_the_oracle():
    """The oracle trajectories of TRAJ_CASES (the GPU test relies on it): the step size `traj_case` chose gives a mean accept
    probability in (0.2, 1) and finite states and energies."""
    assert pc.TRAJ_CASES == [(17, 5, 0), (17, 5, 10), (200, 25, 0), (200, 25, 10), (300, 100, 0), (300, 100, 10), (200, 25, 24)]
    for n, d, H in pc.TRAJ_CASES:
        c = pc.traj_case(n, d, H)
        X1, V1, lj, p = c["ref"]["forward"]
        assert 0.2 < float(p.mean()) < 1.0 and np.all(np.isfinite(X1)) and np.all(np.isfinite(V1)) and np.all(np.isfinite(p))
        U1 = pc.energy(c["c"], X1, dtype=np.float32)[0]
        assert np.all(np.isfinite(U1))
        print("n=%d d=%d H=%d: eps %g, oracle accept %.3f, float32-float64 distances %s" % (n, d, H, c["eps"], p.mean(), c["dist"]["forward"]))


# ---- 5. registers ----------------------------------------------------------------------------------------------------------------
def test_new_kernels_have_no_more_scratch_than_their_twins():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): every kernel of
    the kind-10 units against the kind-9 kernel of the same geometry, every glm kernel of family 6 against family 1's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not os.path.isdir(os.path.join(ROOT, "l2hmc_amd", "csrc", "build", "asm")):
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    res = kr.resources()
    if not res.get("traj_ek10.s") or not res.get("glm_probit.s"):
        pytest.skip("no compiler listings of the probit units under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    for new, old in (("traj_ek10.s", "traj_ek9.s"), ("traj_ladder_ek10.s", "traj_ladder_ek9.s")):
        twins = {k: sc for k, _, sc, _ in res[old]}
        rows = res[new]
        assert len(rows) == len(res[old]) and any(k.startswith("traj_") for k, _, _, _ in rows)
        for k, vg, sc, _ in rows:
            twin = re.sub(r"<10, ", "<9, ", k, count=1)
            assert "<10, " in k and twin in twins, (k, sorted(twins))
            print("%-36s %4d registers, %3d bytes of scratch (kind 9: %d)" % (k, vg, sc, twins[twin]))
            assert sc <= twins[twin], (k, sc, twins[twin])
    twins = {}
    for k, _, sc, _ in res["glm.s"]:
        twins[k] = max(sc, twins.get(k, 0))
    shared = ("chunk_reduce_kernel", "radix_advance_kernel")          # (static kernels of shared headers: one copy per unit)
    seen = [k for k, _, _, _ in res["glm_probit.s"] if k not in shared]
    want = ["glm_loo_kernel<%d, %d>" % (g, m) for g in (1, 2, 4, 8) for m in (0, 1)] + ["glm_loglik_kernel<%d>" % g for g in (1, 2, 4, 8)]
    want += ["glm_predict_kernel<%d>" % g for g in (1, 2, 4, 8)]
    assert sorted(seen) == sorted(want), seen
    for k, vg, sc, _ in res["glm_probit.s"]:
        print("%-28s %4d registers, %d bytes of scratch (family 1: %d)" % (k, vg, sc, twins[k]))
        assert sc <= twins[k] and vg <= 256, (k, vg, sc)
