"""CPU: binomial and negative-binomial regression (`BinomialRegression`, `NegativeBinomialRegression`; L2HMC_ENERGY_BINOMIAL = 9,
L2HMC_GLM_BINOMIAL = 3, L2HMC_GLM_NEGBINOMIAL = 4) as far as they go without a GPU -- the definitions on the float64 host route,
the ABI numbers and every refusal of the library (nothing is launched: every call is refused before it touches a device), the
bounds of tests/binomial_case.py held against a float32 numpy restatement, and the registers of the new kernels from the
compiler's listing."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from l2hmc_amd import BinomialRegression, LogisticRegression, NegativeBinomialRegression, PoissonRegression, _ffi, glm
from l2hmc_amd import distributions as D
from tests import binomial_case as bc
from tests import glm_case as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096              # a non-NULL "device pointer" for calls that are refused before anything reads it


# ---- 1. definitions, float64 host route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 37])
def test_binomial_log_lik_sums_to_one_over_the_responses(m):
    rng = np.random.RandomState(m)
    x = rng.randn(3)
    X, y = np.tile(x, (m + 1, 1)), np.arange(m + 1.0)
    model = BinomialRegression(X, y, m, offset=np.full(m + 1, 0.3))
    W = rng.randn(6, 3)
    ll = model.log_lik(W)
    assert ll.dtype == np.float64 and ll.shape == (6, m + 1)
    assert np.max(np.abs(np.exp(ll).sum(axis=1) - 1.0)) < 1e-12
    p = 1.0 / (1.0 + np.exp(-((W @ x.astype(np.float32).astype(np.float64)) + np.float32(0.3).astype(np.float64))))
    assert np.max(np.abs(model.predict_mean(W) - m * p.mean())) < 1e-12 * m


@pytest.mark.parametrize("phi", [0.5, 10.0])
def test_negative_binomial_is_the_direct_pmf_with_its_mean_and_variance(phi):
    from scipy.stats import nbinom
    x, off, Y = np.array([0.4, -0.2]), 0.7, 1500
    X, y = np.tile(x, (Y + 1, 1)), np.arange(Y + 1.0)
    model = NegativeBinomialRegression(X, y, phi, offset=np.full(Y + 1, off))
    W = np.array([[1.0, 0.5], [-0.5, 1.5]])
    ll = model.log_lik(W)
    for s in range(2):
        mu = np.exp(W[s] @ x.astype(np.float32).astype(np.float64) + np.float64(np.float32(off)))
        assert nbinom.sf(Y, phi, phi / (phi + mu)) < 1e-12                       # (truncated where the tail is below 1e-12)
        direct = nbinom.logpmf(y, phi, phi / (phi + mu))
        big = direct > -60.0
        assert np.max(np.abs(ll[s] - direct)[big]) < 1e-11
        pmf = np.exp(ll[s])
        assert abs(pmf.sum() - 1.0) < 1e-11
        mean = (y * pmf).sum()
        var = (np.square(y - mean) * pmf).sum()
        assert abs(mean - mu) < 1e-9 * mu and abs(var - (mu + mu * mu / phi)) < 1e-8 * (mu + mu * mu / phi)
        assert abs(model.predict_mean(W[s:s + 1].repeat(2, axis=0))[0] - mu) < 1e-12 * mu


@pytest.mark.parametrize("kind,phi", [("binomial", None), ("negbinomial", 0.5), ("negbinomial", 10.0)])
def test_sat_is_the_supremum_of_ll(kind, phi):
    c = bc.case(40, 100, 5, kind, phi)
    model = bc.model(c)
    fam, g = model._glm.lik, model._glm
    sat = fam.saturated(c["y"], c["offset"], g.weight)
    assert np.max(np.abs(sat - bc.saturated(c))) < 1e-12 * np.max(np.abs(sat))        # the library's against the restatement
    ll = model.log_lik(c["W"])
    assert np.all(ll <= sat + 1e-12 * np.abs(sat)) and np.all(ll <= 1e-12)
    # ... reached at sigmoid(t) = y / m: draws that put every interior row there
    o, m, k = bc.terms(c)
    y = c["y"].astype(np.float64)
    inner = (y > 0) & (y < m)
    assert inner.sum() >= 10
    t = np.log(y[inner] / (m[inner] - y[inner]))
    at = y[inner] * t - m[inner] * np.logaddexp(0.0, t) + k[inner]
    assert np.max(np.abs(at - sat[inner])) < 1e-12 * np.max(np.abs(sat[inner]))
    # the float32 constants are these, rounded once, in the rows the header names
    assert g.consts.shape == (4, 100) and g.consts.dtype == np.float32
    for row, v in enumerate((o, m, sat, k)):
        assert np.array_equal(g.consts[row], v.astype(np.float32)), row


def test_one_trial_is_logistic_regression():
    from l2hmc_amd import predictive
    rng = np.random.RandomState(2)
    X = rng.randn(60, 4)
    y = (rng.rand(60) < 0.5).astype(np.float64)
    W = 0.3 * rng.randn(200, 4)
    b, lg = BinomialRegression(X, y, 1, prior_var=1.7), LogisticRegression(X, y, prior_var=1.7)
    assert np.max(np.abs(b.log_density(W[:9]) - lg.log_density(W[:9]))) < 1e-12 * np.max(np.abs(lg.log_density(W[:9])))
    bw, lw = b.waic(W), predictive.waic(W, lg.X, lg.y)
    for k in ("elpd_waic", "p_waic", "lppd", "se"):
        assert abs(bw[k] - lw[k]) <= 1e-9 * abs(lw[k]), k
    assert np.max(np.abs(bw.elpd_i - lw.elpd_i) / np.abs(lw.elpd_i)) < 1e-9
    bl, ll = b.loo(W), predictive.loo(W, lg.X, lg.y)
    for k in ("elpd_loo", "p_loo", "looic", "se"):
        assert abs(bl[k] - ll[k]) <= 1e-9 * abs(ll[k]), k
    assert np.max(np.abs(bl.khat - ll.khat)) < 1e-9 * max(1.0, np.max(np.abs(ll.khat)))
    assert np.max(np.abs(bl.elpd_loo_i - ll.elpd_loo_i) / np.abs(ll.elpd_loo_i)) < 1e-9


def test_arguments_are_checked():
    X, y = np.zeros((4, 2)), np.array([0.0, 1.0, 2.0, 3.0])
    for bad in (0, 2, 2.5, (1 << 24) + 1, [3, 3, 3], np.nan):
        with pytest.raises(ValueError, match="trials"):
            BinomialRegression(X, y, bad)
    with pytest.raises(ValueError, match="successes y"):
        BinomialRegression(X, np.array([0.0, 1.5, 2.0, 3.0]), 3)
    assert np.array_equal(BinomialRegression(X, y, 3).trials, np.full(4, 3.0, dtype=np.float32))       # a scalar broadcasts
    assert np.array_equal(BinomialRegression(X, y, [3, 4, 5, 1 << 24]).trials, np.array([3, 4, 5, 1 << 24], dtype=np.float32))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="dispersion"):
            NegativeBinomialRegression(X, y, bad)
    with pytest.raises(ValueError, match="counts y"):
        NegativeBinomialRegression(X, -y, 1.0)
    for cls, arg in ((BinomialRegression, 3), (NegativeBinomialRegression, 1.0)):
        with pytest.raises(ValueError, match="d <= 128"):
            cls(np.zeros((4, 129)), y, arg)
        with pytest.raises(ValueError, match="offset"):
            cls(X, y, arg, offset=np.zeros(3))
        with pytest.raises(ValueError, match="prior_var"):
            cls(X, y, arg, prior_var=0.0)
    with pytest.raises(ValueError, match="trials"):
        BinomialRegression(X, y, 3).predict_mean(np.zeros((5, 2)), X=X, trials=0)


def test_poisson_results_are_what_the_family_object_gives():
    """`Glm` takes its family as an object; the Poisson model's numbers are those of the definition, as before."""
    from tests import glm_case as gc
    W, X, y, o = gc.case(70, 33, 3)
    m = PoissonRegression(X, y, offset=o)
    assert isinstance(m._glm.lik, glm.Poisson) and m._glm.family == _ffi.GLM_POISSON == 1 and m._glm.consts.shape == (3, 33)
    assert np.array_equal(m._glm.consts, glm.row_constants(y, o))
    ll64, h = gc.log_lik(W, X, y, o)
    assert np.max(np.abs(m.log_lik(W) - ll64)) < 1e-12 * np.max(np.abs(ll64))
    assert np.max(np.abs(m.predict_mean(W) - np.exp(h).mean(axis=0))) < 1e-12 * np.exp(h).max()


def test_torch_energy_is_the_definition():
    import torch
    for kind, phi in (("binomial", None), ("negbinomial", 0.5)):
        c = bc.case(8, 37, 3, kind, phi)
        model = bc.model(c, prior_var=bc.PRIOR_VAR)
        x = torch.as_tensor(c["W"].astype(np.float64))
        U, G = bc.energy(c)
        assert np.max(np.abs(model.energy(x).numpy() - U)) < 1e-6 * np.max(np.abs(U))       # (o and m are the float32 constants)
        assert np.max(np.abs(model.grad_energy(x).numpy() - G)) < 1e-6 * np.max(np.abs(G))
        assert np.max(np.abs(-model.log_density(c["W"]) - U)) < 1e-12 * np.max(np.abs(U))
        xr = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(model.energy(xr).sum(), xr)
        assert np.max(np.abs(g.numpy() - model.grad_energy(x).numpy())) < 1e-10 * np.max(np.abs(G))


# ---- 2. the ABI without a GPU ------------------------------------------------------------------------------------------------
def test_numbers_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    for name, value in (("L2HMC_ENERGY_BINOMIAL", _ffi.ENERGY_BINOMIAL), ("L2HMC_GLM_BINOMIAL", _ffi.GLM_BINOMIAL),
                        ("L2HMC_GLM_NEGBINOMIAL", _ffi.GLM_NEGBINOMIAL)):
        m = re.search(r"%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (_ffi.ENERGY_BINOMIAL, _ffi.GLM_BINOMIAL, _ffi.GLM_NEGBINOMIAL) == (9, 3, 4)
    assert re.search(r"#define\s+L2HMC_ABI_VERSION\s+6\b", header) and _ffi.ABI_VERSION == 6
    assert "l2hmc_binomial_aux_floats" in header and "l2hmc_binomial_aux_floats" in _ffi.SYMBOLS
    assert ctypes.sizeof(_ffi.L2hmcEnergy) == 56


def test_aux_size_query():
    L = _ffi.lib()
    assert [L.l2hmc_binomial_aux_floats(n) for n in (1, 16, 17, 1000, 1 << 20)] == [32, 32, 64, 2016, 1 << 21]
    assert L.l2hmc_binomial_aux_floats(0) == -1 and b"binomial regression" in L.l2hmc_last_error()
    assert L.l2hmc_binomial_aux_floats((1 << 20) + 1) == -1


def test_both_forms_of_the_energy_function():
    for kind, phi in (("binomial", None), ("negbinomial", 10.0)):
        c = bc.case(4, 37, 3, kind, phi)
        model = bc.model(c, prior_var=2.5)
        slow = model.get_energy_function()
        assert type(slow) is D.UserEnergy and slow.kind == D.ENERGY_USER
        e = model.get_energy_function(fused=True)
        assert type(e) is D.BinomialEnergy and isinstance(e, D.EnergyFunction)
        assert e.kind == _ffi.ENERGY_BINOMIAL == 9 and e.n_comp == 37 and e.eta == 2.5 and e.x_dim == 3
        o, m, _ = bc.terms(c)
        assert np.array_equal(e._host["offset"], o.astype(np.float32)) and np.array_equal(e._host["weight"], m.astype(np.float32))


def _energy(kind=9, n=100, mu=FAKE, prec=FAKE, eta=2.0):
    return _ffi.L2hmcEnergy(kind, n, mu, prec, None, eta, 0, 1.0, 0.0, 0.0, 0)


def _traj(e, d):
    a = _ffi.L2hmcTrajectoryArgs()
    a.energy = e
    a.n_chains, a.d, a.T, a.n_steps, a.eps_host = 16, d, 5, 5, 0.1
    a.x = a.v = a.masks = a.trig = FAKE
    return a


@pytest.mark.parametrize("kw,d,msg", [
    ({"prec": None}, 5, b"binomial regression needs the offsets and weights (prec: l2hmc_binomial_aux_floats(n_data) floats"),
    ({"mu": None}, 5, b"binomial regression needs the packed data (mu, l2hmc_pack_logistic with the responses as labels)"),
    ({}, 129, b"binomial regression supports d <= 128 (got 129)"),
    ({"eta": 0.0}, 5, b"binomial regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"eta": float("inf")}, 5, b"binomial regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"eta": float("nan")}, 5, b"binomial regression needs eta = prior variance sigma^2 > 0 and finite"),
    ({"n": 0}, 5, b"binomial regression needs 1 <= n_comp = n_data <= 1048576 (got 0)"),
    ({"n": (1 << 20) + 1}, 5, b"binomial regression needs 1 <= n_comp = n_data <= 1048576 (got 1048577)"),
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
    route = b"train on the same likelihood as a caller-supplied energy"
    assert L.l2hmc_train_fused_lds_bytes(9, 100, 5, 10, 5) == -2
    assert b"binomial / negative-binomial regression target" in L.l2hmc_last_error() and route in L.l2hmc_last_error()
    a = _ffi.L2hmcTrainArgs()
    a.energy = _energy()
    a.n_chains, a.d, a.H, a.T, a.eps_host, a.scale, a.inv_n = 16, 5, 10, 5, 0.1, 0.1, 1.0 / 16
    net = _ffi.L2hmcNet(*([FAKE] * 16))
    a.xnet = a.vnet = ctypes.pointer(net)
    for k in ("masks", "trig", "x", "v", "Lx", "p", "v1", "grad", "workspace"):
        setattr(a, k, FAKE)
    assert L.l2hmc_train_propose_grad(a, None) == -2
    assert b"binomial / negative-binomial regression target" in L.l2hmc_last_error() and route in L.l2hmc_last_error()
    s = _ffi.L2hmcTrainSplitArgs()
    e = _energy()
    s.energy = ctypes.pointer(e)
    s.n_chains, s.d, s.T, s.H = 16, 5, 5, 10
    rc = L.l2hmc_train_split_grad(s, None)
    assert rc == -2, (rc, L.l2hmc_last_error())
    assert b"binomial / negative-binomial regression target" in L.l2hmc_last_error() and route in L.l2hmc_last_error()


def test_trainers_refuse_the_fused_energy_and_name_the_slow_path():
    from l2hmc_amd.training import LogisticTrainer, SplitTrainer, Trainer

    class Dyn(object):                      # what Trainer.__new__ reads before anything else
        pass
    for kind, phi in (("binomial", None), ("negbinomial", 0.5)):
        dyn = Dyn()
        dyn._fn = bc.model(bc.case(4, 37, 3, kind, phi)).get_energy_function(fused=True)
        for cls in (Trainer, SplitTrainer, LogisticTrainer):
            with pytest.raises(NotImplementedError, match=r"get_energy_function\(\)") as ei:
                cls(dyn)
            assert "load_state_dict" in str(ei.value) and "slow path" in str(ei.value)


def test_glm_entries_take_the_new_families_and_no_other():
    L = _ffi.lib()
    ok = 1 << 12

    def loglik(S=100, d=3, n=10, fam=3):
        return L.l2hmc_glm_log_lik(ok, S, d, ok, ok, n, fam, ok, None)

    def predict(S=100, d=3, n=10, fam=3):
        return L.l2hmc_glm_predict(ok, S, d, ok, ok, n, fam, ok, ok, None)

    def tails(S=100, d=3, n=10, fam=3):
        return L.l2hmc_glm_loo_tails(ok, S, d, ok, ok, n, fam, None, 10, ok, ok, ok, ok, ok, ok, None)

    for fn in (loglik, predict, tails):
        for fam in (_ffi.GLM_BINOMIAL, _ffi.GLM_NEGBINOMIAL):
            assert fn(fam=fam, d=129) == -1 and b"<= d <= 128" in L.l2hmc_last_error(), (fn.__name__, fam, L.l2hmc_last_error())
            assert fn(fam=fam, S=1) == -1 and b"n_draws >= 2" in L.l2hmc_last_error()
        for fam in (0, 2, 5):
            assert fn(fam=fam) == -1 and b"unknown family" in L.l2hmc_last_error(), (fn.__name__, fam)
            assert fn(fam=fam, d=129) == -1 and b"unknown family" in L.l2hmc_last_error()


# ---- 3. bounds -------------------------------------------------------------------------------------------------------------------
BOUND_CASES = [("binomial", None), ("negbinomial", 0.5), ("negbinomial", 10.0)]


@pytest.mark.parametrize("kind,phi", BOUND_CASES)
@pytest.mark.parametrize("n,d", [(17, 5), (1000, 25)])
def test_bounds_hold_for_a_float32_restatement(n, d, kind, phi):
    c = bc.case(40, n, d, kind, phi)
    W = c["W"]
    U, G = bc.energy(c)
    U32, G32 = bc.energy(c, dtype=np.float32)
    b = bc.bounds(c)
    sU, sg = bc.used(U32, G32, U, G, b)
    ll, lb = bc.log_lik(c)[0], bc.ll_bounds(c)
    sl = float(np.max(np.abs(bc.log_lik32(c).astype(np.float64) - ll) / lb["B"]))
    print("%s phi=%s n=%d d=%d: float32 numpy uses %.3f of the U bound, %.3f of the grad U bound, %.3f of the ll bound"
          % (kind, phi, n, d, sU, sg, sl))
    assert sU <= 1.0 and sg <= 1.0 and sl <= 1.0
    assert np.all(b["U"] < 1e-3 * np.abs(U).max()) and np.all(b["g"] < 1e-3 * np.abs(G).max() + 1e-3)     # (they bind)
    assert np.all(lb["B"] < 1e-3 * max(1.0, np.abs(ll).max()))
    for T, beta in ((2.5, 1.0), (1.0, 0.3)):
        Us, Gs, bs = bc.scaled(c, temperature=T, beta=beta)
        q = np.float32(0.5) * (W * W).sum(axis=1)
        Ub = (np.float32(1 - beta) * q + np.float32(beta) * U32) / np.float32(T)
        Gb = (np.float32(1 - beta) * W + np.float32(beta) * G32) / np.float32(T)
        sU, sg = bc.used(Ub, Gb, Us, Gs, bs)
        assert sU <= 1.0 and sg <= 1.0, (T, beta, sU, sg)
        assert np.all(bs["U"] < 1e-3 * np.abs(Us).max())


def test_the_bounds_see_a_wrong_link():
    """an energy that counts one padded row (softplus(0) times a weight of 1), reads the weight of the next row, or drops the
    offsets is outside the bounds"""
    c = bc.case(40, 17, 5)
    U, G = bc.energy(c)
    b = bc.bounds(c)
    assert bc.used(U + np.log(2.0), G, U, G, b)[0] > 1.0
    wrong = dict(c)
    wrong["trials"] = np.roll(c["trials"], 1)
    Uw, Gw = bc.energy(wrong)
    assert min(bc.used(Uw, Gw, U, G, b)) > 1.0
    wrong = dict(c)
    wrong["offset"] = np.zeros_like(c["offset"])
    Uw, Gw = bc.energy(wrong)
    assert min(bc.used(Uw, Gw, U, G, b)) > 1.0


def test_far_rows_are_finite_and_bound():
    c = bc.far_case()
    _, t = bc.log_lik(c)
    assert np.all(np.abs(np.abs(t) - 100.0) < 1.0)
    U, G = bc.energy(c)
    U32, G32 = bc.energy(c, dtype=np.float32)
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
    sU, sg = bc.used(U32, G32, U, G, bc.bounds(c))
    assert sU <= 1.0 and sg <= 1.0, (sU, sg)


# ---- 3b. the cases of tests/test_gpu_binomial_geometries.py sit where they say ---------------------------------------------------
def _share(c):
    """(worst |log_lik32 - log_lik| / B, ll64, t, B) of a case."""
    ll, t = bc.log_lik(c)
    B = bc.ll_bounds(c)["B"]
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(bc.log_lik32(c).astype(np.float64) - ll) / B)), ll, t, B


@pytest.mark.parametrize("kind,phi", BOUND_CASES)
@pytest.mark.parametrize("S,n,d", bc.GEOM_SHAPES + bc.LONG)
def test_geometry_and_long_cases_are_bound_and_no_row_underflows(S, n, d, kind, phi):
    """Every shape of GEOM_SHAPES and LONG under each likelihood: the float32 numpy restatement uses at most half of B
    (measured 0.003 .. 0.061), and exp(ll - sat) sums to more than 0 in every row."""
    from tests import glm_case as gc
    assert bc.GEOM_SHAPES == gc.SHAPES[7:] and [-(-s[2] // 16) for s in bc.GEOM_SHAPES] == [3, 3, 5, 6, 7, 7]
    assert bc.SHAPES == gc.SHAPES[:7] and len(bc.STAT_CASES) == 11                   # (the K_* stay what they were measured on)
    c = bc.case(S, n, d, kind, phi)
    share, ll, _, _ = _share(c)
    print("%s phi=%s (%d, %d, %d): float32 numpy uses %.3g of the ll bound" % (kind, phi, S, n, d, share))
    assert share <= 0.5
    assert np.all(np.exp(ll - bc.saturated(c)).sum(axis=0) > 0.0)


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_case_sits_on_the_edges_it_names(S):
    """`binomial_case.edge_case`: the ordinary rows are those of `case(S, 32, 3)` in their order, the edge rows stand at
    `glm_case.EDGE_ROWS`' positions with offset 0; the float32 restatement is within half of B everywhere (B is absolute: it
    carries 8 u m, so it covers the `certain` row's flush to zero); the `certain` row has |t| where float32 e^-|t| is denormal
    (S = 4099 only) and where it is 0; `saturated` is 0 to 1e-40 and `certain` below the float32 normal range; `constant` is
    one value; exp(ll - sat) sums to 0 for `underflow` and `many_trials` alone, which the host `waic` counts; the host `loo`
    gives khat = inf for the five edge rows and a finite khat for every ordinary row."""
    from tests import glm_case as gc
    from tests import loglik_case as lk
    c, ordinary = bc.edge_case(S)
    at, n = bc.EDGE_ROWS, bc.EDGE_N
    assert sorted(at.values()) == sorted(gc.EDGE_ROWS.values()) == [0, 5, 17, 33, 34] and n == 37 and ordinary.sum() == 32
    assert ordinary[-1] and n % 16 != 0 and c["kind"] == "binomial"
    base = bc.case(S, 32, 3)
    assert np.array_equal(c["W"], base["W"])
    for k in ("X", "y", "offset", "trials"):
        assert c[k].dtype == np.float32 and c[k].shape[0] == n and np.array_equal(c[k][ordinary], base[k]), k
    for name, i in at.items():
        tau, y, m = bc.EDGE_SPEC[name]
        assert (c["y"][i], c["trials"][i], c["offset"][i]) == (y, m, 0.0), name
    assert c["trials"][at["many_trials"]] == glm.MAX_COUNT == 1 << 24 and not c["X"][at["constant"]].any()
    bc.model(c)                                                            # (the library takes every row: y <= trials <= 2^24)
    share, ll, t, B = _share(c)
    print("S = %d: float32 numpy uses %.3g of the ll bound" % (S, share))
    assert share <= 0.5
    tc = np.abs(t[:, at["certain"]])
    denormal, zero = (tc > 87.4) & (tc < 103.9), tc > 104.0
    assert np.all(denormal | zero) and zero.any() and denormal.any() == (S == 4099), (tc.min(), tc.max())
    assert np.all(np.abs(ll[:, at["certain"]]) < 2.0 ** -126) and np.all(np.abs(ll[:, at["saturated"]]) <= 1e-40)
    assert np.all(B[:, at["certain"]] > 2.0 ** -126)
    assert np.all(ll[:, at["constant"]] == ll[0, at["constant"]])
    sat = bc.saturated(c)
    assert sat[at["underflow"]] == 0.0 and np.all(ll[:, at["underflow"]] < -1.5e5)
    assert np.all((ll - sat)[:, [at["underflow"], at["many_trials"]]] < -745.0)
    dead = np.exp(ll - sat).sum(axis=0) == 0.0
    assert np.nonzero(dead)[0].tolist() == [at["underflow"], at["many_trials"]]
    m = bc.model(c)
    f = m.waic(c["W"])
    assert f.n_underflow == 2 and np.all(np.isneginf(f.lppd_i[dead])) and np.all(np.isfinite(f.lppd_i[~dead]))
    for r in (None, lk.r_eff_for(n)):
        s = m.loo(c["W"], r_eff=r)
        assert np.all(np.isposinf(s.khat[~ordinary])) and np.all(np.isfinite(s.khat[ordinary])), s.khat


@pytest.mark.parametrize("phi,n_finite", list(zip(bc.NB_EDGE_PHIS, (33, 32))))
def test_dispersion_edge_case(phi, n_finite):
    """`binomial_case.nb_edge_case` at phi = 1e-3 and 1e4: the float32 restatement within half of B (measured 0.28 and 0.09);
    the host khat is finite for 33 of 33 and for 32 of 33 rows."""
    c = bc.nb_edge_case(phi)
    assert c["y"][5] == 100000 and c["phi"] == phi and c["X"].shape == (33, 17) and phi not in bc.NB_PHIS
    share = _share(c)[0]
    print("phi = %g: float32 numpy uses %.3g of the ll bound" % (phi, share))
    assert share <= 0.5
    assert int(np.isfinite(bc.model(c).loo(c["W"]).khat).sum()) == n_finite


def test_trajectory_step_sizes_come_from_the_oracle():
    for n, d, H in [(17, 5, 0), (200, 25, 10)]:
        c = bc.traj_case(n, d, H)
        p = c["ref"]["forward"][3]
        assert 0.2 < float(p.mean()) < 1.0 and np.all(np.isfinite(c["ref"]["forward"][0]))
        print("n=%d d=%d H=%d: eps %g, oracle accept %.3f, float32-float64 distances %s" % (n, d, H, c["eps"], p.mean(), c["dist"]["forward"]))


def test_recorded_gates_are_four_times_the_measured_sensitivities():
    """The K_* of tests/binomial_case.py against a fresh measurement on the two cheapest cases that set them (the whole table
    is tools/binomial_accuracy.py's): a recorded K is 4 x a sensitivity that is at least what these cases show."""
    for kind, phi, S, n, d in (("binomial", None, 25, 3, 2), ("negbinomial", 0.5, 70, 33, 17)):
        k = bc.sensitivity(bc.case(S, n, d, kind, phi))
        for got, K in zip(k, (bc.K_KHAT, bc.K_ELPD, bc.K_NEFF, bc.K_MCSE)):
            assert 4.0 * got <= K * (1 + 1e-9), (kind, S, n, d, k)


# ---- 4. registers ----------------------------------------------------------------------------------------------------------------
def test_new_kernels_have_no_more_scratch_than_their_twins():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): every kernel of
    the kind-9 units against the kind-8 kernel of the same geometry, every glm kernel of families 3 / 4 against family 1's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    res = kr.resources()
    if not res.get("traj_ek9.s") or not res.get("glm_binomial.s"):
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    for new, old in (("traj_ek9.s", "traj_ek8.s"), ("traj_ladder_ek9.s", "traj_ladder_ek8.s")):
        twins = {k: sc for k, _, sc, _ in res[old]}
        rows = res[new]
        assert len(rows) == len(res[old]) and any(k.startswith("traj_") for k, _, _, _ in rows)
        for k, vg, sc, _ in rows:
            twin = re.sub(r"<9, ", "<8, ", k, count=1)
            assert "<9, " in k and twin in twins, (k, sorted(twins))
            print("%-36s %4d registers, %3d bytes of scratch (kind 8: %d)" % (k, vg, sc, twins[twin]))
            assert sc <= twins[twin], (k, sc, twins[twin])
    twins = {}
    for k, _, sc, _ in res["glm.s"]:
        twins[k] = max(sc, twins.get(k, 0))
    shared = ("chunk_reduce_kernel", "radix_advance_kernel")          # (static kernels of shared headers: one copy per unit)
    seen = [k for k, _, _, _ in res["glm_binomial.s"] if k not in shared]
    # one family's matrix and tails (the two share ll) and both families' predictive sums, at the four geometries
    want = ["glm_loo_kernel<%d, %d>" % (g, m) for g in (1, 2, 4, 8) for m in (0, 1)] + ["glm_loglik_kernel<%d>" % g for g in (1, 2, 4, 8)]
    want += ["glm_predict_kernel<%d>" % g for g in (1, 2, 4, 8)] * 2
    assert sorted(seen) == sorted(want), seen
    for k, vg, sc, _ in res["glm_binomial.s"]:
        print("%-28s %4d registers, %d bytes of scratch (family 1: %d)" % (k, vg, sc, twins[k]))
        assert sc <= twins[k] and vg <= 256, (k, vg, sc)
