"""CPU: the Poisson regression (`l2hmc_amd.PoissonRegression`, l2hmc_amd/glm.py) -- its numpy routes against the float64
restatement of tests/glm_case.py, the analytic gradient against central differences, the fixtures' own preconditions, the
refusals, the C ABI's argument validation and the compiler's listing of csrc/glm.hip."""
import os
import re

import numpy as np
import pytest

from tests import glm_case as gc
from tests import loglik_case as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(S, n, d):
    import l2hmc_amd
    W, X, y, o = gc.case(S, n, d)
    return l2hmc_amd.PoissonRegression(X, y, offset=o), W, X, y, o


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_numpy_routes_match_the_restatement(S, n, d):
    """log_lik, predict_mean and waic against the definitions (another summation order: 1e-10), loo against
    `loglik_case.restate` of the float64 matrix on the gates of `loglik_case.gate`."""
    m, W, X, y, o = _model(S, n, d)
    ll, _ = gc.log_lik(W, X, y, o)
    ref = gc.restatement(W, X, y, o)
    got = m.log_lik(W)
    assert got.dtype == np.float64 and np.max(np.abs(got - ll)) <= 1e-10
    if n > 2:
        assert np.array_equal(m.log_lik(W, rows=slice(1, n - 1)), got[:, 1:n - 1])
    assert np.max(np.abs(m.predict_mean(W) - ref["mean_mu"])) <= 1e-10 * np.max(ref["mean_mu"])
    f = m.waic(W)
    for k in ("lppd_i", "p_waic_i", "elpd_i"):
        assert np.max(np.abs(f[k] - ref[k])) <= 1e-10, k
    assert f.n_draws == S and f.n_rows == n and f.n_underflow == 0 and abs(f.elpd_waic - ref["elpd_i"].sum()) <= 1e-9
    assert f.n_high_variance == int(np.sum(ref["p_waic_i"] > 0.4))
    r = lk.r_eff_for(n)
    s = m.loo(W, r_eff=r)
    want = lk.restate(ll, s.tail_len_row, r)
    gk, ge, gn, gm = lk.gate(S)
    fin = np.isfinite(want["khat"])
    assert np.array_equal(fin, np.isfinite(s.khat)) and np.array_equal(s.n_tail, want["n_tail"])
    assert np.max(np.abs(s.elpd_loo_i - want["elpd_loo_i"])) <= ge and np.all(np.abs(s.khat - want["khat"])[fin] <= gk)
    assert np.all(gc.rel(s.n_eff, want["n_eff"])[fin] <= gn)
    # mcse: the finish forms sum w^2 (lik - E)^2 over the body as a three-term difference, whose terms are sum w^2 (lik^2 + E^2)
    # at least; the draws of `case` lie close together, so it cancels and returns the roundings amplified by
    # A_i = sum w^2 (lik + E)^2 / sum w^2 (lik - E)^2, which the restatement's own weights give.  The three terms carry the
    # rounding of their S-term sums, at most (S + 8) 2^-53 relatively, so the variance is off by at most (S + 8) 2^-53 A_i
    # relatively and mcse, its root, by half of that: the gate is gm + (S + 8) 2^-54 A_i, and A_i is capped at 1e6 on the
    # fixtures (6.3e5 at worst) so that nothing hides behind it
    with np.errstate(all="ignore"):
        w = np.exp(want["log_weights"] - np.logaddexp.reduce(want["log_weights"], axis=0))
        lik = np.exp(ll - ll.max(axis=0))
        E = (w * lik).sum(axis=0)
        amp = (w * w * (lik + E) ** 2).sum(axis=0) / (w * w * (lik - E) ** 2).sum(axis=0)
    gate = gm + (S + 8) * 2.0 ** -54 * amp
    print((S, n, d), "mcse amplification up to %.3g, worst error / gate %.3g"
          % (amp[fin].max(), np.max((gc.rel(s.mcse_elpd_loo_i, want["mcse"]) / gate)[fin])))
    assert amp[fin].max() <= 1e6
    assert np.all(gc.rel(s.mcse_elpd_loo_i, want["mcse"])[fin] <= gate[fin])
    if S % 5 == 0:
        h = m.loo(W.reshape(S // 5, 5, d), r_eff=r)
        assert np.array_equal(h.elpd_loo_i, s.elpd_loo_i)


def test_fixtures_have_full_tails_and_surprising_rows():
    """From the float64 matrix alone: no row of `case` has a tail shorter than its length (no ties at the cutoff, so no
    khat = inf at any S), counts reach into the tens, and the larger fixtures have rows on both sides of khat = 0.7."""
    from l2hmc_amd import psis
    high = 0
    for S, n, d in gc.SHAPES:
        m, W, X, y, o = _model(S, n, d)
        ll = m.log_lik(W)                                    # (the model's own float64 matrix: held against the restatement above)
        for r in (None, lk.r_eff_for(n)):
            s = psis.loo_from_log_lik(ll, r_eff=r)
            M = s.tail_len if r is None else s.tail_len_row
            assert np.all(s.n_tail == M) and np.all(M >= 5) and np.all(np.isfinite(s.khat)), (S, n, d)
        high += int(s.n_bad)
        assert y[-1] == np.ceil(3.0 * np.exp(X[-1].astype(np.float64) @ W.astype(np.float64).mean(axis=0) + o[-1]) + 5.0)
        assert np.abs(W.astype(np.float64) @ X.astype(np.float64).T).max() <= 3.0 * (1 + 1e-6) and y.max() <= 1 << 24
    assert high >= 3
    W, X, y, o = gc.exact_case(70, 33, 3, 110)
    ll, _ = gc.log_lik(W, X, y, o)
    assert len(np.unique(ll[:, 0])) < 35


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_case_sits_on_the_edges_it_names(S):
    """`glm_case.edge_case`, on the float64 h of its float32 inputs: no draw within 0.05 of the float32 overflow of mu; the
    overflow rows have between 1 and M - 1, and more than M, draws above 88.8 (ll64 below -FLT_MAX exactly there); the zero row
    has mu below the smallest float32 subnormal in every draw; the underflow row has ll - sat < -745 in every draw and is the
    ONE row the host route counts in `n_underflow`; the large count cancels eleven digits; the edge rows stand at index 0 and
    past 32, the last row of the ragged data block is ordinary, and the ordinary rows are those of `case(S, 32, 3)`."""
    import l2hmc_amd
    from l2hmc_amd import glm
    from l2hmc_amd._pareto import loo_tail_len
    W, X, y, o, ordinary = gc.edge_case(S)
    M = gc.tail_len(S)
    assert M == loo_tail_len(S) and X.shape == (gc.EDGE_N, 3) and X.dtype == y.dtype == o.dtype == W.dtype == np.float32
    W0, X0, y0, o0 = gc.case(S, 32, 3)
    assert np.array_equal(W, W0) and np.array_equal(X[ordinary], X0) and np.array_equal(y[ordinary], y0) and np.array_equal(o[ordinary], o0)
    at = gc.EDGE_ROWS
    assert min(at.values()) == 0 and max(at.values()) > 32 and ordinary[-1] and gc.EDGE_N % 16 != 0 and ordinary.sum() == 32
    ll, h = gc.log_lik(W, X, y, o)
    assert np.abs(h - gc.MU_OVERFLOW_H).min() >= 0.05
    flt_max = float(np.finfo(np.float32).max)
    over = h > 88.8
    assert np.array_equal(over, h > gc.MU_OVERFLOW_H) and np.array_equal(over, ll < -flt_max) and np.all(np.abs(ll[~over]) < flt_max)
    count = over.sum(axis=0)
    assert 1 <= count[at["overflow_few"]] <= M - 1 and M < count[at["overflow_many"]] < S
    assert count.sum() == count[at["overflow_few"]] + count[at["overflow_many"]]
    assert y[at["zero"]] == 0 and np.all(np.exp(h[:, at["zero"]]) < 2.0 ** -150)
    sat = glm.row_constants(y, o)[2].astype(np.float64)
    dead = np.all(ll - sat < -745.0, axis=0)
    assert dead.tolist() == [i == at["underflow"] for i in range(gc.EDGE_N)]
    big = at["large"]
    assert y[big] == 100000 and np.all(np.abs(ll[:, big]) < 1e-5 * y[big] * h[:, big])       # y h ~ 1.15e6 against |ll| < 11.5
    f = l2hmc_amd.PoissonRegression(X, y, offset=o).waic(W)
    assert f.n_underflow == 1 and np.isneginf(f.lppd_i[at["underflow"]])


def test_long_history_shapes_sit_in_their_segment_and_chunk_branches():
    """The long histories of tests/test_gpu_glm_geometries.py, through the workspace-size entries: the gather's segments are
    max(64, ceil(S / 2048)) draws -- 65 at S = 131073 (2017 segments, the last of 33 draws: two tiles and one draw), 69 at
    140001 (2029, the last a full one: four tiles and 5 draws) and at 140003 (2030, the last of 2 draws) -- and the predictive
    sums' chunks are 4 tiles (three rows are one row group: 4096 chunks are aimed for, the floor holds)."""
    from l2hmc_amd import _ffi
    L = _ffi.lib()
    ws, wp = L.l2hmc_glm_loo_workspace_bytes, L.l2hmc_glm_predict_workspace_doubles
    n = 3
    for (S, d), (seg, nseg, last, chunks) in (((131073, 40), (65, 2017, 33, 2049)), ((140001, 40), (69, 2029, 69, 2188)),
                                              ((140001, 100), (69, 2029, 69, 2188)), ((140003, 100), (69, 2030, 2, 2188))):
        assert seg == max(64, -(-S // 2048)) and nseg == -(-S // seg) and last == S - (nseg - 1) * seg
        assert ws(S, n, d) == 8 + n * (256 * 8 + 8 + 8 + 4 + 4) + nseg * 3 * n * 8, (S, d)
        assert wp(S, n, d) == chunks * 4 * n and chunks == -(-(-(-S // 16)) // 4), (S, d)
    assert max(64, -(-131072 // 2048)) == 64                 # 131073 is the first S with segments that are no multiple of 16


def test_row_constants_and_saturation():
    """g = lgamma(y + 1), sat = y log y - y - g (0 at y = 0) is the supremum of ll over eta: exp(ll - sat) <= 1."""
    from scipy.special import gammaln
    from l2hmc_amd import glm
    y = np.array([0, 1, 2, 17, 1000, 1 << 24], dtype=np.float64)
    c = glm.row_constants(y, np.linspace(-1, 2, 6))
    assert c.shape == (3, 6) and c.dtype == np.float32
    assert np.array_equal(c[1], gammaln(y + 1).astype(np.float32)) and c[2, 0] == 0.0 and c[1, 0] == 0.0 and c[1, 1] == 0.0
    h = np.linspace(-5, 20, 2001)[:, None]
    ll = y * h - np.exp(h) - gammaln(y + 1)
    sat = np.where(y > 0, y * np.log(np.maximum(y, 1)) - y - gammaln(y + 1), 0.0)
    assert np.all(ll <= sat + 1e-9 * (1 + np.abs(sat))) and np.allclose(c[2], sat, rtol=1e-6, atol=0)


def test_gradient_matches_central_differences():
    """grad U = X^T (mu - y) + w / prior_var against float64 central differences of the energy; -U is `log_density`; the
    gradient is differentiable torch code (the trainer's Hessian-vector products)."""
    import torch
    import l2hmc_amd
    from l2hmc_amd.distributions import UserEnergy
    W, X, y, o = gc.case(25, 12, 5)
    m = l2hmc_amd.PoissonRegression(X, y, offset=o, prior_var=2.5)
    e = m.get_energy_function()
    assert isinstance(e, UserEnergy) and e.grad_fn is not None
    x = torch.as_tensor(W[:6].astype(np.float64))
    U, g = e.fn(x).numpy(), e.grad_fn(x).numpy()
    assert np.max(np.abs(U + m.log_density(W[:6]))) <= 1e-10 * np.max(np.abs(U))
    eps = 1e-5
    for k in range(5):
        step = torch.zeros(5, dtype=torch.float64)
        step[k] = eps
        num = (e.fn(x + step) - e.fn(x - step)).numpy() / (2 * eps)
        assert np.max(np.abs(num - g[:, k])) <= 1e-6 * (1 + np.max(np.abs(g))), k
    xr = x.clone().requires_grad_(True)
    gr = e.grad_fn(xr)
    assert gr.requires_grad
    u = torch.ones_like(x)
    hv, = torch.autograd.grad((gr * u).sum(), xr)
    X64, o64 = torch.as_tensor(X.astype(np.float64)), torch.as_tensor(o.astype(np.float64))
    want = (torch.exp(x @ X64.t() + o64) * (u @ X64.t())) @ X64 + u / 2.5
    assert torch.max(torch.abs(hv - want)) <= 1e-9 * torch.max(torch.abs(want))


def test_bad_arguments_raise_value_error():
    import l2hmc_amd
    P = l2hmc_amd.PoissonRegression
    W, X, y, o = gc.case(25, 6, 3)
    assert "PoissonRegression" in l2hmc_amd.__all__ and l2hmc_amd.distributions.PoissonRegression is P
    bad = []
    for v in (-1.0, 0.5, float(1 << 24) + 2, np.nan):
        yy = y.astype(np.float64).copy()
        yy[2] = v
        bad.append(dict(X=X, y=yy))
    Xn = X.copy()
    Xn[1, 1] = np.inf
    on = o.copy()
    on[0] = np.nan
    bad += [dict(X=Xn, y=y), dict(X=X, y=y, offset=on), dict(X=X, y=y, offset=o[:5]), dict(X=X, y=y[:5]), dict(X=X[0], y=y),
            dict(X=np.zeros((4, 129)), y=np.zeros(4)), dict(X=X, y=y, prior_var=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            P(**kw)
    m = P(X, y, offset=o)
    for fn, args in ((m.loo, (W[:, :2],)), (m.waic, (W[:1],)), (m.log_lik, (W[0],)), (m.relative_eff, (W,)),
                     (m.predict_mean, (W, X[:, :2])), (m.predict_mean, (W, X, o[:3]))):
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(ValueError):
        m.loo(W, r_eff="always")
    with pytest.raises(ValueError):
        m.loo(W, r_eff="auto")                               # a matrix: its chains are not known
    with pytest.raises(ValueError):
        m.log_lik(W, rows=(3, 9))
    assert P(X, np.full(6, float(1 << 24))).y[0] == float(1 << 24)


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the five entries (ABI version still 6); every L2HMC_ERR_ARG
    case is refused with a message before anything is launched."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_glm_log_lik", "l2hmc_glm_predict_workspace_doubles", "l2hmc_glm_predict", "l2hmc_glm_loo_workspace_bytes",
                 "l2hmc_glm_loo_tails"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION and _ffi.GLM_POISSON == 1
    assert re.search(r"L2HMC_GLM_POISSON = 1\b", hdr)
    ok = 1 << 12                                             # an aligned non-NULL address: refused before it is touched
    P = _ffi.GLM_POISSON

    def loglik(S=100, d=3, n=10, fam=P, ptrs=(ok, ok, ok, ok)):
        return L.l2hmc_glm_log_lik(ptrs[0], S, d, ptrs[1], ptrs[2], n, fam, ptrs[3], None)

    def predict(S=100, d=3, n=10, fam=P, ptrs=(ok, ok, ok, ok, ok)):
        return L.l2hmc_glm_predict(ptrs[0], S, d, ptrs[1], ptrs[2], n, fam, ptrs[3], ptrs[4], None)

    def tails(S=100, d=3, n=10, fam=P, stride=10, ptrs=(ok, ok, ok, None, ok, ok, ok, ok, ok, ok)):
        return L.l2hmc_glm_loo_tails(ptrs[0], S, d, ptrs[1], ptrs[2], n, fam, ptrs[3], stride, *ptrs[4:], None)

    for fn in (loglik, predict, tails):
        for kw, msg in ((dict(fam=0), b"unknown family"), (dict(fam=2), b"unknown family"), (dict(d=129), b"<= d <= 128"),
                        (dict(d=0), b"<= d <= 128"), (dict(S=1), b"n_draws >= 2"), (dict(n=0), b"n_data"),
                        (dict(n=(1 << 20) + 1), b"n_data"), (dict(S=(1 << 40) // 3 + 1), b"too large")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert msg in L.l2hmc_last_error(), (fn.__name__, kw, L.l2hmc_last_error())
    for fn, count, align in ((loglik, 4, (4, 16, 4, 4)), (predict, 5, (4, 16, 4, 8, 8)),
                             (tails, 10, (4, 16, 4, 8, 4, 4, 8, 4, 8, 8))):
        base = [ok] * count
        for at in range(count):
            p = list(base)
            p[at] = None
            if not (fn is tails and at == 3):                # (tail_len_row may be NULL)
                assert fn(ptrs=tuple(p)) == -1 and b"required" in L.l2hmc_last_error(), (fn.__name__, at)
            p[at] = ok + align[at] // 2
            assert fn(ptrs=tuple(p)) == -1 and b"aligned" in L.l2hmc_last_error(), (fn.__name__, at)
    for stride in (-1, 100, 101):
        assert tails(stride=stride) == -1 and b"tail_stride < n_draws" in L.l2hmc_last_error()
    assert tails(S=1 << 24, n=1 << 20, stride=4096) == -1 and b"tail too large" in L.l2hmc_last_error()
    assert loglik(S=1 << 30, n=1 << 11) == -1 and b"matrix too large" in L.l2hmc_last_error()
    p = [ok] * 10
    p[7] = None                                              # tail may be NULL only when tail_stride = 0
    assert tails(ptrs=tuple(p)) == -1 and b"required" in L.l2hmc_last_error()
    ws, wp = L.l2hmc_glm_loo_workspace_bytes, L.l2hmc_glm_predict_workspace_doubles
    assert ws(4096000, 1000, 25) > 0 and ws(4096000, 1000, 25) % 8 == 0 and ws(25, 1, 1) > 0 and wp(4096000, 1000, 25) > 0
    assert ws(1, 10, 3) == -1 and wp(100, 10, 129) == -1
    # the draw chunks of the tails depend on n_draws alone: the workspace grows in proportion to the rows
    assert ws(4099, 64, 25) - ws(4099, 32, 25) == ws(4099, 96, 25) - ws(4099, 64, 25)
    n, S = 100, 4099
    segments = -(-S // 64)                                   # the gather's partials: one per segment of max(64, ceil(S / 2048)) draws
    assert ws(S, n, 25) == 8 + n * (256 * 8 + 8 + 8 + 4 + 4) + segments * 3 * n * 8
    assert ws(140001, n, 25) - ws(140001, n - 1, 25) == 256 * 8 + 24 + -(-140001 // 69) * 3 * 8
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(tails(fam=7))


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of
    glm.s uses scratch at any of the four geometries, every kernel stays within the 256 registers that the two waves per SIMD
    of its launch bounds (and of the unit's header) imply, and the static LDS lets two workgroups share a CU's 160 KiB."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("glm.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = [k for k, _, _, _ in rows]
    want = ["glm_loo_kernel<%d, %d>" % (g, m) for g in (1, 2, 4, 8) for m in (0, 1)]
    want += ["glm_loglik_kernel<%d>" % g for g in (1, 2, 4, 8)] + ["glm_predict_kernel<%d>" % g for g in (1, 2, 4, 8)]
    want += ["radix_advance_kernel", "glm_loo_init_kernel", "chunk_reduce_kernel"]
    assert sorted(want) == sorted(names), names
    for k, vg, sc, _ in rows:
        print("%-28s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0 and vg <= 512 // 2, (k, vg, sc)
    asm = open(os.path.join(kr.ASM, "glm.s")).read()
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", asm)]
    assert len(lds) == len(names) and max(lds) <= 80 * 1024, lds
