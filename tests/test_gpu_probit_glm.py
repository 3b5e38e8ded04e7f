"""GPU: the fused model criticism of binomial regression with the probit link (csrc/glm_probit.hip, family 6 of the l2hmc_glm_*
entries; `ProbitRegression`), mirroring tests/test_gpu_binomial_glm.py -- the matrix `l2hmc_glm_log_lik` writes against float64,
the fused tails against the exact selection of that very matrix bit for bit, the predictive sums and the finished numbers against
their bounds and gates (tests/probit_case.py), and the EDGE rows (t to +-30) through the matrix and the tails."""
import numpy as np
import pytest

from tests import glm_case as gc
from tests import loglik_case as lk
from tests import probit_case as pc

pytestmark = pytest.mark.gpu
_CACHE = {}
_bits = gc.bits
CASES = pc.SHAPES


def _setup(S, n, d):
    """(case, model, Wd, ll32): the case, its model, the draws on the device and the matrix the device writes."""
    import torch
    key = (S, n, d)
    if key not in _CACHE:
        c = pc.case(S, n, d)
        m = pc.model(c)
        Wd = torch.as_tensor(c["W"]).cuda()
        ll32 = m.log_lik(Wd)
        assert ll32.dtype == torch.float32 and tuple(ll32.shape) == (S, n)
        _CACHE[key] = (c, m, Wd, ll32.cpu().numpy())
    return _CACHE[key]


def _raw(m, Wd, lens=None):
    t = m._glm.loo_tails(Wd, tail_len_row=lens)
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["sums"] = np.stack([out["body"], out["body_sq"], out["lik"]])
    return out


@pytest.mark.parametrize("S,n,d", CASES)
def test_matrix_against_float64(S, n, d):
    """|ll32 - ll64| <= B_si of tests/probit_case.py, element by element; a row range equals the same columns of the whole."""
    c, m, Wd, ll32 = _setup(S, n, d)
    ll64, _ = pc.log_lik(c)
    b = pc.ll_bounds(c)
    ratio = float(np.max(np.abs(ll32.astype(np.float64) - ll64) / b["B"]))
    print("probit (%d, %d, %d) worst |ll32 - ll64| / bound: %.3g" % (S, n, d, ratio))
    assert ratio <= 1.0
    if n > 17:
        part = m.log_lik(Wd, rows=(17, n)).cpu().numpy()
        assert np.array_equal(_bits(part), _bits(ll32[:, 17:]))


@pytest.mark.parametrize("S,n,d", CASES)
def test_fused_tails_are_the_exact_selection_of_the_matrix(S, n, d):
    """One tail length (tail_len_row = NULL) and per-row lengths that include 0, 1, 4, 5 and S // 5 in one call: `check_raw`
    holds cutoff, top, n_tail and the tail against the exact selection of the written matrix and the three float64 sums against
    `l2hmc_loglik_tails` of it bit for bit."""
    _, m, Wd, ll32 = _setup(S, n, d)
    gc.check_raw(ll32, None, _raw(m, Wd))
    lens = lk.lengths_for(S, n)
    gc.check_raw(ll32, lens, _raw(m, Wd, lens))


@pytest.mark.parametrize("S,n,d", [(70, 33, 17), (4099, 100, 25)])
def test_bits_do_not_depend_on_the_call(S, n, d):
    """Two calls give identical bits; rows [0, n) in one call equal the rows of two calls split at row 17, and the groups of 7
    rows that a small `max_tail_bytes` makes."""
    c, m, Wd, ll32 = _setup(S, n, d)
    lens = lk.lengths_for(S, n)
    one, two = _raw(m, Wd, lens), _raw(m, Wd, lens)
    head, rest = _raw(pc.model(pc.rows_of(c, 0, 17)), Wd, lens[:17]), _raw(pc.model(pc.rows_of(c, 17, n)), Wd, lens[17:])
    for k in ("cutoff", "top", "n_tail", "sums"):
        assert np.array_equal(_bits(one[k]), _bits(two[k])), k
        assert np.array_equal(_bits(one[k][..., :17]), _bits(head[k])) and np.array_equal(_bits(one[k][..., 17:]), _bits(rest[k])), k
    srt = lambda g, a, b: np.sort(lk.keys(g["tail"][a:b]), axis=1)  # noqa: E731  (monotone keys: the +inf pads last)
    assert np.array_equal(srt(one, 0, n), srt(two, 0, n))
    assert np.array_equal(srt(one, 0, 17)[:, :head["tail"].shape[1]], srt(head, 0, 17))
    assert np.array_equal(srt(one, 17, n)[:, :rest["tail"].shape[1]], srt(rest, 0, n - 17))
    a, b2 = m.waic(Wd), m.waic(Wd)
    assert np.array_equal(_bits(a.elpd_i), _bits(b2.elpd_i))
    r = lk.r_eff_for(n)
    got = m.loo(Wd, r_eff=r)
    small = m.loo(Wd, r_eff=r, max_tail_bytes=4 * 7 * got.tail_len)
    for k in ("elpd_loo_i", "khat", "n_eff", "mcse_elpd_loo_i"):
        assert np.array_equal(_bits(small[k]), _bits(got[k])), k


@pytest.mark.parametrize("S,n,d", CASES)
def test_predictive_sums_against_float64(S, n, d):
    """The predictive mean, lppd_i, mean ll and p_waic_i inside the bounds of tests/probit_case.py; `predict_mean` of new rows
    with `trials=` (the model's own rows handed back give the same bits, one trial gives the probability Phi)."""
    c, m, Wd, _ = _setup(S, n, d)
    ref, b = pc.restatement(c), pc.ll_bounds(c)
    s, f = m._glm.pointwise_sums(Wd), m.waic(Wd)
    got = {"mean_mu": s["sum_mu"] / S, "lppd_i": f.lppd_i, "mean_ll": s["sum_ll"] / S, "p_waic_i": f.p_waic_i}
    ratios = {k: float(np.max(np.abs(got[k] - ref[k]) / b[k])) for k in got}
    print("probit", (S, n, d), " ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert np.array_equal(f.p_mean, got["mean_mu"]) and f.n_underflow == 0 and f.n_draws == S
    new = m.predict_mean(Wd, X=c["X"], offset=c["offset"], trials=c["trials"])
    assert np.array_equal(_bits(new), _bits(got["mean_mu"]))
    prob = m.predict_mean(Wd, X=c["X"], offset=c["offset"])               # trials = 1: the success probability
    one = dict(c, trials=np.ones(n, dtype=np.float32), y=np.zeros(n, dtype=np.float32))
    assert np.all(np.abs(prob - pc.restatement(one)["mean_mu"]) <= pc.ll_bounds(one)["mean_mu"])
    assert np.all((prob > 0.0) & (prob < 1.0))
    host = m.waic(c["W"])
    assert np.max(np.abs(f.elpd_i - host.elpd_i)) <= np.max(b["lppd_i"] + b["p_waic_i"])


def _agree(got, ref, S, mc, fin):
    gk, ge, gn, gm = lk.gate(S)
    dk = float(np.max(np.abs(got.khat - ref.khat)[fin])) if fin.any() else 0.0
    de = float(np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i)))
    out = [dk, de]
    if mc:
        dn = float(np.max(gc.rel(got.n_eff, ref.n_eff)[fin])) if fin.any() else 0.0
        dm = float(np.max(gc.rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i)[fin])) if fin.any() else 0.0
        out += [dn, dm]
    assert np.array_equal(got.n_tail, ref.n_tail) and np.array_equal(np.isfinite(got.khat), fin)
    assert dk <= gk and de <= ge, (dk, de)
    if mc:
        assert np.array_equal(got.tail_len_row, ref.tail_len_row)
        assert dn <= gn and dm <= gm, (dn, dm)
    return out


@pytest.mark.parametrize("S,n,d", CASES)
def test_finished_numbers_equal_the_materialised_route(S, n, d):
    """The fused `loo` against `loo_from_log_lik(select="fused")` on `log_lik`: the tails are identical and the gather adds its
    terms in the order of `l2hmc_loglik_tails`, so khat, elpd_loo_i, n_eff and mcse are equal exactly."""
    import torch
    from l2hmc_amd import psis
    _, m, Wd, ll32 = _setup(S, n, d)
    dev = torch.as_tensor(ll32).cuda()
    for r in (None, lk.r_eff_for(n)):
        got, ref = m.loo(Wd, r_eff=r), psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        assert np.array_equal(got.n_tail, ref.n_tail) and got.n_bad == ref.n_bad and got.n_draws == S and got.n_rows == n
        for k in ("khat", "elpd_loo_i") + (("n_eff", "mcse_elpd_loo_i") if r is not None else ()):
            assert gc.same_bits(np.asarray(got[k]), np.asarray(ref[k])), (k, r is not None)


@pytest.mark.parametrize("S,n,d", CASES)
def test_finished_numbers_against_float64(S, n, d):
    """The fused `loo` against the numpy route of the float64 matrix: gates K x delta_i (tests/probit_case.py)."""
    c, m, Wd, _ = _setup(S, n, d)
    delta = pc.ll_bounds(c)["delta"]
    r = lk.r_eff_for(n)
    got, ref = m.loo(Wd, r_eff=r), m.loo(c["W"], r_eff=r)
    fin = np.isfinite(ref.khat)
    assert np.array_equal(fin, np.isfinite(got.khat)) and np.array_equal(got.n_tail, ref.n_tail)
    shares = {"khat": np.max((np.abs(got.khat - ref.khat) / (pc.K_KHAT * delta))[fin]) if fin.any() else 0.0,
              "elpd_loo_i": np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / (pc.K_ELPD * delta)),
              "n_eff": np.max((gc.rel(got.n_eff, ref.n_eff) / (pc.K_NEFF * delta))[fin]) if fin.any() else 0.0,
              "mcse": np.max((gc.rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / (pc.K_MCSE * delta))[fin]) if fin.any() else 0.0}
    print("probit", (S, n, d), " ".join("%s %.3g" % (k, float(v)) for k, v in shares.items()))
    assert all(float(v) <= 1.0 for v in shares.values()), shares
    plain, ref0 = m.loo(Wd), m.loo(c["W"])
    assert np.max(np.abs(plain.elpd_loo_i - ref0.elpd_loo_i) / (pc.K_ELPD * delta)) <= 1.0


def test_relative_eff_and_auto_on_an_ar1_history():
    """`relative_eff` of a device history against the float64 host route within K_REFF delta_i; `loo(r_eff="auto")` equals the
    call with that r_eff given and `loo_from_log_lik(select="fused")` of the materialised history; row groups of
    `relative_eff` give the same bits."""
    import torch
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split, n = gc.AR1
    c = pc.ar1_case()
    m = pc.model(c)
    Wd = torch.as_tensor(c["W"]).cuda()
    delta = pc.ll_bounds(c)["delta"]
    e, ref = m.relative_eff(Wd, max_lag=max_lag, split=split), m.relative_eff(c["W"], max_lag=max_lag, split=split)
    worst = float(np.max(gc.rel(e.r_eff, ref.r_eff) / (pc.K_REFF * delta)))
    print("r_eff %.3g .. %.3g, worst relative error / (K_REFF delta_i) %.3g" % (e.r_eff.min(), e.r_eff.max(), worst))
    assert worst <= 1.0 and e.n_nan == 0 and e.n_draws == M * N
    grouped = m.relative_eff(Wd, max_lag=max_lag, split=split, max_bytes=4 * M * N * 5)
    assert np.array_equal(_bits(grouped.r_eff), _bits(e.r_eff))
    auto, given = m.loo(Wd, r_eff="auto", max_lag=max_lag, split=split), m.loo(Wd, r_eff=e.r_eff)
    for k in ("r_eff", "elpd_loo_i", "khat", "n_eff", "mcse_elpd_loo_i"):
        assert np.array_equal(_bits(auto[k]), _bits(given[k])), k
    same = psis.loo_from_log_lik(m.log_lik(Wd), r_eff=e.r_eff, select="fused")
    print(" ".join("%.2g" % v for v in _agree(auto, same, M * N, True, np.isfinite(same.khat))))


# ---- the entries called straight: a ragged third block in a second row group, one NaN draw, the tails of the link ---------------
RAW = ("ll", "cutoff", "top", "n_tail", "sums", "psums")


def test_ragged_37_rows_in_two_groups():
    """37 rows: rows 32 .. 36 are a ragged third data block in a second row group.  With poisoned, guarded outputs
    (`probit_case.device_raw`): no in-range element keeps its fill, every guard does, the tails are the exact selection of the
    written matrix, and rows [17, 37) in a call of their own give the bits they have inside the whole."""
    import torch
    S, n, d = 70, 37, 3
    c = pc.case(S, n, d)
    for lens in (None, lk.lengths_for(S, n)):
        res = pc.device_raw(c, lens=lens)
        assert gc.all_written(res), [k for k in RAW + ("tail",) if res[k].dtype.kind == "f" and np.isnan(res[k]).any()]
        assert gc.guards_untouched(res), res["guards"]
        gc.check_raw(res["ll"], lens, res)
        part = pc.device_raw(c, lens=lens, rows=(17, n))
        assert gc.all_written(part) and gc.guards_untouched(part)
        for k in RAW:
            assert gc.same_bits(res[k][..., 17:], part[k]), k
        m = pc.model(c)
        Wd = torch.as_tensor(c["W"]).cuda()
        assert gc.same_bits(m.log_lik(Wd).cpu().numpy(), res["ll"])
        s = m._glm.pointwise_sums(Wd)
        assert gc.same_bits(np.stack([s["sum_lik"], s["sum_ll"], s["sum_ll2"]]), res["psums"][1:])


def test_one_nan_draw():
    """`glm_case.nan_case`'s draws (4099, 35, 17) with a NaN in coordinate 5 of draw 1234, on probit data: the matrix is NaN in
    that draw for every row and keeps the clean call's bits in every other draw; every row's top, tail sums and predictive sums
    are NaN; cutoff, n_tail and the tail are the exact selection of the numbers (a NaN's key is the last: it is never in a
    tail); the error word is 0; `loo` returns NaN for every row, quietly."""
    import torch
    W, _, _, _, bad = gc.nan_case()
    c = pc.case(4099, 35, 17)
    assert np.array_equal(c["W"], W)
    S, n = W.shape[0], 35
    clean, got = pc.device_raw(c), pc.device_raw(c, W=bad)
    assert gc.all_written(clean) and gc.guards_untouched(clean) and gc.guards_untouched(got) and int(got["flag"][0]) == 0
    assert np.isnan(got["ll"][1234]).all()
    others = np.arange(S) != 1234
    assert np.array_equal(gc.bits(got["ll"][others]), gc.bits(clean["ll"][others]))
    assert np.isnan(got["top"]).all() and np.isnan(got["sums"]).all() and np.isnan(got["psums"]).all()
    ex = lk.select_exact(got["ll"], np.full(n, gc.tail_len(S), dtype=np.int64))
    assert np.array_equal(gc.bits(got["cutoff"]), gc.bits(ex["cutoff"])) and np.array_equal(got["n_tail"], ex["n_tail"])
    assert not np.isnan(got["tail"]).any() and not (got["tail"] == -7).any()
    for i in range(n):
        L = int(ex["n_tail"][i])
        assert np.all(np.isposinf(got["tail"][i, L:])) and sorted(lk.keys(got["tail"][i, :L]).tolist()) == [p[0] for p in ex["pairs"][i]], i
    mat = lk.device_raw(got["ll"], want_pos=False)
    for k in ("cutoff", "top", "n_tail", "sums"):
        assert gc.same_bits(got[k], mat[k]), k
    s = pc.model(c).loo(torch.as_tensor(bad).cuda(), r_eff=lk.r_eff_for(n))
    assert np.isnan(s.elpd_loo_i).all() and np.isnan(s.khat).all()


def test_edge_rows_through_the_matrix_and_the_tails():
    """EDGE (t near 0, +-5, +-9, +-15, +-30; y = 0, y = m, between; m = 50): every element of the written matrix is finite and
    within B_si of float64 -- ll = -22716 at t = -30, y = 50 and -1e-196 (0 in float32) at t = +30 -- the mean within Bmean, the
    tails the exact selection of the written matrix with both kinds of tail length, the outputs guarded, and the matrix the
    fused energy's own terms: sum_i (c_i - ll_si) + |w_s|^2 / (2 s2) is U within the sum's roundings."""
    import torch
    c = pc.EDGE
    S, n = c["W"].shape[0], pc.EDGE_N
    ll64, t = pc.log_lik(c)
    b = pc.ll_bounds(c)
    for lens in (None, lk.lengths_for(S, n)):
        res = pc.device_raw(c, lens=lens)
        assert gc.all_written(res) and gc.guards_untouched(res) and int(res["flag"][0]) == 0
        assert np.all(np.isfinite(res["ll"])) and np.all(np.isfinite(res["psums"]))
        share = np.abs(res["ll"].astype(np.float64) - ll64) / b["B"]
        gc.check_raw(res["ll"], lens, res)
    by_tau = " ".join("%g: %.3g" % (tau, share[:, 3 * j:3 * j + 3].max()) for j, tau in enumerate(pc.EDGE_TAUS))
    print("EDGE: worst |ll32 - ll64| / bound %.3g; by tau %s" % (share.max(), by_tau))
    assert share.max() <= 1.0
    mean_share = np.abs(res["psums"][0] / S - pc.restatement(c)["mean_mu"]) / b["mean_mu"]
    print("EDGE: mean / bound %.3g" % mean_share.max())
    assert np.all(mean_share <= 1.0)
    m = pc.model(c, prior_var=pc.PRIOR_VAR)
    U = m.get_energy_function(fused=True).evaluate(torch.as_tensor(c["W"]).cuda())[0].cpu().numpy().astype(np.float64)
    k32 = m._glm.consts[3].astype(np.float64)
    from_ll = (k32 - res["ll"].astype(np.float64)).sum(axis=1) + 0.5 * np.square(c["W"].astype(np.float64)).sum(axis=1) / pc.PRIOR_VAR
    assert np.all(np.abs(U - from_ll) <= (n + 16) * pc.EPS * np.abs(k32 - res["ll"].astype(np.float64)).sum(axis=1) + 4 * pc.EPS * np.abs(U))
