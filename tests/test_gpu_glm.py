"""GPU: the fused model criticism of the Poisson regression (csrc/glm.hip; `l2hmc_amd.PoissonRegression`) -- the matrix
`l2hmc_glm_log_lik` writes against float64, the fused tails against the exact selection of that very matrix bit for bit, the
predictive sums and the finished numbers against their bounds (tests/glm_case.py)."""
import numpy as np
import pytest

from tests import glm_case as gc
from tests import loglik_case as lk

pytestmark = pytest.mark.gpu
_CACHE = {}


_bits = gc.bits


def _setup(S, n, d, exact=False):
    """(model, W, X, y, o, Wd, ll32): the case, its model, the draws on the device and the matrix the device writes."""
    import torch
    import l2hmc_amd
    key = (S, n, d, exact)
    if key not in _CACHE:
        W, X, y, o = gc.exact_case(S, n, d, 40 + S) if exact else gc.case(S, n, d)
        m = l2hmc_amd.PoissonRegression(X, y, offset=o)
        Wd = torch.as_tensor(W).cuda()
        ll32 = m.log_lik(Wd)
        assert ll32.dtype == torch.float32 and tuple(ll32.shape) == (S, n)
        _CACHE[key] = (m, W, X, y, o, Wd, ll32.cpu().numpy())
    return _CACHE[key]


def _raw(m, Wd, lens=None):
    t = m._glm.loo_tails(Wd, tail_len_row=lens)
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["sums"] = np.stack([out["body"], out["body_sq"], out["lik"]])
    return out


_check_raw = gc.check_raw                                   # (shared with tests/test_gpu_glm_geometries.py)


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_matrix_against_float64(S, n, d):
    """|ll32 - ll64| <= B_si of tests/glm_case.py, element by element; a row range equals the same columns of the whole."""
    m, W, X, y, o, Wd, ll32 = _setup(S, n, d)
    ll64, _ = gc.log_lik(W, X, y, o)
    b = gc.bounds(W, X, y, o)
    ratio = float(np.max(np.abs(ll32.astype(np.float64) - ll64) / b["B"]))
    print("(%d, %d, %d) worst |ll32 - ll64| / bound: %.3g" % (S, n, d, ratio))
    assert ratio <= 1.0
    if n > 17:
        part = m.log_lik(Wd, rows=(17, n)).cpu().numpy()
        assert np.array_equal(_bits(part), _bits(ll32[:, 17:]))


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_fused_tails_are_the_exact_selection_of_the_matrix(S, n, d):
    """One tail length (tail_len_row = NULL) and per-row lengths that include 0, 1, 4, 5 and S // 5 in one call."""
    m, _, _, _, _, Wd, ll32 = _setup(S, n, d)
    _check_raw(ll32, None, _raw(m, Wd))
    lens = lk.lengths_for(S, n)
    _check_raw(ll32, lens, _raw(m, Wd, lens))


@pytest.mark.parametrize("S,n,d", gc.EXACT_SHAPES)
def test_fused_tails_with_ties(S, n, d):
    """`exact_case`: eta is exact and ll takes few values -- ties at the cutoff shorten the tails."""
    m, _, _, _, _, Wd, ll32 = _setup(S, n, d, exact=True)
    assert len(np.unique(ll32[:, 0])) < S // 2
    got = _raw(m, Wd)
    _check_raw(ll32, None, got)
    assert np.any(got["n_tail"] < got["tail"].shape[1])
    lens = lk.lengths_for(S, n)
    _check_raw(ll32, lens, _raw(m, Wd, lens))


def test_segments_that_are_no_multiple_of_a_tile():
    """S = 140001 > 131072: the gather's segments are ceil(S / 2048) = 69 draws, cut out of the history at any draw, each four
    full tiles and one of 5 draws (140001 = 2029 x 69: the last segment is a full one; tests/test_gpu_glm_geometries.py has
    the short last segments); the count passes run beyond their floor of 4 tiles per chunk (9)."""
    S, n, d = 140001, 3, 2
    m, _, _, _, _, Wd, ll32 = _setup(S, n, d)
    _check_raw(ll32, None, _raw(m, Wd))
    _check_raw(ll32, lk.lengths_for(S, n), _raw(m, Wd, lk.lengths_for(S, n)))


def test_bits_do_not_depend_on_the_call():
    """Two calls give identical bits; rows [0, n) in one call equal the rows of two calls split at row 17; a first-axis slice
    of a history whose base is only 4-byte aligned gives the bits of its contiguous copy."""
    import torch
    import l2hmc_amd
    for S, n, d in ((70, 33, 17), (4099, 100, 25)):
        m, W, X, y, o, Wd, ll32 = _setup(S, n, d)
        lens = lk.lengths_for(S, n)
        one, two = _raw(m, Wd, lens), _raw(m, Wd, lens)
        head = _raw(l2hmc_amd.PoissonRegression(X[:17], y[:17], offset=o[:17]), Wd, lens[:17])
        rest = _raw(l2hmc_amd.PoissonRegression(X[17:], y[17:], offset=o[17:]), Wd, lens[17:])
        buf = torch.zeros(S * d + 1, dtype=torch.float32, device="cuda")
        buf[1:] = Wd.reshape(-1)
        sliced = buf[1:].view(S, d)
        assert sliced.data_ptr() % 8 == 4 and sliced.is_contiguous()
        off = _raw(m, sliced, lens)
        assert np.array_equal(_bits(m.log_lik(sliced).cpu().numpy()), _bits(ll32))
        for k in ("cutoff", "top", "n_tail", "sums"):
            assert np.array_equal(_bits(one[k]), _bits(two[k])) and np.array_equal(_bits(one[k]), _bits(off[k])), k
            assert np.array_equal(_bits(one[k][..., :17]), _bits(head[k])) and np.array_equal(_bits(one[k][..., 17:]), _bits(rest[k])), k
        srt = lambda g, a, b: np.sort(lk.keys(g["tail"][a:b]), axis=1)  # noqa: E731  (monotone keys: the +inf pads last)
        assert np.array_equal(srt(one, 0, n), srt(two, 0, n)) and np.array_equal(srt(one, 0, n), srt(off, 0, n))
        assert np.array_equal(srt(one, 0, 17)[:, :head["tail"].shape[1]], srt(head, 0, 17))
        assert np.array_equal(srt(one, 17, n)[:, :rest["tail"].shape[1]], srt(rest, 0, n - 17))
        a, b = m.waic(Wd), m.waic(sliced)
        assert np.array_equal(_bits(a.elpd_i), _bits(b.elpd_i)) and np.array_equal(_bits(a.elpd_i), _bits(m.waic(Wd).elpd_i))


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_predictive_sums_against_float64(S, n, d):
    """mean mu, lppd_i, mean ll and p_waic_i inside the bounds of tests/glm_case.py; `predict_mean` of new rows too."""
    m, W, X, y, o, Wd, _ = _setup(S, n, d)
    ref, b = gc.restatement(W, X, y, o), gc.bounds(W, X, y, o)
    s, f = m._glm.pointwise_sums(Wd), m.waic(Wd)
    got = {"mean_mu": s["sum_mu"] / S, "lppd_i": f.lppd_i, "mean_ll": s["sum_ll"] / S, "p_waic_i": f.p_waic_i}
    ratios = {k: float(np.max(np.abs(got[k] - ref[k]) / b[k])) for k in got}
    print((S, n, d), " ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert np.array_equal(f.p_mean, got["mean_mu"]) and f.n_underflow == 0 and f.n_draws == S
    new = m.predict_mean(Wd, X=X, offset=o)
    assert np.array_equal(_bits(new), _bits(got["mean_mu"]))
    host = m.waic(W)
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
    print("S = %d: khat, elpd_loo_i%s differences %s against the gates %s"
          % (S, ", n_eff, mcse" if mc else "", " ".join("%.3g" % v for v in out), " ".join("%.3g" % v for v in (gk, ge, gn, gm)[:len(out)])))
    assert np.array_equal(got.n_tail, ref.n_tail) and np.array_equal(np.isfinite(got.khat), fin)
    assert dk <= gk and de <= ge, (dk, de)
    if mc:
        assert np.array_equal(got.tail_len_row, ref.tail_len_row)
        assert dn <= gn and dm <= gm, (dn, dm)
    return out


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_finished_numbers_on_the_same_keys(S, n, d):
    """The fused `loo` against `loo_from_log_lik(select="fused")` on the materialised matrix, with and without an r_eff array:
    the tails are identical, only the order of the float64 sums differs -- the gates of `loglik_case.gate(S)`.  Rows whose
    reference tail has fewer than 5 members (khat = inf) are compared on elpd_loo_i only; at S >= 70 there is none.

    The gather adds its terms in the order of `l2hmc_loglik_tails` (segments of consecutive draws, each in draw order), so the
    raw sums, and with them every finished number, are equal bit for bit; the gates are the issue's all the same."""
    import torch
    from l2hmc_amd import psis
    m, _, _, _, _, Wd, ll32 = _setup(S, n, d)
    dev = torch.as_tensor(ll32).cuda()
    for r in (None, lk.r_eff_for(n)):
        got, ref = m.loo(Wd, r_eff=r), psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        fin = np.isfinite(ref.khat)
        short = ref.n_tail < 5
        assert np.array_equal(~fin, short)
        if S >= 70:
            assert not short.any()
        else:                                                # only rows with ties at the cutoff may
            M = ref.tail_len if r is None else ref.tail_len_row
            assert np.all((ref.n_tail < M)[short])
        print((S, n, d), r is not None, " ".join("%.2g" % v for v in _agree(got, ref, S, r is not None, fin)))
        assert got.n_bad == ref.n_bad and got.n_draws == S and got.n_rows == n
        small = m.loo(Wd, r_eff=r, max_tail_bytes=4 * 7 * got.tail_len)          # groups of 7 rows: the same bits
        for k in ("elpd_loo_i", "khat") + (("n_eff", "mcse_elpd_loo_i") if r is not None else ()):
            assert np.array_equal(_bits(small[k]), _bits(got[k])), k


@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_finished_numbers_against_float64(S, n, d):
    """The fused `loo` against the numpy route of the float64 matrix: gates K x delta_i (tests/glm_case.py)."""
    m, W, X, y, o, Wd, _ = _setup(S, n, d)
    delta = gc.bounds(W, X, y, o)["delta"]
    r = lk.r_eff_for(n)
    got, ref = m.loo(Wd, r_eff=r), m.loo(W, r_eff=r)
    fin = np.isfinite(ref.khat)
    assert np.array_equal(fin, np.isfinite(got.khat)) and np.array_equal(got.n_tail, ref.n_tail)
    shares = {"khat": np.max((np.abs(got.khat - ref.khat) / (gc.K_KHAT * delta))[fin]) if fin.any() else 0.0,
              "elpd_loo_i": np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / (gc.K_ELPD * delta)),
              "n_eff": np.max((gc.rel(got.n_eff, ref.n_eff) / (gc.K_NEFF * delta))[fin]) if fin.any() else 0.0,
              "mcse": np.max((gc.rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / (gc.K_MCSE * delta))[fin]) if fin.any() else 0.0}
    print((S, n, d), " ".join("%s %.3g" % (k, float(v)) for k, v in shares.items()))
    assert all(float(v) <= 1.0 for v in shares.values()), shares
    plain, ref0 = m.loo(Wd), m.loo(W)
    assert np.max(np.abs(plain.elpd_loo_i - ref0.elpd_loo_i) / (gc.K_ELPD * delta)) <= 1.0


def test_relative_eff_and_auto_on_an_ar1_history():
    """`relative_eff` of a device history against the float64 host route within K_REFF delta_i; `loo(r_eff="auto")` equals the
    call with that r_eff given, and agrees with `loo_from_log_lik(select="fused")` of the materialised history on the gates
    of `loglik_case`; row groups of `relative_eff` give the same bits."""
    import torch
    import l2hmc_amd
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split, n = gc.AR1
    W, X, y, o = gc.ar1_case()
    m = l2hmc_amd.PoissonRegression(X, y, offset=o)
    Wd = torch.as_tensor(W).cuda()
    delta = gc.bounds(W, X, y, o)["delta"]
    e, ref = m.relative_eff(Wd, max_lag=max_lag, split=split), m.relative_eff(W, max_lag=max_lag, split=split)
    worst = float(np.max(gc.rel(e.r_eff, ref.r_eff) / (gc.K_REFF * delta)))
    print("r_eff %.3g .. %.3g, worst relative error / (K_REFF delta_i) %.3g" % (e.r_eff.min(), e.r_eff.max(), worst))
    assert worst <= 1.0 and e.n_nan == 0 and e.n_draws == M * N
    grouped = m.relative_eff(Wd, max_lag=max_lag, split=split, max_bytes=4 * M * N * 5)
    assert np.array_equal(_bits(grouped.r_eff), _bits(e.r_eff))
    auto, given = m.loo(Wd, r_eff="auto", max_lag=max_lag, split=split), m.loo(Wd, r_eff=e.r_eff)
    for k in ("r_eff", "elpd_loo_i", "khat", "n_eff", "mcse_elpd_loo_i"):
        assert np.array_equal(_bits(auto[k]), _bits(given[k])), k
    ll = m.log_lik(Wd)
    same = psis.loo_from_log_lik(ll, r_eff=e.r_eff, select="fused")
    print(" ".join("%.2g" % v for v in _agree(auto, same, M * N, True, np.isfinite(same.khat))))
