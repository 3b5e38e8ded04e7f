"""GPU: the three entries of csrc/glm.hip called straight (`glm_case.device_raw_glm`: outputs filled with NaN / -7 before the
call and 8 guard elements longer than the entry is told) where tests/test_gpu_glm.py does not reach:

  geometries    every shape of `glm_case.SHAPES` -- with (70, 35, d) every count of live feature tiles below the compiled one,
                NT / NTM = 3 / 4 (d = 33, 40), 5 / 8 (65), 6 / 8 (96), 7 / 8 (100, 112): every in-range element is written, no
                guard element is, and the outputs are the public route's bit for bit (whose `torch.empty` outputs would not
                show an element the kernel skipped);
  long          S > 131072 with three rows, where the gather's segments are no multiple of a tile and the loads are issued
                late (`kLate`: the gather at NTM >= 4, the predictive sums at NTM = 8): S = 131073 (65-draw segments: four tiles
                and one of ONE draw; a last segment of 33 draws) at d = 40, S = 140001 (69 = 4 x 16 + 5; 140001 = 2029 x 69, so
                the last segment is a full one) at d = 40 and 100, and S = 140003 (a last segment of 2 draws) at d = 100;
                tests/test_glm_cpu.py pins the segment and chunk counts;
  edges         `glm_case.edge_case`: float32 overflow of mu in fewer and in more draws than the tail holds (ll = -inf: a finite
                and an infinite cutoff), a row constant at -0.0, a row whose likelihood underflows in every draw, a count of
                100000 -- against the float64 likelihood, the exact selection of the written matrix, `l2hmc_loglik_tails` of
                it, `loo_from_log_lik(select="fused")` of it and the same ordinary rows in a model without the edge rows;
  one NaN draw  every row's sums and maximum are NaN, the other 4098 draws of the matrix keep their bits (the 15 other draws of
                its tile share its MFMA operand), the selection is the exact one of the numbers.
No figure here comes from the device: the bounds are `glm_case.bounds` and `loglik_case.sum_bounds`, the rest is equality."""
import numpy as np
import pytest

from tests import glm_case as gc
from tests import loglik_case as lk

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
LONG = [(131073, 3, 40), (140001, 3, 40), (140001, 3, 100), (140003, 3, 100)]
RAW = ("ll", "cutoff", "top", "n_tail", "sums", "psums")
_EDGE = {}


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _sorted_tail(tail):
    return np.sort(lk.keys(tail), axis=1)                    # (monotone keys: the +inf pads last; a tail never holds a NaN)


def _public(m, Wd, lens):
    """The public route's outputs under the names of `device_raw_glm`."""
    t = {k: v.cpu().numpy() for k, v in m._glm.loo_tails(Wd, tail_len_row=lens).items()}
    s = m._glm.pointwise_sums(Wd)
    return {"ll": m.log_lik(Wd).cpu().numpy(), "cutoff": t["cutoff"], "top": t["top"], "n_tail": t["n_tail"], "tail": t["tail"],
            "sums": np.stack([t["body"], t["body_sq"], t["lik"]]), "flag": t["flag"],
            "psums": np.stack([s["sum_mu"], s["sum_lik"], s["sum_ll"], s["sum_ll2"]])}


def _same(a, b, cols=slice(None), what=""):
    """Two results of `device_raw_glm` / `_public` equal bit for bit (NaNs by position), `a` on the rows `cols`; the tails as
    sorted rows (their slot order is arrival order)."""
    for k in RAW:
        assert gc.same_bits(a[k][..., cols], b[k]), (what, k)
    assert np.array_equal(_sorted_tail(a["tail"][cols])[:, :b["tail"].shape[1]], _sorted_tail(b["tail"])), (what, "tail")
    past = np.sort(a["tail"][cols], axis=1)[:, b["tail"].shape[1]:]
    assert np.all(np.isposinf(past)), (what, "pads")
    assert int(a["flag"][0]) == int(b["flag"][0]) == 0


# ---- every geometry, with poisoned outputs and guards --------------------------------------------------------------------------
@pytest.mark.parametrize("S,n,d", gc.SHAPES)
def test_raw_entries_write_every_element_and_no_other(S, n, d):
    """With one tail length and with per-row lengths that include 0, 1, 4, 5 and S // 5: no in-range element keeps its fill,
    every guard element does, and matrix, cutoff, top, n_tail, the sorted tail, the three tail sums and the four predictive
    sums are the public route's bit for bit; rows [17, n) in a call of their own give the bits they have inside the whole."""
    import l2hmc_amd
    W, X, y, o = gc.case(S, n, d)
    m, Wd = l2hmc_amd.PoissonRegression(X, y, offset=o), _dev(W)
    for lens in (None, lk.lengths_for(S, n)):
        res = gc.device_raw_glm((X, y, o), Wd, lens)
        assert gc.all_written(res), [k for k in RAW + ("tail",) if res[k].dtype.kind == "f" and np.isnan(res[k]).any()]
        assert gc.guards_untouched(res), res["guards"]
        _same(res, _public(m, Wd, lens), what="public route")
        if n > 17:
            part = gc.device_raw_glm((X, y, o), Wd, lens, rows=(17, n))
            assert gc.all_written(part) and gc.guards_untouched(part)
            _same(res, part, cols=slice(17, n), what="rows [17, n)")


# ---- long histories where the loads are late -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n,d", LONG)
def test_ragged_segment_tiles_under_late_loads(S, n, d):
    """`glm_case.check_raw` (the exact selection of the written matrix, its sums inside `loglik_case.sum_bounds`, bit equality
    with `l2hmc_loglik_tails` of it) with one tail length and with per-row lengths; the matrix within B_si of the float64
    likelihood; mean mu, lppd_i, mean ll and p_waic_i within the bounds of `glm_case.bounds`."""
    from l2hmc_amd import glm
    W, X, y, o = gc.case(S, n, d)
    Wd = _dev(W)
    for lens in (None, lk.lengths_for(S, n)):
        res = gc.device_raw_glm((X, y, o), Wd, lens)
        assert gc.all_written(res) and gc.guards_untouched(res)
        gc.check_raw(res["ll"], lens, res)
    ll64, _ = gc.log_lik(W, X, y, o)
    b, ref = gc.bounds(W, X, y, o), gc.restatement(W, X, y, o)
    ratio = float(np.max(np.abs(res["ll"].astype(np.float64) - ll64) / b["B"]))
    got, f = gc.predictive_of(res["psums"], glm.row_constants(y, o)[2].astype(np.float64), S)
    ratios = {k: float(np.max(np.abs(got[k] - ref[k]) / b[k])) for k in got}
    print((S, n, d), "ll / B %.3g " % ratio, " ".join("%s %.3g" % kv for kv in ratios.items()))
    assert ratio <= 1.0 and all(v <= 1.0 for v in ratios.values()), (ratio, ratios)
    assert f.n_underflow == 0 and f.n_draws == S


# ---- the edges of the Poisson likelihood ---------------------------------------------------------------------------------------
def _edge(S):
    """The edge case, its model, the draws on the device and the raw outputs with one tail length: computed once."""
    if S not in _EDGE:
        import l2hmc_amd
        W, X, y, o, ordinary = gc.edge_case(S)
        Wd = _dev(W)
        _EDGE[S] = (W, X, y, o, ordinary, l2hmc_amd.PoissonRegression(X, y, offset=o), Wd, gc.device_raw_glm((X, y, o), Wd))
    return _EDGE[S]


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_matrix_against_float64(S):
    """-inf exactly where the float64 ll lies below -FLT_MAX (mu overflowed) and finite elsewhere; -0.0 bit for bit in the
    constant row (the float64 value there, -e^h = -1e-52, is below the float32 range and B, a relative bound, does not
    speak of a flush to zero); within B_si wherever |ll64| lies inside the float32 range."""
    W, X, y, o, _, _, _, res = _edge(S)
    assert gc.guards_untouched(res) and int(res["flag"][0]) == 0
    ll32 = res["ll"]
    ll64, _ = gc.log_lik(W, X, y, o)
    B = gc.bounds(W, X, y, o)["B"]
    over = ll64 < -FLT_MAX
    zero = gc.EDGE_ROWS["zero"]
    assert np.array_equal(np.isneginf(ll32), over) and np.all(np.isfinite(ll32[~over]))
    assert np.all(gc.bits(ll32[:, zero]) == 0x80000000) and np.all(np.abs(ll64[:, zero]) < 2.0 ** -149)
    inside = ~over
    inside[:, zero] = False
    assert np.all(np.abs(ll64[inside]) >= 2.0 ** -126)
    ratio = float(np.max((np.abs(ll32.astype(np.float64) - ll64) / B)[inside]))
    print("S = %d: %d elements at -inf, worst |ll32 - ll64| / bound elsewhere %.3g" % (S, int(over.sum()), ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_tails_are_the_exact_selection_of_the_matrix(S):
    """With one tail length and with per-row lengths: cutoff, top, n_tail and the sorted tail are `loglik_case.select_exact` of
    the written matrix, the sums lie inside `sum_bounds` (NaN where a draw at -inf stands outside the tail of a row whose
    cutoff is -inf), and all of them equal `l2hmc_loglik_tails` of the written matrix bit for bit, NaNs by position."""
    _, X, y, o, _, _, Wd, first = _edge(S)
    ll32, M, at = first["ll"], gc.tail_len(S), gc.EDGE_ROWS
    n = ll32.shape[1]
    for lens in (None, lk.lengths_for(S, n)):
        res = first if lens is None else gc.device_raw_glm((X, y, o), Wd, lens)
        eff = np.full(n, M, dtype=np.int64) if lens is None else lens
        ex = lk.select_exact(ll32, eff)
        assert int(res["flag"][0]) == 0 and gc.guards_untouched(res) and gc.same_bits(res["ll"], ll32)
        assert np.array_equal(gc.bits(res["cutoff"]), gc.bits(ex["cutoff"])) and np.array_equal(gc.bits(res["top"]), gc.bits(ex["top"]))
        assert np.array_equal(res["n_tail"], ex["n_tail"]) and res["tail"].shape == (n, int(eff.max()))
        for i in range(n):
            L = int(ex["n_tail"][i])
            assert np.all(np.isposinf(res["tail"][i, L:])), i
            assert sorted(lk.keys(res["tail"][i, :L]).tolist()) == [p[0] for p in ex["pairs"][i]], i
        ref, bound = lk.sum_bounds(ll32, ex)
        assert lk.sums_within(res["sums"], ref, bound), (res["sums"], ref, bound)
        mat = lk.device_raw(ll32, lens, want_pos=False)
        for k in ("cutoff", "top", "n_tail", "sums"):
            assert gc.same_bits(res[k], mat[k]), k
        assert np.array_equal(_sorted_tail(res["tail"]), _sorted_tail(mat["tail"]))
    res = first
    few, many, zero = at["overflow_few"], at["overflow_many"], at["zero"]
    n_inf = np.isneginf(ll32).sum(axis=0)
    assert np.isfinite(res["cutoff"][few]) and res["n_tail"][few] == M and np.isneginf(res["tail"][few]).sum() == n_inf[few] >= 1
    assert np.isneginf(res["cutoff"][many]) and res["n_tail"][many] == 0 and n_inf[many] > M and np.isfinite(res["top"][many])
    assert np.isnan(res["sums"][:2, many]).all() and np.isfinite(res["sums"][2, many])
    assert gc.bits(res["cutoff"])[zero] == gc.bits(res["top"])[zero] == 0x80000000 and res["n_tail"][zero] == 0
    assert np.array_equal(res["sums"][:, zero], [S, S, S])
    rest = np.ones(n, dtype=bool)
    rest[many] = False
    assert np.all(np.isfinite(res["sums"][:, rest])) and np.all(res["n_tail"] <= M)


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_finished_numbers_are_those_of_the_materialised_route(S):
    """`loo` against `loo_from_log_lik(select="fused")` of the written matrix, with and without r_eff: the same NaN / inf
    pattern and the same bits elsewhere (the raw material is the same bit for bit and the finish is the same code)."""
    from l2hmc_amd import psis
    _, _, _, _, ordinary, m, Wd, first = _edge(S)
    n = first["ll"].shape[1]
    dev = _dev(first["ll"])
    for r in (None, lk.r_eff_for(n)):
        got, ref = m.loo(Wd, r_eff=r), psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        for k in ("khat", "elpd_loo_i", "lppd_i", "n_tail") + (("n_eff", "mcse_elpd_loo_i", "tail_len_row") if r is not None else ()):
            assert gc.same_bits(np.asarray(got[k]), np.asarray(ref[k])), (k, got[k], ref[k])
        assert np.all(np.isfinite(got.elpd_loo_i[ordinary])) and np.all(np.isfinite(got.khat[ordinary]))
        assert np.isnan(got.elpd_loo_i[gc.EDGE_ROWS["overflow_many"]]) and got.khat[gc.EDGE_ROWS["zero"]] == np.inf


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_ordinary_rows_do_not_depend_on_the_edge_rows(S):
    """The 32 ordinary rows equal, bit for bit, the same rows of the model without the edge rows: matrix, cutoff, top, n_tail,
    the sorted tail, the tail sums and the predictive sums, with one tail length and with per-row lengths."""
    W, X, y, o, ordinary, _, Wd, first = _edge(S)
    lens = lk.lengths_for(S, X.shape[0])
    assert lens[ordinary].max() == lens.max()
    for ln, res in ((None, first), (lens, gc.device_raw_glm((X, y, o), Wd, lens))):
        alone = gc.device_raw_glm((X[ordinary], y[ordinary], o[ordinary]), Wd, None if ln is None else ln[ordinary])
        assert gc.all_written(alone) and gc.guards_untouched(alone)
        _same(res, alone, cols=ordinary, what="without the edge rows")


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_predictive_sums_follow_the_written_matrix(S):
    """sum ll, sum ll^2 and sum exp(ll - sat) against extended-precision sums of the written float32 matrix: S 2^-53 relative to
    the sum of the terms' magnitudes for the additions in whatever order (sum ll^2 is one fma per term), and per term of the
    third the bound of `loglik_case.sum_bounds` -- (|ll - sat| + 2) (2^-52 + the reference's epsilon); infinite exactly where
    the reference is.  sum mu is +inf in the overflow rows, 0 in the constant row and within mean Bmu elsewhere.  The underflow
    row has sum_lik = 0 and lppd_i = -inf, and it is the one row `n_underflow` counts, as on the host route."""
    from l2hmc_amd import glm
    W, X, y, o, _, m, Wd, res = _edge(S)
    at, ld = gc.EDGE_ROWS, np.longdouble
    ps, ll = res["psums"], res["ll"].astype(ld)
    s = m._glm.pointwise_sums(Wd)
    assert gc.same_bits(ps, np.stack([s["sum_mu"], s["sum_lik"], s["sum_ll"], s["sum_ll2"]]))
    sat = glm.row_constants(y, o)[2].astype(ld)
    u = ld(2.0) ** -53
    with np.errstate(all="ignore"):
        lik = np.exp(ll - sat)
        per_term = np.where(lik == 0, ld(0), lik * (np.abs(ll - sat) + 2) * (2 * u + ld(np.finfo(ld).eps)))      # (a zero term is exact)
        want = {1: (lik.sum(axis=0), per_term.sum(axis=0) + S * u * lik.sum(axis=0)),
                2: (ll.sum(axis=0), S * u * np.abs(ll).sum(axis=0)), 3: ((ll * ll).sum(axis=0), S * u * (ll * ll).sum(axis=0))}
        for k, (ref, bound) in want.items():
            ref, bound = ref.astype(np.float64), bound.astype(np.float64)
            fin = np.isfinite(ref)
            assert np.array_equal(ps[k][~fin], ref[~fin]) and np.all(np.abs(ps[k] - ref)[fin] <= bound[fin]), (k, ps[k], ref, bound)
    over = np.isneginf(res["ll"]).any(axis=0)
    assert over.sum() == 2 and np.all(np.isposinf(ps[0][over])) and ps[0][at["zero"]] == 0.0
    _, h = gc.log_lik(W, X, y, o)
    plain = ~over
    plain[at["zero"]] = False
    assert np.all((np.abs(ps[0] / S - np.exp(h).mean(axis=0)) <= gc.bounds(W, X, y, o)["mean_mu"])[plain])
    f, host = m.waic(Wd), m.waic(W)
    assert ps[1][at["underflow"]] == 0.0 and np.isneginf(f.lppd_i[at["underflow"]])
    assert f.n_underflow == host.n_underflow == 1


# ---- one NaN draw --------------------------------------------------------------------------------------------------------------
def test_one_nan_draw():
    """(4099, 35, 17) with a NaN in coordinate 5 of draw 1234: the matrix is NaN in that draw for every row and keeps the clean
    call's bits in every other draw; every row's top, tail sums and predictive sums are NaN; cutoff, n_tail and the tail are
    the exact selection of the numbers (a NaN's key is the last: it is never in a tail); the error word is 0; `relative_eff`
    (of the first 4098 draws as two chains) counts every row in n_nan and `loo` returns NaN for every row, quietly."""
    import l2hmc_amd
    W, X, y, o, bad = gc.nan_case()
    S, n = W.shape[0], X.shape[0]
    clean, got = gc.device_raw_glm((X, y, o), W), gc.device_raw_glm((X, y, o), bad)
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
    m = l2hmc_amd.PoissonRegression(X, y, offset=o)
    hist = _dev(bad)[:S - 1].reshape((S - 1) // 2, 2, 17)    # (4099 is a prime and the diagnostics need two chains: 2049 x 2)
    e = m.relative_eff(hist)
    assert e.n_nan == n and np.isnan(e.r_eff).all()
    s = m.loo(_dev(bad), r_eff=lk.r_eff_for(n))
    assert np.isnan(s.elpd_loo_i).all() and np.isnan(s.khat).all()
