"""GPU: the PSIS-LOO kernels (csrc/loo.hip behind `l2hmc_logistic_loo_tails`) and the device `loo_finish` against the float64
numpy route of the same module on the same float32 inputs.

Gates (tests/loo_case.py; derived from the inputs, never from the code under test).  eps = 2^-24, A_si = sum_k |w_sk| |x_ik|,
delta_i = max_s (d + 8) eps A_si bounds the error of every float32 logit of row i, and order statistics are 1-Lipschitz in the
sup norm: the cutoff and every sorted tail element lie within delta_i of the reference's order statistics; the finished numbers
are gated at K_KHAT delta_i and K_ELPD delta_i (sensitivities of the float64 estimator, profiles/loo_accuracy.txt).

Plan branches (`loo_plan`).  (a) The kernel geometry is chosen by the feature tiles NT = ceil(d / 16): NTM = 1, 2, 4, 8; a
wave holds 32 rows.  (b) A chunk is tpc = ceil(tiles / 1024) 16-draw tiles, raised to 4 when smaller: the floor holds up to
S = 65536, every longer history -- every real one -- has tpc > 4 and about 1024 chunks.  Shapes with at least two draw
chunks AND two row groups (n > 32) in every branch: NTM = 1 (70, 35, 5); NTM = 2 (523, 33, 17) and (4099, 100, 25); NTM = 4
(70, 35, 40); NTM = 8 (300, 50, 128) -- all on the floor tpc = 4 -- and tpc = 5: (65609, 33, 1) [NTM = 1; 4101 tiles, 821
chunks, a last tile of 9 draws, a last chunk of one tile, three dead waves in the last workgroup of a row group] and
(70000, 35, 17) [NTM = 2; 875 chunks]; the exact-input and the row-group checks run at S = 65609 and 70000 too.
(c) Fewer live feature tiles than the compiled geometry holds (the masks `tg < NT` of block_fragments and tile_logits, the
label offset 512 NT, the zeroed LDS columns, tile_load's `e < tile_elems`; csrc/draw_tiles.hpp): NT 3 / NTM 4 is (70, 35, 40),
NT 5 / NTM 8 is (70, 35, 72) (d = 100 and 112 are not used: their reference khat lies within one gate-width of a threshold);
and both beyond the floor, tpc = 5: (65609, 33, 40) [NT 3 / NTM 4] and (65609, 33, 72) [NT 5 / NTM 8], 821 chunks each.
tests/test_loo_cpu.py pins these shapes to their chunk counts.  (4, 3, 2) has M = 0: no tail at all."""
import numpy as np
import pytest
import torch

from tests import loo_case as lc
from tests import predictive_case as pc

pytestmark = pytest.mark.gpu
SHAPES = lc.FIXTURES + [(70, 35, 5), (70, 35, 40), (70, 35, 72), (4, 3, 2)]
# tpc = 5: more than the floor of 4 tiles per chunk; d = 40 and 72 run it with NT 3 / NTM 4 and NT 5 / NTM 8
BIG = [(65609, 33, 1), (70000, 35, 17), (65609, 33, 40), (65609, 33, 72)]
RAW = ("cutoff", "n_tail", "tail", "body", "sum_lik")
_CASES = {}


def _dev(a):
    return torch.as_tensor(a).cuda()


def _host(tails):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in tails.items()}


def _case(S, n, d):
    """Inputs, the numpy route's raw dict and Summary, the device's raw dict (on the host) and Summary: computed once."""
    if (S, n, d) not in _CASES:
        from l2hmc_amd import predictive
        W, X, y = lc.case(S, n, d)
        ref_t = predictive.loo_tails(W, X, y)
        dev_t = predictive.loo_tails(_dev(W), _dev(X), _dev(y))
        _CASES[(S, n, d)] = (W, X, y, ref_t, predictive.loo_finish(ref_t), dev_t, predictive.loo_finish(dev_t))
    return _CASES[(S, n, d)]


def _same_bits(a, b, what=""):
    """Every raw output equal bit for bit; the tail as a sorted row (its slot order is arrival order)."""
    a, b = _host(a), _host(b)
    for k in RAW:
        x, y = (np.sort(v, axis=1) if k == "tail" else v for v in (a[k], b[k]))
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)
    assert a["tail_len"] == b["tail_len"] and a["n_draws"] == b["n_draws"]


def _log_sum_ratios(t, M):
    m = np.minimum(np.asarray(t["cutoff"], dtype=np.float64), 0.0)
    tail = np.asarray(t["tail"], dtype=np.float64)
    with np.errstate(all="ignore"):
        lam = np.where(np.isfinite(tail), np.logaddexp(0.0, -tail), -np.inf)
        return np.logaddexp(np.log(t["body"]) - m, np.logaddexp.reduce(lam, axis=1) if M else -np.inf)


@pytest.mark.parametrize("S,n,d", SHAPES + BIG)
def test_raw_outputs_match_the_numpy_route(S, n, d):
    """cutoff and the sorted tail within delta_i of the reference's order statistics; M - #{|t - c_ref| <= 2 delta_i} <= L <= M;
    the log of the summed ratios (which does not depend on the side near-cutoff draws fell on) within delta_i + 16 eps; sum_lik
    within the predictive bound; slots past L are +inf."""
    W, X, y, ref_t, _, dev_t, _ = _case(S, n, d)
    M = lc.tail_len(S)
    got = _host(dev_t)
    assert got["tail_len"] == M and got["n_draws"] == S
    assert got["cutoff"].dtype == np.float32 and got["tail"].dtype == np.float32 and got["tail"].shape == (n, M)
    assert got["n_tail"].dtype == np.int64 and got["body"].dtype == np.float64 and got["sum_lik"].dtype == np.float64
    di, _ = lc.delta(W, X)
    t = np.sort(lc.signed_logits(W, X, y), axis=0)                     # the reference's order statistics, (S, n)
    assert np.array_equal(t[M], ref_t["cutoff"])
    rc = np.abs(got["cutoff"] - t[M]) / di
    L = got["n_tail"]
    near = (np.abs(t - t[M]) <= 2 * di).sum(axis=0)
    assert np.all(L <= M) and np.all(L >= M - near), (L, M, near)
    tail = np.sort(got["tail"].astype(np.float64), axis=1)
    slot = np.arange(M)[None, :]
    assert np.all(np.where(slot >= L[:, None], tail == np.inf, np.isfinite(tail)))
    rt = np.where(slot < L[:, None], np.abs(tail - t[:M].T), 0.0) / di[:, None]
    rl = np.abs(_log_sum_ratios(got, M) - _log_sum_ratios(ref_t, M)) / (di + 16 * lc.EPS)
    bounds = pc.device_bounds(W, X, y)
    ll = bounds["ll"]
    rs = np.abs(got["sum_lik"] - ref_t["sum_lik"]) / (np.exp(ll) * bounds["B"]).sum(axis=0)
    print("(%d, %d, %d): error / gate  cutoff %.3g  tail %.3g  log sum ratios %.3g  sum_lik %.3g;  L < M on %d rows"
          % (S, n, d, rc.max(), rt.max() if M else 0.0, rl.max(), rs.max(), int(np.sum(L < M))))
    assert rc.max() <= 1.0 and (M == 0 or rt.max() <= 1.0) and rl.max() <= 1.0 and rs.max() <= 1.0


@pytest.mark.parametrize("kind", ["plain", "twice", "half", "constant"])
def test_exact_inputs_give_the_numpy_routes_tails_exactly(kind):
    """Small-integer W and dyadic X: every t is exact in float32 and float64, ties abound.  cutoff, n_tail and the sorted tail
    equal the numpy route EXACTLY, on the plain case and on the three degenerate histories (every draw twice; half the draws
    one vector: L < M on some row; all draws identical: L = 0)."""
    from l2hmc_amd import predictive
    W, X, y = lc.exact_case(210, 37, 19, seed=5)
    if kind != "plain":
        W = lc.degenerate(kind, W)
    ref = predictive.loo_tails(W, X, y)
    got = _host(predictive.loo_tails(_dev(W), X, y))
    M = lc.tail_len(W.shape[0])
    assert np.array_equal(got["cutoff"].astype(np.float64), ref["cutoff"])
    assert np.array_equal(got["n_tail"], ref["n_tail"])
    assert np.array_equal(np.sort(got["tail"].astype(np.float64), axis=1), ref["tail"])
    assert np.max(np.abs(got["body"] - ref["body"]) / ref["body"]) <= 16 * lc.EPS
    if kind == "twice":
        assert M == lc.tail_len(420) and np.all(got["n_tail"] <= M)
    if kind == "half":
        assert np.any(got["n_tail"] < M)
    if kind == "constant":
        assert np.all(got["n_tail"] == 0) and np.all(got["tail"] == np.inf)
        s = predictive.loo_finish(predictive.loo_tails(_dev(W), X, y))
        ll = -np.logaddexp(0.0, -lc.signed_logits(W[:1], X, y)[0])
        assert np.all(s.khat == np.inf) and np.max(np.abs(s.elpd_loo_i - ll)) <= 32 * lc.EPS


def test_exact_inputs_with_more_than_four_tiles_per_chunk():
    """The exact-input check at S = 65609 (tpc = 5, 821 chunks, M = 769): cutoff, n_tail and the sorted tail equal the numpy
    route EXACTLY, ties and all; the body sum within the rounding of its float32 terms."""
    from l2hmc_amd import predictive
    W, X, y = lc.exact_case(65609, 37, 19, seed=6)
    ref = predictive.loo_tails(W, X, y)
    got = _host(predictive.loo_tails(_dev(W), X, y))
    assert got["tail_len"] == lc.tail_len(65609) == 769
    assert np.array_equal(got["cutoff"].astype(np.float64), ref["cutoff"])
    assert np.array_equal(got["n_tail"], ref["n_tail"]) and np.any(got["n_tail"] < 769)
    assert np.array_equal(np.sort(got["tail"].astype(np.float64), axis=1), ref["tail"])
    assert np.max(np.abs(got["body"] - ref["body"]) / ref["body"]) <= 16 * lc.EPS


@pytest.mark.parametrize("S,n,d", SHAPES)
def test_finished_numbers_match_the_numpy_route(S, n, d):
    """khat within K_KHAT delta_i and elpd_loo_i within K_ELPD delta_i of the numpy route, p_loo_i within the sum of that and
    the predictive bound of lppd_i; n_bad and n_above_threshold equal the reference's."""
    W, X, y, _, ref, _, got = _case(S, n, d)
    di, _ = lc.delta(W, X)
    fin = np.isfinite(ref.khat)
    assert np.array_equal(fin, np.isfinite(got.khat)) and np.all(got.khat[~fin] == np.inf)
    lppd_bound = pc.device_bounds(W, X, y)["lppd_i"]
    rk = (np.abs(got.khat - ref.khat)[fin] / (lc.K_KHAT * di[fin])).max() if fin.any() else 0.0
    re_ = (np.abs(got.elpd_loo_i - ref.elpd_loo_i) / (lc.K_ELPD * di)).max()
    rp = (np.abs(got.p_loo_i - ref.p_loo_i) / (lc.K_ELPD * di + lppd_bound)).max()
    print("(%d, %d, %d): error / gate  khat %.3g  elpd_loo_i %.3g  p_loo_i %.3g" % (S, n, d, rk, re_, rp))
    assert rk <= 1.0 and re_ <= 1.0 and rp <= 1.0
    assert got.n_bad == ref.n_bad and got.n_above_threshold == ref.n_above_threshold
    assert got.n_underflow == 0 and got.tail_len == ref.tail_len and np.all(got.n_tail <= got.tail_len)


@pytest.mark.parametrize("S,n,d", [(523, 33, 17), (300, 50, 128), (4099, 100, 25)])
def test_device_finish_matches_numpy_finish_on_the_same_tails(S, n, d):
    """Both float64: library ulps and summation order only (gates: 100 x the worst measured difference, never looser than
    1e-6; tests/loo_case.py).  Row chunks of the device finish change nothing beyond that either."""
    from l2hmc_amd import predictive
    _, _, _, _, _, dev_t, got = _case(S, n, d)
    assert lc.FINISH_KHAT <= 1e-6 and lc.FINISH_ELPD <= 1e-6
    same = predictive.loo_finish(_host(dev_t))
    fin = np.isfinite(same.khat)
    assert np.array_equal(fin, np.isfinite(got.khat))
    dk, de = np.abs(got.khat - same.khat)[fin].max(), np.abs(got.elpd_loo_i - same.elpd_loo_i).max()
    print("(%d, %d, %d): device finish - numpy finish  khat %.3g  elpd_loo_i %.3g" % (S, n, d, dk, de))
    assert dk <= lc.FINISH_KHAT and de <= lc.FINISH_ELPD
    assert np.array_equal(got.n_tail, same.n_tail) and got.n_bad == same.n_bad
    old, predictive._FINISH_CHUNK_BYTES = predictive._FINISH_CHUNK_BYTES, 1
    try:
        one = predictive.loo_finish(dev_t)                             # one row at a time
    finally:
        predictive._FINISH_CHUNK_BYTES = old
    assert np.abs(one.khat - got.khat)[fin].max() <= lc.FINISH_KHAT and np.abs(one.elpd_loo_i - got.elpd_loo_i).max() <= lc.FINISH_ELPD


def test_reproducible_views_slices_and_row_groups():
    """Two calls give identical bits in every raw output; a history (M, N, d) and its (M N, d) view too; a first-axis slice
    x_hist[3:] (a 4-byte aligned base) equals its contiguous copy; max_tail_bytes small enough for 4 row groups gives the bits
    of one group; numpy X and y with device draws go the same way."""
    from l2hmc_amd import predictive
    W, X, y = lc.case(520, 50, 17, seed=77)
    Wd, Xd, yd = _dev(W), _dev(X), _dev(y)
    a = predictive.loo_tails(Wd, Xd, yd)
    _same_bits(a, predictive.loo_tails(Wd, Xd, yd), "second call")
    _same_bits(a, predictive.loo_tails(Wd.reshape(40, 13, 17), Xd, yd), "history view")
    _same_bits(a, predictive.loo_tails(Wd, X, y), "numpy X, y")
    M = lc.tail_len(520)
    grouped = predictive.loo_tails(Wd, Xd, yd, max_tail_bytes=4 * M * 13)           # 13 rows per group: 13 + 13 + 13 + 11
    _same_bits(a, grouped, "4 row groups")
    one = predictive.loo(Wd, Xd, yd)
    many = predictive.loo(Wd, Xd, yd, max_tail_bytes=4 * M * 13)
    assert np.array_equal(one.elpd_loo_i, many.elpd_loo_i) and np.array_equal(one.khat, many.khat)
    # the same at tpc = 5 (S = 70000, M = 794): 12 + 12 + 11 rows against one group of 35, 175 tiles of float64 terms per row
    Wb, Xb, yb = lc.case(*BIG[1])
    Wb = _dev(Wb)
    _same_bits(predictive.loo_tails(Wb, Xb, yb), predictive.loo_tails(Wb, Xb, yb, max_tail_bytes=4 * lc.tail_len(70000) * 12), "3 row groups, tpc 5")
    _same_bits(predictive.loo_tails(Wb, Xb, yb), predictive.loo_tails(Wb.reshape(700, 100, 17), Xb, yb), "history view, tpc 5")
    hist = Wd.reshape(40, 13, 17)
    view = hist[3:]
    assert view.is_contiguous() and view.data_ptr() == hist.data_ptr() + 4 * 3 * 13 * 17 and view.data_ptr() % 16 != 0
    _same_bits(predictive.loo_tails(view, Xd, yd), predictive.loo_tails(view.clone(), Xd, yd), "x_hist[3:]")


def test_end_to_end_on_the_librarys_own_sampler():
    """LogisticRegression n = 100, d = 5; HMC sample_chain(record=True, seed=1), 256 chains x 40 proposals: model.loo(x_hist)
    equals predictive.loo(x_hist, X, y) bit for bit, everything is finite, nothing underflows, and lppd equals that of
    model.waic(x_hist) within the predictive bounds."""
    from l2hmc_amd import Dynamics, LogisticRegression, predictive, sample_chain
    rng = np.random.RandomState(3)
    n, d = 100, 5
    X = rng.randn(n, d).astype(np.float32)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ rng.randn(d)))).astype(np.float32)
    model = LogisticRegression(X, y, prior_var=1.0)
    dyn = Dynamics(d, model.get_energy_function(), T=5, eps=0.08, hmc=True)
    x0 = _dev((0.1 * rng.randn(256, d)).astype(np.float32))
    _, _, hist = sample_chain(x0, dyn, 40, seed=1, record=True)
    kept = hist[10:]
    a, b = model.loo(kept), predictive.loo(kept, X, y)
    for k in ("elpd_loo_i", "khat", "p_loo_i", "lppd_i", "n_tail"):
        assert np.array_equal(a[k], b[k]), k
    assert a.n_draws == 30 * 256 and a.n_rows == n and a.n_underflow == 0
    assert np.all(np.isfinite(a.elpd_loo_i)) and np.all(np.isfinite(a.khat)) and np.isfinite(a.se) and a.elpd_loo < a.lppd
    w = model.waic(kept)
    bound = pc.device_bounds(kept.cpu().numpy(), X, y)["lppd_i"]
    assert np.all(np.abs(a.lppd_i - w.lppd_i) <= 2 * bound) and abs(a.lppd - w.lppd) <= 2 * bound.sum()
    print("elpd_loo %.3f  elpd_waic %.3f  p_loo %.3f  p_waic %.3f  max khat %.3f  n_bad %d" % (
        a.elpd_loo, w.elpd_waic, a.p_loo, w.p_waic, a.khat.max(), a.n_bad))
