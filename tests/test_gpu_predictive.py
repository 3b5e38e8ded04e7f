"""GPU: the posterior-predictive / WAIC kernel (csrc/predictive.hip behind `l2hmc_logistic_predict`) against the float64
numpy path of the same module on the same float32 inputs.

Gates (derived from the inputs, tests/predictive_case.py `device_bounds`; never from the code under test).  With eps = 2^-24,
A_si = sum_k |w_sk| |x_ik| and B_si = (d + 8) eps A_si + 8 eps (1 + |ll_si|):
    |d p_mean| <= mean_s B / 4,  |d lppd_i| <= max_s B,  |d mean ll| <= mean_s B,
    |d p_waic_i| <= (2 sd_i max_s B + (max_s B)^2) S / (S - 1) + 4 S 2^-52 mean_s ll^2.
The worst measured ratio of each quantity is in profiles/predictive_accuracy.txt (tools/predictive_accuracy.py)."""
import numpy as np
import pytest
import torch

from tests import predictive_case as pc

pytestmark = pytest.mark.gpu
SHAPES = [(21, 1, 1), (37, 17, 3), (16, 16, 16), (523, 33, 17), (300, 50, 128), (4099, 100, 25),
          # live feature tiles NT = ceil(d / 16) under the compiled NTM: 3 / 4 (the first launch of predict_kernel<4, 2>) and
          # 4 / 4, 5 / 8, 7 / 8 with a full last tile -- the masks `tg < NT` of block_fragments and tile_logits, the label offset
          # 512 NT, the zeroed LDS columns and tile_load's `e < tile_elems` (csrc/draw_tiles.hpp); two row groups each
          (70, 35, 40), (70, 35, 50), (70, 35, 72), (70, 35, 112)]
SUMS = ("sum_p", "sum_lik", "sum_ll", "sum_ll2")
_CASES = {}


def _case(S, n, d, **kw):
    """Inputs, the host path's Summary (with mean_ll) and the bounds, computed once and shared."""
    key = (S, n, d) + tuple(sorted(kw.items()))
    if key not in _CASES:
        from l2hmc_amd import predictive
        W, X, y = pc.case(S, n, d, seed=1000 + S + n + d, **kw)
        _CASES[key] = (W, X, y, _finished(predictive.pointwise_sums(W, X, y)), pc.device_bounds(W, X, y))
    return _CASES[key]


def _finished(sums):
    from l2hmc_amd import predictive
    f = predictive.finish(sums)
    f["mean_ll"] = np.asarray(sums["sum_ll"]) / sums["n_draws"]
    return f


def _dev(a):
    return torch.as_tensor(a).cuda()


def _gate(got, ref, bounds, what):
    r = pc.ratios(got, ref, bounds)
    print("%s: error / bound  p_mean %.3g  lppd_i %.3g  mean ll %.3g  p_waic_i %.3g" % (
        what, r["p_mean"], r["lppd_i"], r["mean_ll"], r["p_waic_i"]))
    for k, v in r.items():
        assert v <= 1.0, (what, k, v)
    return r


@pytest.mark.parametrize("S,n,d", SHAPES)
def test_sums_and_finished_numbers_match_the_host_path(S, n, d):
    """The smallest shapes that exercise every mask: a last draw tile with 5, 5, 16, 11, 12 and 3 live draws, a last data block
    with 1, 1, 16, 1, 2 and 4 live rows, d below, at and across the 16-feature tiles; logits reach +-10.  The (70, 35, d) shapes
    run fewer live feature tiles than the compiled geometry holds (d = 40, 72, 112) and the full NTM = 4 (d = 50)."""
    from l2hmc_amd import predictive
    W, X, y, ref, bounds = _case(S, n, d)
    sums = predictive.pointwise_sums(_dev(W), _dev(X), _dev(y))
    for k in SUMS:
        assert sums[k].dtype == np.float64 and sums[k].shape == (n,) and np.all(np.isfinite(sums[k])), k
    assert sums["n_draws"] == S
    got = _finished(sums)
    _gate(got, ref, bounds, "(%d, %d, %d)" % (S, n, d))
    # the totals follow from the rows: the sum of the per-row bounds gates them
    assert abs(got.lppd - ref.lppd) <= bounds["lppd_i"].sum() and abs(got.p_waic - ref.p_waic) <= bounds["p_waic_i"].sum()
    assert abs(got.elpd_waic - ref.elpd_waic) <= (bounds["lppd_i"] + bounds["p_waic_i"]).sum()
    assert got.n_underflow == 0 and got.n_high_variance == ref.n_high_variance
    assert np.max(np.abs(predictive.predict_proba(_dev(W), X) - ref.p_mean) / bounds["p_mean"]) <= 1.0
    # numpy X and y with device draws go the same way
    assert np.array_equal(predictive.pointwise_sums(_dev(W), X, y)["sum_ll"], sums["sum_ll"])


def test_padded_tail_of_the_last_draw_tile_contributes_nothing():
    """(37, 17, 3): the same call on the draws padded by hand to 48 with copies of real draws, minus those copies' exact
    contribution, equals the call on the 37 draws within the device error of the 11 copies -- so the 11 lanes past S in the
    last tile of the unpadded call added nothing (a zero draw would add p1 = 0.5, lik = 0.5, ll = -log 2: far outside)."""
    from l2hmc_amd import predictive
    W, X, y, _, bounds = _case(37, 17, 3)
    extra = W[5:16]
    plain = predictive.pointwise_sums(_dev(W), X, y)
    padded = predictive.pointwise_sums(_dev(np.concatenate([W, extra])), X, y)
    exact = predictive.pointwise_sums(extra, X, y)
    assert padded["n_draws"] == 48 and exact["n_draws"] == 11
    B, ll = bounds["B"][5:16], bounds["ll"][5:16]
    gates = {"sum_p": B.sum(axis=0) / 4, "sum_lik": (np.exp(ll) * B).sum(axis=0), "sum_ll": B.sum(axis=0),
             "sum_ll2": (2 * np.abs(ll) * B + B * B).sum(axis=0)}
    for k in SUMS:
        err = np.abs(padded[k] - exact[k] - plain[k])
        print("%s: worst |padded - copies - plain| / gate %.3g" % (k, np.max(err / gates[k])))
        assert np.all(err <= gates[k]), k


def test_history_slices_are_read_in_place():
    """x_hist (9, 7, 3) on the device: x_hist[1:] and x_hist[3:] start 21 and 63 floats into the allocation (4-byte aligned
    bases).  They give the numbers of their .clone() bit for bit and match the host path within the gate."""
    from l2hmc_amd import predictive
    W, X, y = pc.case(63, 20, 3, seed=7)
    hist = _dev(W.reshape(9, 7, 3))
    for first in (1, 3):
        view = hist[first:]
        assert view.is_contiguous() and view.data_ptr() == hist.data_ptr() + 4 * 21 * first
        a = predictive.pointwise_sums(view, X, y)
        b = predictive.pointwise_sums(view.clone(), X, y)
        for k in SUMS:
            assert np.array_equal(a[k], b[k]), (first, k)
        Wv = W.reshape(9, 7, 3)[first:]
        _gate(_finished(a), _finished(predictive.pointwise_sums(Wv, X, y)), pc.device_bounds(Wv, X, y), "x_hist[%d:]" % first)


def test_two_calls_give_identical_bits_and_draws_are_additive():
    """(4099, 100, 25): two calls return identical float64 sums; the sums of draws[:1000] plus those of draws[1000:] equal
    the sums of all draws to 1e-12 relative (float64 sums of the same float32 values in another order) -- the basis of the
    sharded path."""
    from l2hmc_amd import predictive
    W, X, y, _, _ = _case(4099, 100, 25)
    Wd, Xd, yd = _dev(W), _dev(X), _dev(y)
    a = predictive.pointwise_sums(Wd, Xd, yd)
    b = predictive.pointwise_sums(Wd, Xd, yd)
    head = predictive.pointwise_sums(Wd[:1000], Xd, yd)
    tail = predictive.pointwise_sums(Wd[1000:], Xd, yd)
    assert head["n_draws"] + tail["n_draws"] == 4099
    for k in SUMS:
        assert np.array_equal(a[k], b[k]), k
        assert np.all(np.abs(head[k] + tail[k] - a[k]) <= 1e-12 * np.abs(a[k])), k


@pytest.mark.parametrize("labels", ["ones", "zeros"])
def test_constant_labels_and_no_labels(labels):
    """All-ones and all-zeros labels within the gate; y = None gives the same sum_p bit for bit as any labels."""
    from l2hmc_amd import predictive
    W, X, y, ref, bounds = _case(523, 33, 17, labels=labels)
    sums = predictive.pointwise_sums(_dev(W), X, y)
    _gate(_finished(sums), ref, bounds, "labels %s" % labels)
    none = predictive.pointwise_sums(_dev(W), X)
    rand = predictive.pointwise_sums(_dev(W), X, _case(523, 33, 17)[2])
    assert np.array_equal(none["sum_p"], sums["sum_p"]) and np.array_equal(rand["sum_p"], sums["sum_p"])
    assert np.array_equal(predictive.predict_proba(_dev(W), X), sums["sum_p"] / 523)


def test_saturated_logits_stay_finite_and_within_the_gate():
    """Logits up to +-60, by scaling X: sigmoid saturates to 1 - 2^-24 and below, exp(-60) = 8.8e-27 is far above the smallest
    float32 -- everything is finite, within the gate, and nothing underflows."""
    from l2hmc_amd import predictive
    W, X, y, ref, bounds = _case(523, 33, 17, max_logit=60.0, x_scale=8.0)
    assert 59.0 < np.abs(W.astype(np.float64) @ X.astype(np.float64).T).max() < 61.0
    sums = predictive.pointwise_sums(_dev(W), X, y)
    got = _finished(sums)
    for k in SUMS:
        assert np.all(np.isfinite(sums[k])), k
    assert np.all(np.isfinite(got.lppd_i)) and got.n_underflow == 0
    _gate(got, ref, bounds, "logits +-60")


def test_end_to_end_on_the_librarys_own_sampler():
    """LogisticRegression n = 100, d = 5; HMC sample_chain(record=True, seed=1), 256 chains x 60 proposals:
    model.waic(x_hist[10:]) on the device against waic on the host copy, model.predict_proba on new rows likewise; a float64
    device tensor and a non-contiguous one (x_hist[10::2]) are accepted and agree with the host path."""
    from l2hmc_amd import Dynamics, LogisticRegression, predictive, sample_chain
    rng = np.random.RandomState(3)
    n, d = 100, 5
    X = rng.randn(n + 40, d).astype(np.float32)
    w_true = rng.randn(d)
    y = (rng.rand(n + 40) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ w_true))).astype(np.float32)
    X_test, X, y = X[n:], X[:n], y[:n]
    model = LogisticRegression(X, y, prior_var=1.0)
    dyn = Dynamics(d, model.get_energy_function(), T=5, eps=0.08, hmc=True)
    x0 = _dev((0.1 * rng.randn(256, d)).astype(np.float32))
    _, _, hist = sample_chain(x0, dyn, 60, seed=1, record=True)
    assert tuple(hist.shape) == (60, 256, d) and hist.is_cuda
    kept = hist[10:]
    host = kept.cpu().numpy()
    bounds = pc.device_bounds(host, X, y)
    got = model.waic(kept)
    ref = predictive.waic(host, X, y)
    got["mean_ll"] = ref["mean_ll"] = np.zeros(n)              # (not part of a Summary: gated through p_waic_i and lppd_i)
    _gate(got, ref, bounds, "sampler history")
    assert got.n_draws == 50 * 256 and abs(got.elpd_waic - ref.elpd_waic) <= (bounds["lppd_i"] + bounds["p_waic_i"]).sum()
    pb = pc.device_bounds(host, X_test, np.zeros(40))["p_mean"]
    assert np.all(np.abs(model.predict_proba(kept, X_test) - predictive.predict_proba(host, X_test)) <= pb)
    for other, other_host in ((kept.double(), host), (hist[10::2], host[::2])):
        assert other.dtype == torch.float64 or not other.is_contiguous()
        g, r = model.waic(other), predictive.waic(other_host, X, y)
        g["mean_ll"] = r["mean_ll"] = np.zeros(n)
        _gate(g, r, pc.device_bounds(other_host, X, y), "dtype %s contiguous %s" % (other.dtype, other.is_contiguous()))
