"""GPU: the three entries of csrc/glm.hip for the probit family (csrc/glm_probit.hip) called straight
(`probit_case.device_raw`: outputs filled with NaN / -7 before the call and 8 guard elements longer than the entry is told) where
tests/test_gpu_probit_glm.py does not reach -- the mirror of tests/test_gpu_binomial_geometries.py:

  geometries    `probit_case.GEOM_SHAPES`, (70, 35, d) with NT / NTM = 3 / 4 (d = 33, 40), 5 / 8 (65), 6 / 8 (96), 7 / 8 (100,
                112): every in-range element is written, no guard element is, the tails are the exact selection of the written
                matrix, the outputs are the public route's bit for bit, rows [17, n) alone give the bits they have inside the
                whole, and matrix and predictive numbers lie inside `probit_case.ll_bounds`;
  long          `probit_case.LONG`: S > 131072 with three rows, where the gather's segments are no multiple of a tile.
No figure here comes from the device: the bounds are `probit_case.ll_bounds` and `loglik_case.sum_bounds`, the rest is equality."""
import numpy as np
import pytest

from tests import glm_case as gc
from tests import loglik_case as lk
from tests import probit_case as pc

pytestmark = pytest.mark.gpu
RAW = ("ll", "cutoff", "top", "n_tail", "sums")


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _sorted_tail(tail):
    return np.sort(lk.keys(tail), axis=1)                    # (monotone keys: the +inf pads last; a tail never holds a NaN)


def _public(m, Wd, lens):
    """The public route's outputs under the names of `device_raw`."""
    t = {k: v.cpu().numpy() for k, v in m._glm.loo_tails(Wd, tail_len_row=lens).items()}
    s = m._glm.pointwise_sums(Wd)
    return {"ll": m.log_lik(Wd).cpu().numpy(), "cutoff": t["cutoff"], "top": t["top"], "n_tail": t["n_tail"], "tail": t["tail"],
            "sums": np.stack([t["body"], t["body_sq"], t["lik"]]), "flag": t["flag"],
            "psums": np.stack([s["sum_mu"], s["sum_lik"], s["sum_ll"], s["sum_ll2"]])}


def _same(a, b, cols=slice(None), what=""):
    """Two results equal bit for bit (NaNs by position), `a` on the rows `cols`; the tails as sorted rows (their slot order is
    arrival order)."""
    for k in RAW + ("psums",):
        assert gc.same_bits(a[k][..., cols], b[k]), (what, k)
    assert np.array_equal(_sorted_tail(a["tail"][cols])[:, :b["tail"].shape[1]], _sorted_tail(b["tail"])), (what, "tail")
    past = np.sort(a["tail"][cols], axis=1)[:, b["tail"].shape[1]:]
    assert np.all(np.isposinf(past)), (what, "pads")
    assert int(a["flag"][0]) == int(b["flag"][0]) == 0


def _shares(c, res, S):
    """The share of each bound of `probit_case.ll_bounds` the matrix and the predictive numbers use."""
    ll64, _ = pc.log_lik(c)
    b, ref = pc.ll_bounds(c), pc.restatement(c)
    sat = pc.model(c)._glm.consts[2].astype(np.float64)
    got, f = gc.predictive_of(res["psums"], sat, S)
    shares = {"ll": float(np.max(np.abs(res["ll"].astype(np.float64) - ll64) / b["B"]))}
    shares.update({k: float(np.max(np.abs(got[k] - ref[k]) / b[k])) for k in got})
    return shares, f


@pytest.mark.parametrize("S,n,d", pc.GEOM_SHAPES)
def test_raw_entries_write_every_element_and_no_other(S, n, d):
    """With one tail length and with per-row lengths that include 0, 1, 4, 5 and S // 5: no in-range element keeps its fill,
    every guard element does, `check_raw` holds (the exact selection of the written matrix, `l2hmc_loglik_tails` of it bit for
    bit), the outputs are the public route's bit for bit, rows [17, n) in a call of their own give the bits they have inside
    the whole; the matrix within B_si and mean, lppd_i, mean ll and p_waic_i inside `ll_bounds`; at d = 100 `predict_mean` of
    the model's own rows handed back as new ones returns the bits of sum_mu / S."""
    c = pc.case(S, n, d)
    m, Wd = pc.model(c), _dev(c["W"])
    for lens in (None, lk.lengths_for(S, n)):
        res = pc.device_raw(c, Wd, lens)
        assert gc.all_written(res), [k for k in RAW + ("psums", "tail") if res[k].dtype.kind == "f" and np.isnan(res[k]).any()]
        assert gc.guards_untouched(res), res["guards"]
        gc.check_raw(res["ll"], lens, res)
        _same(res, _public(m, Wd, lens), what="public route")
        part = pc.device_raw(c, Wd, lens, rows=(17, n))
        assert gc.all_written(part) and gc.guards_untouched(part)
        _same(res, part, cols=slice(17, n), what="rows [17, n)")
    shares, f = _shares(c, res, S)
    print("probit", (S, n, d), "NT / NTM %d / %d " % (-(-d // 16), 4 if d <= 64 else 8), " ".join("%s %.3g" % kv for kv in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), shares
    assert f.n_underflow == 0 and f.n_draws == S
    if d == 100:
        new = m.predict_mean(Wd, X=c["X"], offset=c["offset"], trials=c["trials"])
        assert gc.same_bits(new, res["psums"][0] / S)


@pytest.mark.parametrize("S,n,d", pc.LONG)
def test_ragged_segment_tiles_under_late_loads(S, n, d):
    """`glm_case.check_raw` (the exact selection of the written matrix, its sums inside `loglik_case.sum_bounds`, bit equality
    with `l2hmc_loglik_tails` of it) with one tail length and with per-row lengths; the matrix within B_si of the float64
    likelihood; the mean, lppd_i, mean ll and p_waic_i within `probit_case.ll_bounds`."""
    c = pc.case(S, n, d)
    Wd = _dev(c["W"])
    for lens in (None, lk.lengths_for(S, n)):
        res = pc.device_raw(c, Wd, lens)
        assert gc.all_written(res) and gc.guards_untouched(res)
        gc.check_raw(res["ll"], lens, res)
    shares, f = _shares(c, res, S)
    print("probit", (S, n, d), " ".join("%s %.3g" % kv for kv in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), shares
    assert f.n_underflow == 0 and f.n_draws == S
