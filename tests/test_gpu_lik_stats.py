"""GPU: the likelihood-statistics kernels (csrc/lik_stats.hip behind `l2hmc_logistic_lik_stats`) and
`predictive.relative_eff` on the device against float64 on the same float32 inputs.

Gates (tests/lik_stats_case.py; derived from the inputs and the float64 route, never from the kernel).  The raw sums are held
to the bounds derived there: |d mean| <= mean_t e, |d M2| <= 2 sqrt(M2 sum e^2) + sum e^2, |d G_t| <= sum_c [...] + 64 eps G_0
with e = lik B the error of one float32 likelihood.  The kernel folds its float32 products into float64 every 8 steps, not
every 32 as csrc/chain_stats.hip does: its own term is (2 + 8) eps G_0, inside the 64 eps G_0 that is gated.  The finished
r_eff is held at K_REFF delta_i relative (a measured sensitivity of the float64 estimator, profiles/lik_stats_accuracy.txt) on
the rows whose Geyer truncation index does not move under +-delta_si in the float64 route; at most 10 % of a fixture's rows
may be excluded that way, and on the others the truncation flags must agree.

Plan branches (`lik_stats_plan`): the geometry NTM = 1, 2, 4, 8 by d; chain blocks of 16 with a ragged last one; one wave per
16-row block (n = 37: three, the last with 5 rows); lag tiles of 8 with a ragged last one; both halves of a split."""
import numpy as np
import pytest
import torch

from tests import lik_stats_case as ls
from tests import loo_case as lc

pytestmark = pytest.mark.gpu
_CASES = {}


def _dev(a):
    return torch.as_tensor(a).cuda()


_raw = ls.device_raw


def _case(fixture):
    """Inputs, the numpy route's Summary and the device's: computed once."""
    if fixture not in _CASES:
        from l2hmc_amd import predictive
        M, N, d, rho, max_lag, split = fixture
        W, X, y = ls.ar1_case(M, N, d, rho)
        ref = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
        got = predictive.relative_eff(_dev(W), X, y, max_lag=max_lag, split=split)
        _CASES[fixture] = (W, X, y, ref, got)
    return _CASES[fixture]


@pytest.mark.parametrize("fixture", ls.FIXTURES)
def test_raw_sums_within_their_derived_bounds(fixture):
    """(a) mean, M2 and G of the kernel against float64, each within the bound derived from the inputs (module docstring);
    every output element is written."""
    M, N, d, rho, max_lag, split = fixture
    W, X, y = ls.ar1_case(M, N, d, rho)
    ref, bound = ls.raw_bounds(W, X, y, max_lag, split)
    got = dict(zip(("mean", "m2", "G"), _raw(W, X, y, max_lag, split)))
    for k in ("mean", "m2", "G"):
        assert got[k].shape == ref[k].shape and np.all(np.isfinite(got[k])), k
        r = float(np.max(np.abs(got[k] - ref[k]) / bound[k]))
        print("%s %-4s worst error / bound %.3g" % (fixture, k, r))
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("fixture", ls.FIXTURES)
def test_relative_eff_matches_the_numpy_route(fixture):
    """(b) r_eff within K_REFF delta_i (relative) of the numpy route and the same truncation flags, on the rows away from a
    truncation boundary; the Summary's other fields equal."""
    W, X, y, ref, got = _case(fixture)
    _, near, _ = ls.sensitivity(fixture)
    assert near.mean() <= ls.EXCLUDED_AT_MOST
    di, _ = ls.delta(W, X)
    keep = ~near
    assert np.all(np.isfinite(got.r_eff)) and got.r_eff.dtype == np.float64
    r = np.abs(got.r_eff / ref.r_eff - 1.0) / (ls.K_REFF * di)
    print("%s r_eff worst relative error / (K_REFF delta_i) %.3g over %d rows" % (fixture, r[keep].max(), keep.sum()))
    assert np.all(r[keep] <= 1.0)
    assert np.array_equal(got.truncated[keep], ref.truncated[keep])
    for k in ("n_draws", "n_steps", "n_chains", "max_lag", "n_nan"):
        assert got[k] == ref[k], k
    assert np.array_equal(got.r_eff, got.ess / got.n_draws)


def test_two_calls_and_any_row_grouping_give_the_same_bits():
    """(f) Two calls agree bit for bit, and so do calls whose rows go to the kernel in groups of 5 and of 16 (a row changes its
    16-row block and its lane)."""
    from l2hmc_amd import _ffi, predictive
    for fixture in (ls.FIXTURES[1], ls.FIXTURES[2], ls.FIXTURES[8]):
        M, N, d, rho, max_lag, split = fixture
        W, X, y, _, got = _case(fixture)
        Wd = _dev(W)
        again = predictive.relative_eff(Wd, X, y, max_lag=max_lag, split=split)
        assert np.array_equal(again.ess.view(np.uint8), got.ess.view(np.uint8))
        C = N * (2 if split else 1)
        per_row = 16 * C + _ffi.lib().l2hmc_logistic_lik_stats_workspace_bytes(M, N, d, 1, max_lag, int(split))
        for rows in (5, 16):
            grouped = predictive.relative_eff(Wd, X, y, max_lag=max_lag, split=split, max_bytes=rows * per_row)
            assert np.array_equal(grouped.ess.view(np.uint8), got.ess.view(np.uint8)), (fixture, rows)
            assert np.array_equal(grouped.truncated, got.truncated)
    a, b = _raw(W, X, y, max_lag, split), _raw(W, X, y, max_lag, split)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


def test_a_first_axis_slice_is_read_in_place():
    """(h) x_hist[k:] goes to the kernel where it lies (no copy) and gives the bits of its contiguous copy."""
    from l2hmc_amd import predictive
    from l2hmc_amd._history import in_place
    M, N, d, rho, max_lag, split = ls.FIXTURES[6]
    W, X, y = ls.ar1_case(M + 7, N, d, rho)
    Wd = _dev(W)
    cut = Wd[7:]
    assert in_place(cut).data_ptr() == cut.data_ptr() == Wd.data_ptr() + 7 * N * d * 4
    a = predictive.relative_eff(cut, X, y, max_lag=max_lag)
    b = predictive.relative_eff(cut.clone(), X, y, max_lag=max_lag)
    assert np.array_equal(a.ess.view(np.uint8), b.ess.view(np.uint8))
    assert a.n_steps == M and a.n_draws == M * N and np.all(np.isfinite(a.r_eff))


def test_degenerate_histories_on_the_device():
    """All draws identical: every r_eff is NaN, as on the host.  One NaN draw: every row meets it, every r_eff is NaN.  One NaN
    feature of ONE data row: that row's r_eff alone is NaN and the others keep their bits."""
    from l2hmc_amd import predictive
    fixture = ls.FIXTURES[7]
    M, N, d, rho, max_lag, split = fixture
    W, X, y, _, got = _case(fixture)
    const = np.broadcast_to(W[:1, :1], W.shape).copy()
    s = predictive.relative_eff(_dev(const), X, y, max_lag=max_lag)
    assert np.all(np.isnan(s.r_eff)) and s.n_nan == X.shape[0] and not s.truncated.any()
    bad = W.copy()
    bad[5, 2, 0] = np.nan
    s = predictive.relative_eff(_dev(bad), X, y, max_lag=max_lag)
    assert np.all(np.isnan(s.r_eff)) and s.n_nan == X.shape[0]
    Xb = X.copy()
    Xb[20, 1] = np.nan
    s = predictive.relative_eff(_dev(W), Xb, y, max_lag=max_lag)
    other = np.arange(X.shape[0]) != 20
    assert np.isnan(s.r_eff[20]) and s.n_nan == 1
    assert np.array_equal(s.ess[other].view(np.uint8), got.ess[other].view(np.uint8))


def test_the_model_method_on_the_device():
    import l2hmc_amd
    from l2hmc_amd import predictive
    fixture = ls.FIXTURES[5]
    M, N, d, rho, max_lag, split = fixture
    W, X, y, _, got = _case(fixture)
    model = l2hmc_amd.LogisticRegression(X, y, prior_var=2.0)
    s = model.relative_eff(_dev(W), max_lag=max_lag)
    assert np.array_equal(s.ess.view(np.uint8), got.ess.view(np.uint8))
    default = predictive.relative_eff(_dev(W), X, y)
    assert default.max_lag == M - 1 and default.n_chains == N and default.n_steps == M


def test_exact_inputs_hold_the_raw_sums_to_the_sigmoid_alone():
    """Small-integer W and dyadic X: the float32 logits are the float64 ones, so the likelihood's error is the hardware
    sigmoid's alone, e = lik 8 eps (1 + |ll|), and mean, M2 and G are held to the bounds derived from that e (many ties, many
    equal likelihoods, logits up to +-40: saturated series among them)."""
    for M, N, d, n, max_lag, split in ((48, 20, 5, 37, 17, False), (33, 18, 20, 21, 15, True)):
        W, X, y = ls.exact_case(M, N, d, n, 7 + M)
        ref, bound = ls.raw_bounds(W, X, y, max_lag, split, exact=True)
        got = dict(zip(("mean", "m2", "G"), _raw(W, X, y, max_lag, split)))
        for k in ("mean", "m2", "G"):
            err = np.abs(got[k] - ref[k])
            with np.errstate(all="ignore"):
                r = np.where(err == 0, 0.0, err / bound[k])              # (a constant series: 0 <= 0)
            print("exact %s %-4s worst error / bound %.3g" % ((M, N, d), k, r.max()))
            assert np.all(r <= 1.0), (k, r.max())


def _host(t):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in t.items()}


@pytest.mark.parametrize("S,n,d", lc.FIXTURES)
def test_uniform_lengths_give_the_old_entry_bits(S, n, d):
    """(c) `l2hmc_logistic_loo_tails_mc` with every length M = tail_len(S): cutoff, n_tail, the tail as a set, body and sum_lik
    equal `l2hmc_logistic_loo_tails`' bit for bit."""
    from l2hmc_amd import predictive
    W, X, y = lc.case(S, n, d)
    M = lc.tail_len(S)
    old = _host(predictive.loo_tails(_dev(W), X, y))
    new = _host(predictive.loo_tails(_dev(W), X, y, tail_len_row=np.full(n, M)))
    assert new["tail_len"] == old["tail_len"] == M and new["tail"].shape == (n, M) and new["body_sq"].shape == (n,)
    for k in ("cutoff", "n_tail", "tail", "body", "sum_lik"):
        a, b = (np.sort(v, axis=1) if k == "tail" else v for v in (old[k], new[k]))
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def _log_sums(t):
    """(log of the summed importance ratios, log of the summed SQUARED ratios): neither depends on the side of the cutoff a
    draw fell on"""
    m = np.minimum(np.asarray(t["cutoff"], dtype=np.float64), 0.0)
    tail = np.asarray(t["tail"], dtype=np.float64)
    with np.errstate(all="ignore"):
        lam = np.where(np.isfinite(tail), np.logaddexp(0.0, -tail), -np.inf)
        return (np.logaddexp(np.log(t["body"]) - m, np.logaddexp.reduce(lam, axis=1)),
                np.logaddexp(np.log(t["body_sq"]) - 2.0 * m, np.logaddexp.reduce(2.0 * lam, axis=1)))


@pytest.mark.parametrize("fixture", [ls.FIXTURES[0], ls.FIXTURES[2], ls.FIXTURES[3], ls.FIXTURES[5]])
def test_per_row_lengths_match_the_numpy_route(fixture):
    """(d) Per-row lengths M_i: cutoff and the sorted tail within delta_i of the reference's order statistics of rank M_i;
    M_i - #{|t - c_ref| <= 2 delta_i} <= L_i <= M_i; slots past L_i are +inf up to the stride; the log of the summed ratios
    within delta_i + 16 eps as in tests/test_gpu_loo.py, and the log of the summed SQUARED ratios (e^-2m body_sq plus the tail's)
    within 2 (delta_i + 16 eps): every ratio 1 + e^-t moves by at most a relative delta_i + 16 eps, its square by twice that,
    and the sum of all of them does not depend on the side of the cutoff a draw fell on.  Two calls and row groups: same bits."""
    from l2hmc_amd import predictive
    M, N, d, rho, max_lag, split = fixture
    W, X, y, ref_s, _ = _case(fixture)
    S, n = M * N, X.shape[0]
    lens = predictive.tail_len_rows(ref_s.r_eff, S)
    assert lens.min() < lens.max() or (M, N) == (40, 5)
    ref_t = predictive.loo_tails(W, X, y, tail_len_row=lens)
    got = _host(predictive.loo_tails(_dev(W), X, y, tail_len_row=lens))
    di, _ = ls.delta(W, X)
    t = np.sort(ls.signed_logits(W, X, y).reshape(S, n), axis=0)
    c_ref = t[lens, np.arange(n)]
    assert np.max(np.abs(c_ref - ref_t["cutoff"])) <= 1e-12 and got["tail"].shape == (n, lens.max())   # (another matmul shape)
    L = got["n_tail"]
    near = (np.abs(t - c_ref) <= 2 * di).sum(axis=0)
    assert np.all(L <= lens) and np.all(L >= lens - near), (L, lens, near)
    tail = np.sort(got["tail"].astype(np.float64), axis=1)
    slot = np.arange(lens.max())[None, :]
    assert np.all(np.where(slot >= L[:, None], tail == np.inf, np.isfinite(tail)))
    rc = np.abs(got["cutoff"] - c_ref) / di
    rt = np.where(slot < L[:, None], np.abs(tail - t[:lens.max()].T), 0.0) / di[:, None]
    (l1, l2), (r1, r2) = _log_sums(got), _log_sums(ref_t)
    rl = np.abs(l1 - r1) / (di + 16 * ls.EPS)
    rq = np.abs(l2 - r2) / (2 * (di + 16 * ls.EPS))
    print("%s cutoff %.3g tail %.3g log-sum %.3g log-sum-sq %.3g of their bounds" % (fixture, rc.max(), rt.max(), rl.max(), rq.max()))
    assert rc.max() <= 1 and rt.max() <= 1 and rl.max() <= 1 and rq.max() <= 1
    again = _host(predictive.loo_tails(_dev(W), X, y, tail_len_row=lens))
    grouped = _host(predictive.loo_tails(_dev(W), X, y, tail_len_row=lens, max_tail_bytes=4 * int(lens.max()) * 5))
    for other in (again, grouped):
        for k in ("cutoff", "n_tail", "tail", "body", "sum_lik", "body_sq"):
            a, b = (np.sort(v, axis=1) if k == "tail" else v for v in (got[k], other[k]))
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


@pytest.mark.parametrize("fixture", ls.FIXTURES)
def test_loo_with_r_eff_auto_matches_the_numpy_route(fixture):
    """(e) `loo(r_eff="auto")` on the device, both finishes, against the numpy route: khat and elpd_loo_i at K_KHAT delta_i and
    K_ELPD delta_i (tests/loo_case.py), n_eff and mcse_elpd_loo_i at K_NEFF delta_i and K_MCSE delta_i relative, on the rows
    away from a truncation boundary (at most 10 % excluded); the device finishes against the numpy finish on the same tails at
    FINISH_NEFF / FINISH_MCSE."""
    from l2hmc_amd import predictive
    M, N, d, rho, max_lag, split = fixture
    W, X, y = ls.ar1_case(M, N, d, rho)
    _, near, _, _ = ls.loo_sensitivity(fixture)
    assert near.mean() <= ls.EXCLUDED_AT_MOST
    keep = ~near
    di, _ = ls.delta(W, X)
    ref = predictive.loo(W, X, y, r_eff="auto")
    for finish in ("torch", "kernel"):
        got = predictive.loo(_dev(W), X, y, finish=finish, r_eff="auto")
        fin = np.isfinite(ref.khat) & keep
        assert np.array_equal(np.isfinite(got.khat), np.isfinite(ref.khat))
        rk = np.abs(got.khat - ref.khat)[fin] / (lc.K_KHAT * di[fin])
        re_ = np.abs(got.elpd_loo_i - ref.elpd_loo_i)[keep] / (lc.K_ELPD * di[keep])
        rn = np.abs(got.n_eff / ref.n_eff - 1.0)[keep] / (ls.K_NEFF * di[keep])
        rm = np.abs(got.mcse_elpd_loo_i / ref.mcse_elpd_loo_i - 1.0)[keep] / (ls.K_MCSE * di[keep])
        print("%s %-6s khat %.3g elpd %.3g n_eff %.3g mcse %.3g of their gates; %d rows with another M_i" % (
            fixture, finish, rk.max(), re_.max(), rn.max(), rm.max(), int(np.sum(got.tail_len_row != ref.tail_len_row))))
        assert rk.max() <= 1 and re_.max() <= 1 and rn.max() <= 1 and rm.max() <= 1
        assert got.n_reff_nan == 0 and got.tail_len == int(got.tail_len_row.max())
        assert np.isnan(got.mcse_elpd_loo) == np.isnan(ref.mcse_elpd_loo)
        # the same device tails through the numpy finish
        dev_t = predictive.loo_tails(_dev(W), X, y, tail_len_row=got.tail_len_row)
        same = predictive.loo_finish(_host(dev_t), r_eff=got.r_eff)
        mine = predictive.loo_finish(dev_t, finish=finish, r_eff=got.r_eff)
        fn = float(np.max(np.abs(mine.n_eff / same.n_eff - 1.0)))
        fm = float(np.max(np.abs(mine.mcse_elpd_loo_i / same.mcse_elpd_loo_i - 1.0)))
        print("%s %-6s device finish - numpy finish: n_eff %.3g mcse %.3g (relative)" % (fixture, finish, fn, fm))
        assert fn <= ls.FINISH_NEFF and fm <= ls.FINISH_MCSE


def test_exact_inputs_with_per_row_lengths():
    """(g) Small-integer W and dyadic X: cutoffs, n_tail and tails equal the numpy route exactly with per-row lengths, ties
    included."""
    from l2hmc_amd import predictive
    for M, N, d, n in ((48, 20, 5, 37), (33, 18, 20, 21)):
        W, X, y = ls.exact_case(M, N, d, n, 7 + M)
        S = M * N
        lens = np.random.RandomState(M).randint(0, S // 5 + 1, size=n)
        ref = predictive.loo_tails(W, X, y, tail_len_row=lens)
        got = _host(predictive.loo_tails(_dev(W), X, y, tail_len_row=lens))
        assert np.array_equal(got["cutoff"].astype(np.float64), ref["cutoff"]) and np.array_equal(got["n_tail"], ref["n_tail"])
        assert np.array_equal(np.sort(got["tail"].astype(np.float64), axis=1), ref["tail"])
        assert np.any(ref["n_tail"] < lens)                  # ties at the cutoff shorten some tails


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_loo_with_r_eff_in_row_groups_gives_the_one_group_result():
    """`loo(r_eff=array)` whose 50 rows go to the kernels in four groups of 13 against the one-group call, both finishes, per-row
    tail lengths 49 .. 104 and one NaN efficiency.  The tails' bits do not depend on the grouping, nor do the kernel finish's
    khat and elpd_loo_i.  n_eff, mcse_elpd_loo_i and the torch finish's numbers pass through torch reductions whose order could
    depend on the chunk's shape (13 rows against 50); their gates would be the finish-against-finish ones of tests/loo_case.py
    and tests/lik_stats_case.py, but on the MI355X every field is bit-equal under both finishes, so that is what is asserted
    (the gates are stated after it: they say how far a field may move before the test's premise is gone)."""
    from l2hmc_amd import predictive
    W, X, y = lc.case(520, 50, 17, seed=77)
    r = 0.2 + 1.8 * np.random.RandomState(77).rand(50)
    r[11] = np.nan
    lens = predictive.tail_len_rows(r, 520)
    Mmax = int(lens.max())
    assert lens.min() < Mmax and -(-50 // 13) == 4
    Wd = _dev(W)
    live = ~np.isnan(r)
    for finish in ("torch", "kernel"):
        one = predictive.loo(Wd, X, y, finish=finish, r_eff=r)
        four = predictive.loo(Wd, X, y, finish=finish, r_eff=r, max_tail_bytes=4 * Mmax * 13)
        assert np.array_equal(one.tail_len_row, lens) and one.tail_len == four.tail_len == Mmax and four.n_reff_nan == 1
        fin = np.isfinite(one.khat)
        assert np.all(np.isnan(four.n_eff[~live])) and np.all(np.isnan(four.mcse_elpd_loo_i[~live]))
        assert np.all(np.isfinite(four.n_eff[live])) and np.all(np.isfinite(four.mcse_elpd_loo_i[live]))
        dk = float(np.max(np.abs(one.khat - four.khat)[fin]))
        de = float(np.max(np.abs(one.elpd_loo_i - four.elpd_loo_i)))
        dn = float(np.max(np.abs(four.n_eff / one.n_eff - 1.0)[live]))
        dm = float(np.max(np.abs(four.mcse_elpd_loo_i / one.mcse_elpd_loo_i - 1.0)[live]))
        print("%-6s four groups - one group: khat %.3g elpd_loo_i %.3g n_eff %.3g mcse %.3g (the last two relative)"
              % (finish, dk, de, dn, dm))
        for k in ("n_tail", "tail_len_row", "khat", "elpd_loo_i", "n_eff", "mcse_elpd_loo_i"):
            assert _bits_equal(one[k], four[k]), (finish, k)
        assert dk <= lc.FINISH_KHAT and de <= lc.FINISH_ELPD and dn <= ls.FINISH_NEFF and dm <= ls.FINISH_MCSE
