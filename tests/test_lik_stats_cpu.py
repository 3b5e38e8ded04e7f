"""CPU: the per-row relative efficiency of PSIS-LOO -- `l2hmc_amd.predictive.relative_eff`'s numpy route against the direct
restatement of tests/lik_stats_case.py, the fixtures' own preconditions, degenerate histories, refusals, the C ABI's argument
validation and the compiler's listing of the new unit."""
import os
import re

import numpy as np
import pytest

from tests import lik_stats_case as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _ref(fixture):
    if fixture not in _REF:
        M, N, d, rho, max_lag, split = fixture
        W, X, y = ls.ar1_case(M, N, d, rho)
        _REF[fixture] = (W, X, y, ls.restatement(W, X, y, max_lag, split))
    return _REF[fixture]


@pytest.mark.parametrize("fixture", ls.FIXTURES)
def test_numpy_route_matches_the_direct_restatement(fixture):
    """r_eff within 1e-10 (about 1e-13 measured: another summation order), the truncation flags equal; a CPU tensor and the
    host's row chunking (one row at a time) change nothing; the Summary's fields."""
    import torch
    from l2hmc_amd import diagnostics, predictive
    M, N, d, rho, max_lag, split = fixture
    W, X, y, ref = _ref(fixture)
    got = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
    dr = float(np.max(np.abs(got.r_eff - ref["r_eff"])))
    print("numpy route - restatement: r_eff %.2g" % dr)
    assert dr <= 1e-10 and np.array_equal(got.truncated, ref["truncated"])
    assert isinstance(got, diagnostics.Summary) and np.array_equal(got.r_eff, got.ess / (M * N))
    Mh = M // 2 if split else M
    assert (got.n_draws, got.n_steps, got.n_chains, got.max_lag) == (M * N, Mh, N * (2 if split else 1), max_lag)
    assert got.n_nan == 0 and got.n_truncated == int(ref["truncated"].sum())
    tens = predictive.relative_eff(torch.as_tensor(W), torch.as_tensor(X), torch.as_tensor(y), max_lag=max_lag, split=split)
    assert np.array_equal(tens.r_eff, got.r_eff)
    old, predictive._HOST_CHUNK_ELEMS = predictive._HOST_CHUNK_ELEMS, M * N
    try:
        one = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
    finally:
        predictive._HOST_CHUNK_ELEMS = old
    assert np.max(np.abs(one.r_eff - ref["r_eff"])) <= 1e-10 and np.array_equal(one.truncated, ref["truncated"])


def test_fixtures_have_the_properties_they_were_chosen_for():
    """From the restatement alone: r_eff inside a loose band (3/4 of the low end .. 5/4 of the high end) around the range each
    fixture was chosen for, no NaN, at most one truncated row in the one fixture that may have one and none elsewhere, a tail
    length M_i that differs from the uncorrelated M on every row of the rho = 0.7 cases and lies on both sides of it in the iid
    case, the cap S // 5 binding on every row of the smallest case -- and at most 10 % of a fixture's rows so near a truncation
    boundary that +-delta_si moves their truncation index."""
    for fixture in ls.FIXTURES:
        M, N, d, rho, max_lag, split = fixture
        ref, near, worst = ls.sensitivity(fixture)
        r, S = ref["r_eff"], M * N
        Mi, M1 = ls.tail_lengths(r, S), int(ls.tail_lengths(np.ones(1), S)[0])
        print(fixture, "r_eff %.3f .. %.3f, %d truncated, %d near a boundary, M_i %d .. %d against %d, sensitivity %.3g"
              % (r.min(), r.max(), ref["truncated"].sum(), near.sum(), Mi.min(), Mi.max(), M1, worst))
        assert np.all(np.isfinite(r)) and np.all(r > 0)
        if fixture in ls.R_EFF_RANGE:
            lo, hi = ls.R_EFF_RANGE[fixture]
            assert 0.75 * lo <= r.min() and r.max() <= 1.25 * hi, (fixture, r.min(), r.max())
        assert ref["truncated"].sum() <= (1 if fixture == ls.MAY_TRUNCATE else 0), fixture
        assert near.mean() <= ls.EXCLUDED_AT_MOST
        assert worst <= ls.K_REFF / 4 * 1.0000001, "tests/lik_stats_case.py K_REFF is stale: run tools/lik_stats_accuracy.py"
        if rho == 0.7:
            assert np.all(Mi != M1) and np.all(Mi > 2 * M1)
        if rho == 0.0:
            assert Mi.min() < M1 < Mi.max()
        if (M, N) == (40, 5):
            assert np.all(Mi == S // 5)


def test_degenerate_histories():
    """All draws identical: a constant series, r_eff = NaN on every row.  One NaN draw: its chain meets every row, every r_eff
    is NaN.  One NaN feature of one data row: that row alone."""
    from l2hmc_amd import predictive
    fixture = ls.FIXTURES[7]
    M, N, d, rho, max_lag, split = fixture
    W, X, y, ref = _ref(fixture)
    const = np.broadcast_to(W[:1, :1], W.shape).copy()
    s = predictive.relative_eff(const, X, y, max_lag=max_lag)
    assert np.all(np.isnan(s.r_eff)) and s.n_nan == ls.N_ROWS and not s.truncated.any() and s.n_truncated == 0
    bad = W.copy()
    bad[5, 2, 0] = np.nan
    s = predictive.relative_eff(bad, X, y, max_lag=max_lag)
    assert np.all(np.isnan(s.r_eff)) and s.n_nan == ls.N_ROWS
    Xb = X.copy()
    Xb[20, 1] = np.nan
    s = predictive.relative_eff(W, Xb, y, max_lag=max_lag)
    other = np.arange(ls.N_ROWS) != 20
    assert np.isnan(s.r_eff[20]) and s.n_nan == 1 and np.max(np.abs(s.r_eff[other] - ref["r_eff"][other])) <= 1e-10


def test_defaults_exports_and_the_model_method():
    """`split=False` and max_lag = min(steps - 1, diagnostics.DEFAULT_MAX_LAG) by default; r_eff is what `diagnostics.summarize`
    gives for the likelihoods as a history."""
    import l2hmc_amd
    from l2hmc_amd import diagnostics, predictive
    assert l2hmc_amd.relative_eff is predictive.relative_eff and "relative_eff" in l2hmc_amd.__all__
    fixture = ls.FIXTURES[5]
    M, N, d, rho, max_lag, split = fixture
    W, X, y, _ = _ref(fixture)
    got = predictive.relative_eff(W, X, y)
    assert got.max_lag == min(M - 1, diagnostics.DEFAULT_MAX_LAG) and got.n_steps == M and got.n_chains == N
    direct = diagnostics.summarize(ls.likelihoods(ls.signed_logits(W, X, y)), split=False)
    assert np.max(np.abs(got.ess - direct.ess)) <= 1e-9 * np.max(direct.ess)
    both = predictive.relative_eff(W, X, y, split=True)
    assert both.n_steps == M // 2 and both.n_chains == 2 * N and both.n_draws == M * N
    model = l2hmc_amd.LogisticRegression(X, y, prior_var=2.0)
    assert np.array_equal(model.relative_eff(W).r_eff, got.r_eff)
    assert np.array_equal(model.relative_eff(W, max_lag=7, split=True).r_eff, predictive.relative_eff(W, X, y, 7, True).r_eff)


def test_bad_arguments_raise_value_error():
    from l2hmc_amd import predictive
    W, X, y = ls.ar1_case(40, 5, 2, 0.5)
    bad_y = y.copy()
    bad_y[2] = 0.5
    for args, kw in (((W.reshape(-1, 2), X, y), {}),         # a matrix of draws: the chains are not known
                     ((W, X[:, :1], y), {}), ((W, X, bad_y), {}), ((W, X, y[:5]), {}), ((W, X[0], y), {}), ((W, X, None), {}),
                     ((W, X, y), {"max_lag": 40}), ((W, X, y), {"max_lag": -1}), ((W, X, y), {"max_lag": 20, "split": True}),
                     ((W[:3], X, y), {}), ((W[:7], X, y), {"split": True}), ((W[:, :1], X, y), {})):
        with pytest.raises(ValueError):
            predictive.relative_eff(*args, **kw)
    assert predictive.relative_eff(W[:, :1], X, y, split=True).n_chains == 2          # one chain, split in two


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the two entries (ABI version still 6); the workspace is the
    partial lag sums of at most 16 chain-block walkers, linear in the rows and independent of d; every L2HMC_ERR_ARG case of
    `chain_stats_plan` and `logistic_history_args_ok` is refused with a message before anything is launched."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_logistic_lik_stats_workspace_bytes", "l2hmc_logistic_lik_stats"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws, stats = L.l2hmc_logistic_lik_stats_workspace_bytes, L.l2hmc_logistic_lik_stats
    for (M, N, d, n, lag, split) in ((200, 20, 3, 37, 63, 0), (81, 20, 3, 37, 39, 1), (64, 48, 17, 37, 31, 0), (1000, 4096, 25, 1000, 255, 0),
                                     (1000, 4096, 128, 1000, 255, 1)):
        walkers = min((N + 15) // 16, 16)
        assert ws(M, N, d, n, lag, split) == (2 if split else 1) * walkers * n * (lag + 1) * 8, (M, N, d, n, lag, split)
    assert ws(1000, 4096, 25, 1, 255, 0) * 1000 == ws(1000, 4096, 25, 1000, 255, 0)
    for (M, N, d, n, lag, split), msg in (((0, 20, 3, 10, 1, 0), b">= 1"), ((200, 0, 3, 10, 1, 0), b">= 1"), ((200, 20, 0, 10, 1, 0), b">= 1"),
                                          ((200, 20, 3, 10, 1, 2), b"split 0 or 1"), ((3, 20, 3, 10, 1, 0), b">= 4 steps"),
                                          ((7, 20, 3, 10, 1, 1), b">= 4 steps"), ((200, 1, 3, 10, 1, 0), b">= 2 chains"),
                                          ((200, 20, 3, 10, 200, 0), b"max_lag"), ((200, 20, 3, 10, -1, 0), b"max_lag"),
                                          ((200, 20, 3, 10, 100, 1), b"max_lag"), ((200, 20, 3, 0, 1, 0), b"n_data"),
                                          ((200, 20, 3, (1 << 20) + 1, 1, 0), b"n_data"), ((200, 20, 129, 10, 1, 0), b"<= d <= 128"),
                                          (((1 << 31) + 1, 20, 3, 10, 1, 0), b"too large"), ((1 << 20, 1 << 21, 3, 10, 1, 0), b"too large"),
                                          ((1 << 20, (1 << 20) // 25 + 1, 25, 10, 1, 0), b"too large")):
        assert ws(M, N, d, n, lag, split) == -1, (M, N, d, n, lag, split)
        assert msg in L.l2hmc_last_error(), ((M, N, d, n, lag, split), L.l2hmc_last_error())
        assert stats(None, M, N, d, None, n, lag, split, None, None, None, None, None) == -1
        assert msg in L.l2hmc_last_error(), ((M, N, d, n, lag, split), L.l2hmc_last_error())
    assert stats(None, 200, 20, 3, None, 10, 63, 0, None, None, None, None, None) == -1              # valid shape, NULL pointers
    assert b"required" in L.l2hmc_last_error()
    ok = 1 << 12                                             # an aligned non-NULL address: refused before it is touched
    for at in (0, 4, 8, 9, 10, 11):
        args = [ok, 200, 20, 3, ok, 10, 63, 0, ok, ok, ok, ok, None]
        args[at] = ok + (2 if at == 0 else 4)
        assert stats(*args) == -1 and b"aligned" in L.l2hmc_last_error(), at
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(stats(None, 200, 20, 3, None, 10, 63, 0, None, None, None, None, None))


@pytest.mark.parametrize("fixture", ls.FIXTURES)
def test_loo_with_r_eff_matches_the_direct_restatement(fixture):
    """The numpy route of `loo(r_eff="auto")` against the restatement (a full sort, M_i from r_eff_i, n_eff and mcse from the
    normalised weight vector): khat and elpd_loo_i within 1e-10 as in tests/test_loo_cpu.py, n_eff and mcse within 1e-10
    relative, n_tail and tail_len_row equal; an r_eff array gives what "auto" gives; loo = loo_finish(loo_tails)."""
    from l2hmc_amd import predictive
    M, N, d, rho, max_lag, split = fixture
    W, X, y, _ = _ref(fixture)
    ref, _, sn, sm = ls.loo_sensitivity(fixture)
    assert sn <= ls.K_NEFF / 4 * 1.0000001 and sm <= ls.K_MCSE / 4 * 1.0000001, "K_NEFF / K_MCSE are stale"
    got = predictive.loo(W, X, y, r_eff="auto")
    fin = np.isfinite(ref["khat"])
    assert np.array_equal(fin, np.isfinite(got.khat))
    dk = float(np.max(np.abs(got.khat - ref["khat"])[fin]))
    de = float(np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])))
    dn = float(np.max(np.abs(got.n_eff / ref["n_eff"] - 1.0)))
    dm = float(np.max(np.abs(got.mcse_elpd_loo_i / ref["mcse"] - 1.0)))
    print("numpy route - restatement: khat %.2g elpd_loo_i %.2g n_eff %.2g mcse %.2g (relative)" % (dk, de, dn, dm))
    assert max(dk, de, dn, dm) <= 1e-10
    assert np.array_equal(got.n_tail, ref["n_tail"]) and np.array_equal(got.tail_len_row, ref["tail_len_row"])
    assert got.tail_len == int(ref["tail_len_row"].max()) and got.n_reff_nan == 0
    assert np.max(np.abs(got.r_eff - ref["r_eff"])) <= 1e-10 and got.min_n_eff == float(got.n_eff.min())
    want = float(np.sqrt(np.sum(got.mcse_elpd_loo_i ** 2))) if not np.any(got.khat > 0.7) else np.nan
    assert np.array_equal(got.mcse_elpd_loo, want, equal_nan=True)
    arr = predictive.loo(W, X, y, r_eff=got.r_eff)
    assert np.array_equal(arr.n_eff, got.n_eff) and np.array_equal(arr.elpd_loo_i, got.elpd_loo_i)
    lens = predictive.tail_len_rows(got.r_eff, M * N)
    two = predictive.loo_finish(predictive.loo_tails(W, X, y, tail_len_row=lens), r_eff=got.r_eff)
    assert np.array_equal(two.n_eff, got.n_eff) and np.array_equal(two.mcse_elpd_loo_i, got.mcse_elpd_loo_i)


def test_the_torch_finish_agrees_with_the_numpy_finish_on_host_tensors():
    """`_loo_rows` with the Monte Carlo extras over torch's operations (CPU tensors here; the device route runs the same lines)
    against numpy's on the same tails with per-row lengths: rows whose tail is shorter than the stride have dead slots, which
    must add nothing."""
    import torch
    from l2hmc_amd import predictive
    fixture = ls.FIXTURES[3]
    M, N, d, rho, max_lag, split = fixture
    W, X, y, ref = _ref(fixture)
    lens = predictive.tail_len_rows(ref["r_eff"], M * N)
    assert lens.min() < lens.max()
    t = predictive.loo_tails(W, X, y, tail_len_row=lens)
    keys = ("cutoff", "n_tail", "tail", "body", "sum_lik", "body_sq")
    middle, S, Mmax = predictive._MIDDLES["torch"], M * N, int(lens.max())
    a = predictive._loo_rows(predictive._Numpy(), middle, S, Mmax, *(t[k] for k in keys), ref["r_eff"])
    b = predictive._loo_rows(predictive._Torch(), middle, S, Mmax, *(torch.as_tensor(t[k]) for k in keys), torch.as_tensor(ref["r_eff"]))
    assert len(a) == len(b) == 5
    for u, v in zip(a, b):
        v = v.numpy()
        assert np.all(np.isfinite(v)) and np.max(np.abs(v / u - 1.0)) <= 1e-10


def test_r_eff_none_is_the_old_summary_and_ones_change_no_estimate():
    """`r_eff=None` returns the old keys and values exactly; an r_eff of ones has every M_i = M: the same khat and elpd_loo_i,
    and n_eff equals `psis.psis`' n_eff on the same ratios; NaN r_eff: M_i as for 1, NaN in both fields, counted; mcse_elpd_loo
    is NaN when a khat exceeds 0.7."""
    from l2hmc_amd import predictive, psis
    from tests import loo_case as lc
    old_keys = {"elpd_loo_i", "p_loo_i", "lppd_i", "khat", "n_tail", "elpd_loo", "p_loo", "lppd", "looic", "se", "khat_threshold",
                "n_bad", "n_above_threshold", "tail_len", "n_draws", "n_rows", "n_underflow"}
    for W, X, y in (ls.ar1_case(200, 20, 3, 0.7), lc.case(523, 33, 17)):
        n = X.shape[0]
        S = int(np.prod(W.shape[:-1]))
        none = predictive.loo(W, X, y, r_eff=None)
        plain = predictive.loo(W, X, y)
        assert set(none) == old_keys
        for k in old_keys:
            assert np.array_equal(none[k], plain[k], equal_nan=True), k
        ones = predictive.loo(W, X, y, r_eff=np.ones(n))
        assert np.all(ones.tail_len_row == predictive.loo_tail_len(S)) and ones.tail_len == none.tail_len
        assert np.array_equal(ones.khat, none.khat) and np.array_equal(ones.elpd_loo_i, none.elpd_loo_i)
        assert np.array_equal(ones.n_tail, none.n_tail)
        ref = psis.psis(np.logaddexp(0.0, -lc.signed_logits(W, X, y)))
        assert np.max(np.abs(ones.n_eff / ref.n_eff - 1.0)) <= 1e-10
        assert np.isnan(ones.mcse_elpd_loo) == bool(np.any(ones.khat > 0.7))
        r = np.ones(n)
        r[3], r[5], r[6] = np.nan, -0.5, 0.0                 # not a positive number: no efficiency, reported as NaN
        nan = predictive.loo(W, X, y, r_eff=r)
        assert nan.n_reff_nan == 3 and np.all(np.isnan(nan.r_eff[[3, 5, 6]]))
        assert np.all(np.isnan(nan.n_eff[[3, 5, 6]])) and np.all(np.isnan(nan.mcse_elpd_loo_i[[3, 5, 6]]))
        assert np.array_equal(nan.elpd_loo_i, ones.elpd_loo_i) and np.array_equal(np.delete(nan.n_eff, [3, 5, 6]), np.delete(ones.n_eff, [3, 5, 6]))
    assert np.array_equal(ls.tail_lengths(np.array([0.2, 1.0, np.nan, -1.0, 1e-9]), 4000),
                          predictive.tail_len_rows(np.array([0.2, 1.0, np.nan, -1.0, 1e-9]), 4000))


def test_loo_r_eff_refusals_and_the_model_method():
    import l2hmc_amd
    from l2hmc_amd import predictive
    W, X, y = ls.ar1_case(40, 5, 2, 0.5)
    flat = W.reshape(-1, 2)
    for kw in ({"r_eff": "yes"}, {"r_eff": np.ones(5)}, {"r_eff": np.ones((37, 1))}):
        with pytest.raises(ValueError):
            predictive.loo(W, X, y, **kw)
    with pytest.raises(ValueError):
        predictive.loo(flat, X, y, r_eff="auto")             # a matrix of draws has no chains
    with pytest.raises(ValueError):
        predictive.loo_tails(W, X, y, tail_len_row=np.full(37, 200))
    with pytest.raises(ValueError):
        predictive.loo_tails(W, X, y, tail_len_row=np.ones(5, dtype=np.int64))
    with pytest.raises(ValueError):
        predictive.loo_finish(predictive.loo_tails(W, X, y), r_eff=np.ones(37))      # tails without body_sq
    assert predictive.loo(flat, X, y, r_eff=np.ones(37)).n_eff.shape == (37,)        # an array needs no chains
    model = l2hmc_amd.LogisticRegression(X, y, prior_var=2.0)
    a, b = model.loo(W, r_eff="auto"), predictive.loo(W, X, y, r_eff="auto")
    assert np.array_equal(a.n_eff, b.n_eff) and np.array_equal(a.mcse_elpd_loo_i, b.mcse_elpd_loo_i)
    assert np.all(b.tail_len_row == 40)                      # the cap S // 5 binds on every row


def test_the_mc_entry_is_declared_bound_and_validates_without_gpu():
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_logistic_loo_mc_workspace_bytes", "l2hmc_logistic_loo_tails_mc"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    ws, old = L.l2hmc_logistic_loo_mc_workspace_bytes, L.l2hmc_logistic_loo_workspace_bytes
    for S, n, d in ((4000, 37, 3), (4096000, 1000, 25)):     # one more partial sum per (chunk, row)
        head = 8 + n * (256 * 8 + 8) + (n * 4 + 7) // 8 * 8
        assert (ws(S, n, d) - head) * 2 == (old(S, n, d) - head) * 3
    mc = L.l2hmc_logistic_loo_tails_mc
    for (S, n, d, stride), msg in (((1, 10, 3, 0), b"n_draws >= 2"), ((100, 0, 3, 5), b"n_data"), ((100, 10, 129, 5), b"<= d <= 128"),
                                   ((100, 10, 3, -1), b"tail_stride"), ((100, 10, 3, 100), b"tail_stride"),
                                   ((1 << 30, 1 << 20, 1, 1 << 12), b"tail too large")):
        assert mc(None, S, d, None, n, None, stride, None, None, None, None, None, None) == -1
        assert msg in L.l2hmc_last_error(), ((S, n, d, stride), L.l2hmc_last_error())
    ok = 1 << 12
    assert mc(ok, 100, 3, ok, 10, None, 20, ok, ok, ok, ok, ok, None) == -1 and b"tail_len_row is required" in L.l2hmc_last_error()
    assert mc(None, 100, 3, ok, 10, ok, 20, ok, ok, ok, ok, ok, None) == -1 and b"required" in L.l2hmc_last_error()
    assert mc(ok, 100, 3, ok, 10, ok + 4, 20, ok, ok, ok, ok, ok, None) == -1 and b"aligned" in L.l2hmc_last_error()


def test_loo_kernels_keep_their_budget_with_the_third_mode():
    """The listing of loo.s has the MODE 2 instantiations, within the 256 registers and without scratch (tests/test_loo_cpu.py
    holds every kernel of the unit to that)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("loo.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    got = {k: (vg, sc) for k, vg, sc, _ in rows}
    for g in (1, 2, 4, 8):
        vg, sc = got["loo_kernel<%d, 2>" % g]
        assert sc == 0 and vg <= 256, (g, vg, sc)


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of
    lik_stats.s uses scratch; the lag-sum kernel stays within the 512 registers of the one wave per SIMD its header states, the
    moments kernel within 256; the static LDS is the four waves' staging regions."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("lik_stats.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    want = {"%s<%d>" % (k, g) for k in ("lik_moments_kernel", "lik_lagsum_kernel") for g in (1, 2, 4, 8)} | {"chunk_reduce_kernel"}
    assert want <= names, names
    header = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "lik_stats.hip")).read()
    assert "1 wave per SIMD" in header and "tile_logits ALONE" in header
    for k, vg, sc, _ in rows:
        print("%-24s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0 and vg <= (512 if k.startswith("lik_lagsum") else 256), (k, vg, sc)
    asm = open(os.path.join(kr.ASM, "lik_stats.s")).read()
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", asm)]
    assert len(lds) >= 9 and max(lds) <= 4 * 8448, lds


@pytest.mark.parametrize("tensors", (False, True))
def test_loo_finish_of_loo_tails_is_loo_field_for_field(tensors):
    """`loo_finish(loo_tails(...))` and `loo(...)` give the same Summary, every field bit for bit, without `r_eff` and with one
    (per-row lengths that differ, one NaN efficiency), on numpy and on CPU tensors."""
    import torch
    from l2hmc_amd import predictive
    W, X, y = ls.ar1_case(40, 5, 3, 0.5)
    S, n = 200, X.shape[0]
    r = 0.2 + 1.8 * np.random.RandomState(5).rand(n)
    r[4] = np.nan
    lens = predictive.tail_len_rows(r, S)
    assert lens.min() < lens.max()
    if tensors:
        W, X, y = (torch.as_tensor(a) for a in (W, X, y))
    for kw, tail_kw in (({}, {}), ({"r_eff": r}, {"tail_len_row": lens})):
        one = predictive.loo(W, X, y, **kw)
        two = predictive.loo_finish(predictive.loo_tails(W, X, y, **tail_kw), **kw)
        assert set(one) == set(two) and ("n_eff" in one) == bool(kw)
        for k in one:
            a, b = np.asarray(one[k]), np.asarray(two[k])
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k
        assert one.n_rows == n and one.n_draws == S and np.all(np.isfinite(one.elpd_loo_i))
    assert one.n_reff_nan == 1 and np.array_equal(one.tail_len_row, lens) and np.isnan(one.n_eff[4])


def test_labels_outside_0_and_1_are_refused_on_host_input():
    """One refusal, one text, from every host route that reads the labels."""
    import torch
    from l2hmc_amd import predictive
    W, X, y = ls.ar1_case(40, 5, 2, 0.5)
    bad = y.copy()
    bad[2] = 0.5
    for conv in (np.asarray, torch.as_tensor):
        for call in (predictive.pointwise_sums, predictive.loo_tails, predictive.relative_eff):
            with pytest.raises(ValueError, match=r"^labels y must be 0 or 1$"):
                call(conv(W), conv(X), conv(bad))
