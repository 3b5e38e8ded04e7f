"""CPU: PSIS-LOO of logistic regression -- `l2hmc_amd.predictive.loo`'s numpy route against the direct restatement of
tests/loo_case.py, the fixtures' own preconditions, three degenerate histories, the `Summary` algebra, refusals, the C ABI's
argument validation and the compiler's listing of the new unit."""
import os
import re

import numpy as np
import pytest

from tests import loo_case as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _ref(S, n, d):
    if (S, n, d) not in _REF:
        W, X, y = lc.case(S, n, d)
        _REF[(S, n, d)] = (W, X, y, lc.restatement(W, X, y))
    return _REF[(S, n, d)]


def _agree(got, ref):
    fin = np.isfinite(ref["khat"])
    assert np.array_equal(fin, np.isfinite(got.khat)) and np.all(got.khat[~fin] == np.inf)
    dk = float(np.max(np.abs(got.khat[fin] - ref["khat"][fin]))) if fin.any() else 0.0
    de = float(np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])))
    print("numpy route - restatement: khat %.2g elpd_loo_i %.2g" % (dk, de))
    assert dk <= 1e-10 and de <= 1e-10
    assert np.array_equal(got.n_tail, ref["n_tail"]) and got.n_tail.dtype == np.int64
    assert np.max(np.abs(got.lppd_i - ref["lppd_i"])) <= 1e-10


@pytest.mark.parametrize("S,n,d", lc.FIXTURES)
def test_numpy_route_matches_the_direct_restatement(S, n, d):
    """elpd_loo_i and khat within 1e-10 (about 1e-14 measured: another summation order), n_tail equal; a 3-d history and its 2-d
    view give equal results; loo = loo_finish(loo_tails)."""
    from l2hmc_amd import predictive
    W, X, y, ref = _ref(S, n, d)
    got = predictive.loo(W, X, y)
    _agree(got, ref)
    assert got.tail_len == lc.tail_len(S) == predictive.loo_tail_len(S) and got.n_draws == S and got.n_rows == n
    assert got.khat_threshold == lc.khat_threshold(S) and got.n_underflow == 0
    if S % 4 == 0:
        hist = predictive.loo(W.reshape(S // 4, 4, d), X, y)
        assert np.array_equal(hist.elpd_loo_i, got.elpd_loo_i) and np.array_equal(hist.khat, got.khat)
    two = predictive.loo_finish(predictive.loo_tails(W, X, y))
    assert np.array_equal(two.elpd_loo_i, got.elpd_loo_i) and np.array_equal(two.khat, got.khat, equal_nan=True)
    if S <= 523:                                             # the host chunking (one draw at a time) changes no decision
        old, predictive._HOST_CHUNK_ELEMS = predictive._HOST_CHUNK_ELEMS, 7 * n
        try:
            _agree(predictive.loo(W, X, y), ref)
        finally:
            predictive._HOST_CHUNK_ELEMS = old


def test_fixtures_have_good_and_bad_rows_away_from_the_gates():
    """From the restatement alone: the larger fixtures each have a row with khat > 0.7 and one with khat < 0.5,
    and no reference khat lies within its gate K_KHAT delta_i of 0.7 or of khat_threshold."""
    for S, n, d in lc.FIXTURES:
        W, X, y, ref = _ref(S, n, d)
        fin = np.isfinite(ref["khat"])
        if not fin.any():
            assert lc.tail_len(S) < 5
            continue
        di, _ = lc.delta(W, X)
        k = ref["khat"]
        gap = np.minimum(np.abs(k - lc.KHAT_BAD), np.abs(k - lc.khat_threshold(S)))
        print((S, n, d), "khat %.3f .. %.3f, nearest gate / (K delta) %.3g" % (k[fin].min(), k[fin].max(), np.min((gap / (lc.K_KHAT * di))[fin])))
        assert np.all(gap[fin] > lc.K_KHAT * di[fin])
    from l2hmc_amd import predictive
    for shape in ((37, 17, 3), (523, 33, 17), (300, 50, 128), (4099, 100, 25)):
        W, X, y, ref = _ref(*shape)
        k = ref["khat"]
        assert k.max() > 0.7 and k.min() < 0.5, shape
        got = predictive.loo(W, X, y)                        # ... and the library counts the same rows on either side
        assert got.n_bad == int(np.sum(k > 0.7)) and got.n_above_threshold == int(np.sum(k > lc.khat_threshold(shape[0])))


def test_degenerate_histories():
    """Every draw twice: L = M on every row.  Half the draws one repeated vector: the tie at the cutoff shortens the tail of
    at least one row below M, as in the restatement.  All draws identical: L = 0, khat = +inf and elpd_loo_i = ll."""
    from l2hmc_amd import predictive
    W, X, y = lc.case(300, 50, 128)
    twice = lc.degenerate("twice", W)
    got = predictive.loo(twice, X, y)
    _agree(got, lc.restatement(twice, X, y))
    assert np.all(got.n_tail == lc.tail_len(600))
    half = lc.degenerate("half", W)
    got = predictive.loo(half, X, y)
    _agree(got, lc.restatement(half, X, y))
    assert np.any(got.n_tail < lc.tail_len(300)) and np.any(got.n_tail == lc.tail_len(300))
    const = lc.degenerate("constant", W)
    got = predictive.loo(const, X, y)
    ll = -np.logaddexp(0.0, -lc.signed_logits(const[:1], X, y)[0])
    assert np.all(got.n_tail == 0) and np.all(got.khat == np.inf) and got.n_bad == 50
    assert np.max(np.abs(got.elpd_loo_i - ll)) <= 1e-12 and np.max(np.abs(got.p_loo_i)) <= 1e-12


def test_summary_algebra():
    from l2hmc_amd import diagnostics, predictive
    W, X, y, ref = _ref(523, 33, 17)
    s = predictive.loo(W, X, y)
    assert isinstance(s, diagnostics.Summary)
    assert s.elpd_loo == float(s.elpd_loo_i.sum()) and s.p_loo == float(s.p_loo_i.sum()) and s.lppd == float(s.lppd_i.sum())
    assert s.looic == -2.0 * s.elpd_loo and np.array_equal(s.p_loo_i, s.lppd_i - s.elpd_loo_i)
    assert abs(s.se - np.sqrt(33 * s.elpd_loo_i.var(ddof=1))) <= 1e-12 * s.se
    assert s.n_bad == int(np.sum(ref["khat"] > 0.7)) >= 1
    assert s.n_above_threshold == int(np.sum(ref["khat"] > lc.khat_threshold(523))) >= s.n_bad
    assert np.all(s.p_loo_i > 0) and s.elpd_loo < s.lppd
    w = predictive.waic(W, X, y)
    assert abs(s.lppd - w.lppd) <= 1e-9 * abs(w.lppd)
    one = predictive.loo(W, X[:1], y[:1])
    assert np.isnan(one.se) and one.n_rows == 1 and np.isfinite(one.elpd_loo)
    # a NaN draw makes every row NaN, quietly
    bad = W.copy()
    bad[5, 0] = np.nan
    nan = predictive.loo(bad, X, y)
    assert np.all(np.isnan(nan.elpd_loo_i)) and np.isnan(nan.elpd_loo)


def test_exports_and_the_model_method():
    import l2hmc_amd
    from l2hmc_amd import predictive
    assert l2hmc_amd.loo is predictive.loo and "loo" in l2hmc_amd.__all__
    W, X, y, _ = _ref(37, 17, 3)
    model = l2hmc_amd.LogisticRegression(X, y, prior_var=2.0)
    a, b = model.loo(W), predictive.loo(W, X, y)
    assert np.array_equal(a.elpd_loo_i, b.elpd_loo_i) and np.array_equal(a.khat, b.khat)


def test_bad_arguments_raise_value_error():
    from l2hmc_amd import predictive
    W, X, y = lc.case(40, 6, 3)
    bad_y = y.copy()
    bad_y[2] = 0.5
    for args in ((W, X[:, :2], y), (W[:1], X, y), (W, X, bad_y), (W, X, y[:5]), (W[0], X, y), (W, X[0], y), (W, X, None)):
        for fn in (predictive.loo, predictive.loo_tails):
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        predictive.loo_finish(dict(predictive.loo_tails(W, X, y), n_draws=1))
    assert predictive.loo(W[:2], X, y).tail_len == 0


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the three entries (ABI version still 6); every L2HMC_ERR_ARG
    case is refused with a message before anything is launched."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_logistic_loo_tail_len", "l2hmc_logistic_loo_workspace_bytes", "l2hmc_logistic_loo_tails"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    for S in (2, 4, 5, 24, 25, 37, 100, 523, 4099, 4096000, 10 ** 9, (1 << 40) - 1):
        assert L.l2hmc_logistic_loo_tail_len(S) == lc.tail_len(S), S
    assert L.l2hmc_logistic_loo_tail_len(4096000) == 6072
    ws = L.l2hmc_logistic_loo_workspace_bytes
    assert ws(4096000, 1000, 25) > 0 and ws(4096000, 1000, 25) % 8 == 0 and ws(25, 1, 1) > 0
    # the draw chunks depend on n_draws alone: the partial sums grow in proportion to the rows
    assert ws(4099, 64, 25) - ws(4099, 32, 25) == ws(4099, 96, 25) - ws(4099, 64, 25)
    tails = L.l2hmc_logistic_loo_tails
    for (S, n, d), msg in (((1, 10, 3), b"n_draws >= 2"), ((0, 10, 3), b"n_draws >= 2"), ((100, 0, 3), b"n_data"),
                           ((100, (1 << 20) + 1, 3), b"n_data"), ((100, 10, 0), b"<= d <= 128"), ((100, 10, 129), b"<= d <= 128"),
                           (((1 << 40) // 25 + 1, 10, 25), b"too large"), (((1 << 40) + 1, 10, 1), b"too large"),
                           ((4096000, 1 << 20, 25), b"tail too large")):
        assert ws(S, n, d) == -1, (S, n, d)
        assert msg in L.l2hmc_last_error(), ((S, n, d), L.l2hmc_last_error())
        assert tails(None, S, d, None, n, None, None, None, None, None, None) == -1
        assert msg in L.l2hmc_last_error(), ((S, n, d), L.l2hmc_last_error())
    assert tails(None, 100, 3, None, 10, None, None, None, None, None, None) == -1                 # valid shape, NULL pointers
    assert b"required" in L.l2hmc_last_error()
    ok = 1 << 12                                             # an aligned non-NULL address: refused before it is touched
    for at in range(6):
        args = [ok, 100, 3, ok, 10, ok, ok, ok, ok, ok, None]
        args[(0, 3, 5, 6, 8, 9)[at]] = ok + (2 if at in (0, 2) else 4)
        assert tails(*args) == -1 and b"aligned" in L.l2hmc_last_error(), at
    args = [ok, 100, 3, ok, 10, ok, ok, ok + 2, ok, ok, None]
    assert tails(*args) == -1 and b"aligned" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(tails(None, 100, 3, None, 10, None, None, None, None, None, None))


def test_gpu_shapes_sit_in_their_chunk_branch():
    """The planner cuts the draws into chunks of tpc = max(4, ceil(tiles / 1024)) tiles.  The workspace is
    8 + n (256 x 8 + 8) + n x 4 rounded up to 8 + chunks x 2 n x 8 bytes, so its size tells the chunks: the small GPU shapes sit on
    the floor tpc = 4, the two large ones of tests/test_gpu_loo.py and the headline shape beyond it."""
    from l2hmc_amd import _ffi
    ws = _ffi.lib().l2hmc_logistic_loo_workspace_bytes

    def chunks(S, n, d):
        rest = ws(S, n, d) - 8 - n * (256 * 8 + 8) - (n * 4 + 7) // 8 * 8
        assert rest > 0 and rest % (16 * n) == 0
        return rest // (16 * n)
    for (S, n, d), tpc in (((70, 35, 5), 4), ((70, 35, 72), 4), ((523, 33, 17), 4), ((300, 50, 128), 4), ((4099, 100, 25), 4),
                           ((65536, 33, 1), 4), ((65537, 33, 1), 5), ((65609, 33, 1), 5), ((65609, 37, 19), 5), ((70000, 35, 17), 5),
                           ((65609, 33, 40), 5), ((65609, 33, 72), 5), ((4096000, 1000, 25), 250)):
        tiles = (S + 15) // 16
        assert chunks(S, n, d) == -(-tiles // tpc), (S, n, d)
        assert tpc == max(4, -(-tiles // 1024))
    assert chunks(65609, 33, 1) == 821 and chunks(65609, 33, 1) % 4 == 1 and chunks(70000, 35, 17) == 875
    assert chunks(65609, 33, 40) == 821 and chunks(65609, 33, 72) == 821     # NT 3 / NTM 4 and NT 5 / NTM 8 beyond the floor
    assert chunks(70000, 12, 17) == chunks(70000, 35, 17)            # the chunks do not depend on the rows of a call


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of
    loo.s uses scratch, every geometry of the main kernel stays within the 256 registers that the two waves per SIMD stated in
    the unit's header need, and its static LDS lets two workgroups share a CU's 160 KiB."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("loo.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    want = {"loo_kernel<%d, %d>" % (g, m) for g in (1, 2, 4, 8) for m in (0, 1)}
    want |= {"radix_advance_kernel", "loo_init_kernel", "chunk_reduce_kernel"}
    assert want <= names, names
    header = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "loo.hip")).read()
    assert "2 waves per SIMD" in header and "ONE device function" in header
    for k, vg, sc, _ in rows:
        print("%-24s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0 and vg <= 512 // 2, (k, vg, sc)
    asm = open(os.path.join(kr.ASM, "loo.s")).read()
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", asm)]
    assert len(lds) >= 11 and max(lds) <= 80 * 1024, lds
