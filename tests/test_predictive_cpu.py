"""CPU: posterior predictive, lppd and WAIC of logistic regression -- `l2hmc_amd.predictive`'s numpy path and `finish` against
the scipy restatement of tests/predictive_case.py, a statistical sanity check with a known answer (p_waic ~ d), visible
underflow, the C ABI's argument validation, the compiler's listing of the new unit, and the sharded form on gloo."""
import os
import pickle
import re
import socket
import warnings

import numpy as np
import pytest

from tests import predictive_case as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_ROW = ("p_mean", "lppd_i", "p_waic_i", "elpd_i")
TOTALS = ("lppd", "p_waic", "elpd_waic", "waic", "se")


def _close(got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= tol * np.abs(ref)))


@pytest.mark.parametrize("S,n,d", [(500, 17, 3), (1000, 37, 5), (2000, 50, 128)])
def test_numpy_path_matches_the_restatement(S, n, d):
    """Every per-row array and every total agrees with the scipy restatement to 1e-12 relative; a 3-d history and its 2-d
    reshape give equal results."""
    from l2hmc_amd import predictive
    W, X, y = pc.case(S, n, d, seed=S + d)
    ref = pc.restatement(W, X, y)
    got = predictive.waic(W, X, y)
    for key in PER_ROW + TOTALS:
        assert _close(got[key], ref[key], 1e-12), (key, got[key], ref[key])
    assert got.n_draws == S and got.n_underflow == 0 and got.p_mean.shape == (n,)
    hist = predictive.waic(W.reshape(S // 4, 4, d), X, y)
    for key in PER_ROW + TOTALS:
        assert np.array_equal(hist[key], got[key]), key
    assert _close(predictive.predict_proba(W, X), ref["p_mean"], 1e-12)
    held = predictive.log_predictive_density(W, X, y)
    assert _close(held.lppd, ref["lppd"], 1e-12) and _close(held.lppd_i, ref["lppd_i"], 1e-12)
    assert _close(held.se, np.sqrt(n * ref["lppd_i"].var(ddof=1)), 1e-12)
    # the four plain sums (what ranks add up) give the same numbers through `finish` without the two-pass extras
    sums = predictive.pointwise_sums(W, X, y)
    plain = predictive.finish({k: sums[k] for k in ("sum_p", "sum_lik", "sum_ll", "sum_ll2", "n_draws")})
    for key in PER_ROW:
        assert _close(plain[key], ref[key], 1e-9), key


def test_effective_number_of_parameters_of_a_laplace_posterior():
    """Draws from the Gaussian approximation at the posterior mode of a well-identified model with n = 2000 >> d = 10:
    p_waic ~ d (a float64 run of this recipe gave 10.00), no row with a high variance, none underflowed."""
    from l2hmc_amd import predictive
    draws, X, y = pc.laplace_recipe()
    d = X.shape[1]
    s = predictive.waic(draws, X, y)
    print("p_waic %.4f for d = %d; lppd %.3f elpd_waic %.3f se %.3f" % (s.p_waic, d, s.lppd, s.elpd_waic, s.se))
    assert 0.8 * d <= s.p_waic <= 1.2 * d
    assert s.n_high_variance == 0 and s.n_underflow == 0
    assert s.elpd_waic < s.lppd < 0 and s.waic == -2 * s.elpd_waic and s.se > 0


def test_underflow_is_visible():
    """One row whose every draw gives a logit of -800 against label 1.  The float64 numpy path stays finite there (lppd_i =
    -800 by logaddexp); in the float32 convention of the device sum_lik = 0 for that row, and `finish` reports it:
    n_underflow = 1, lppd_i = -inf, without a warning or an exception."""
    from l2hmc_amd import predictive
    S = 50
    W = np.full((S, 2), 1.0, dtype=np.float32)
    X = np.array([[-400.0, -400.0], [0.5, -0.25]], dtype=np.float32)
    y = np.array([1.0, 1.0], dtype=np.float32)
    with warnings.catch_warnings(), np.errstate(all="raise"):
        warnings.simplefilter("error")
        host = predictive.waic(W, X, y)
        assert host.n_underflow == 0 and np.isfinite(host.lppd_i).all() and abs(host.lppd_i[0] + 800.0) < 1e-9
        sums = predictive.pointwise_sums(W, X, y)
        dev = {"n_draws": S, "sum_p": sums["sum_p"], "sum_ll": sums["sum_ll"], "sum_ll2": sums["sum_ll2"],
               "sum_lik": np.where(sums["sum_lik"] < 1e-38 * S, 0.0, sums["sum_lik"])}
        assert dev["sum_lik"][0] == 0.0 and dev["sum_lik"][1] > 0.0
        got = predictive.finish(dev)
    assert got.n_underflow == 1 and got.lppd_i[0] == -np.inf and np.isfinite(got.lppd_i[1])
    assert got.lppd == -np.inf and got.elpd_i[0] == -np.inf and np.isfinite(got.p_waic)


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the two new entries (ABI version still 6), and the host
    refuses bad arguments with L2HMC_ERR_ARG and a message before anything is launched."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_logistic_predict_workspace_doubles", "l2hmc_logistic_predict"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws = L.l2hmc_logistic_predict_workspace_doubles
    assert ws(4 * 10 ** 6, 1000, 25) > 0 and ws(21, 1, 1) > 0
    assert ws(4 * 10 ** 6, 1000, 25) % 4000 == 0 and ws(21, 1, 1) % 4 == 0          # whole (4, n) partials
    assert ws(21, 1 << 20, 128) > 0 and ws((1 << 40) // 128, 5, 128) > 0
    for (S, n, d), msg in (((1, 10, 3), b"n_draws >= 2"), ((0, 10, 3), b"n_draws >= 2"), ((100, 0, 3), b"n_data"),
                           ((100, (1 << 20) + 1, 3), b"n_data"), ((100, 10, 0), b"<= d <= 128"), ((100, 10, 129), b"<= d <= 128"),
                           (((1 << 40) // 25 + 1, 10, 25), b"too large"), (((1 << 40) + 1, 10, 1), b"too large")):
        assert ws(S, n, d) == -1, (S, n, d)
        assert msg in L.l2hmc_last_error(), ((S, n, d), L.l2hmc_last_error())
        assert L.l2hmc_logistic_predict(None, S, d, None, n, None, None, None) == -1
        assert msg in L.l2hmc_last_error(), ((S, n, d), L.l2hmc_last_error())
    assert L.l2hmc_logistic_predict(None, 100, 3, None, 10, None, None, None) == -1             # valid shape, NULL pointers
    assert b"required" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(L.l2hmc_logistic_predict(None, 100, 3, None, 10, None, None, None))


def test_bad_arguments_raise_value_error():
    from l2hmc_amd import predictive
    W, X, y = pc.case(40, 6, 3, seed=0)
    bad_y = y.copy()
    bad_y[2] = 0.5
    for args in ((W, X[:, :2], y),                          # feature-count mismatch
                 (W[:1], X, y),                              # S < 2
                 (W.reshape(1, 1, -1)[:, :, :3], X, y),      # a history with one draw
                 (W, X, bad_y),                              # y not in {0, 1}
                 (W, X, y[:5]),                              # y of another length
                 (W[0], X, y),                               # 1-d draws
                 (W, X[0], y)):                              # 1-d X
        with pytest.raises(ValueError):
            predictive.pointwise_sums(*args)
    with pytest.raises(ValueError):
        predictive.waic(W, X, None)
    with pytest.raises(ValueError):
        predictive.finish({"n_draws": 1, "sum_p": y, "sum_lik": y, "sum_ll": y, "sum_ll2": y})
    assert predictive.pointwise_sums(W[:2], X)["n_draws"] == 2


def test_exports_methods_and_pickling():
    import copy
    import l2hmc_amd
    from l2hmc_amd import diagnostics, predictive
    assert l2hmc_amd.waic is l2hmc_amd.predictive.waic is predictive.waic
    assert "predictive" in l2hmc_amd.__all__ and "waic" in l2hmc_amd.__all__
    W, X, y = pc.case(64, 9, 4, seed=3)
    s = predictive.waic(W, X, y)
    assert isinstance(s, diagnostics.Summary) and hasattr(s, "elpd_waic") and not hasattr(s, "nothing")
    for t in (pickle.loads(pickle.dumps(s)), copy.deepcopy(s)):
        assert isinstance(t, diagnostics.Summary) and np.array_equal(t.elpd_i, s.elpd_i) and t.waic == s.waic
    model = l2hmc_amd.LogisticRegression(X, y, prior_var=2.0)
    assert np.array_equal(model.waic(W).elpd_i, s.elpd_i)
    assert np.array_equal(model.predict_proba(W), s.p_mean)
    assert np.array_equal(model.predict_proba(W, X[:4]), predictive.predict_proba(W, X[:4]))


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of
    predictive.s uses scratch, and every geometry of the main kernel stays within the 256 registers that the two waves per
    SIMD stated in the unit's header need."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("predictive.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    want = {"predict_kernel<%d, %d>" % g for g in ((1, 4), (2, 4), (4, 2), (8, 2))} | {"chunk_reduce_kernel"}
    assert want <= names, names
    header = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "predictive.hip")).read()
    assert "2 waves per SIMD" in header
    for k, vg, sc, _ in rows:
        print("%-28s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0 and vg <= 512 // 2, (k, vg, sc)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, hist, X, y, out):
    import torch.distributed as dist
    from l2hmc_amd import sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(int(t.numel())), real(t, *a, **k))[1]
    try:
        lo, hi = (0, 23) if rank == 0 else (23, 64)                     # ragged shards
        s = sharding.predictive(hist[:, lo:hi], X, y)
        out.put((rank, s, tuple(calls)))
        dist.barrier()
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_ranks_reproduce_the_single_process_waic():
    """Chains sharded 23 + 41 over two gloo ranks: ONE all-reduce of [n_draws | 4 n sums], then `finish`, equals `waic` on
    all 64 chains to 1e-12."""
    import torch.multiprocessing as mp
    from l2hmc_amd import predictive
    n, d = 19, 4
    W, X, y = pc.case(30 * 64, n, d, seed=11, max_logit=4.0)
    hist = W.reshape(30, 64, d)
    ctx = mp.get_context("spawn")
    out = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, hist, X, y, out)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(100)
        assert pr.exitcode == 0
    res = dict((r, (s, c)) for r, s, c in (out.get() for _ in range(2)))
    ref = predictive.waic(hist, X, y)
    for rank in (0, 1):
        s, calls = res[rank]
        assert calls == (1 + 4 * n,), calls
        assert s["n_draws"] == 30 * 64 and s["n_underflow"] == 0
        for key in PER_ROW + TOTALS:
            assert _close(s[key], ref[key], 1e-12), (rank, key, s[key], ref[key])
