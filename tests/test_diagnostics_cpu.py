"""CPU: the per-coordinate convergence diagnostics (split R-hat, effective sample size) -- the estimator itself on AR(1)
chains whose answer is known, `l2hmc_amd.diagnostics`' numpy path and `finish` against the float64 restatement of
tests/diagnostics_case.py, the C ABI's argument validation, and the sharded form on gloo."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

from tests import diagnostics_case as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(dc.FIXTURES)


def test_fixtures_keep_every_pair_sum_away_from_zero():
    """The condition the GPU gates rest on: for every coordinate the reference's pair sums up to and including the stopping
    pair satisfy |P_j| >= 1e-4, so a device rounding of rho (bounded below 4e-5) cannot move a stopping index by more than the
    pair it belongs to.  (Prototype: A 5.7e-4, B 4.5e-3, C 5.1e-4, D 1.36e-4, E 8.1e-2, F 6.7e-4; truncated coordinates
    1, 1, 4, 4, 0, 3.)"""
    for name, n_trunc in zip(NAMES, (1, 1, 4, 4, 0, 3)):
        X, max_lag = dc.fixture(name)
        ref = dc.reference_summary(X, max_lag)
        smallest = min(np.abs(p).min() for p in ref["pairs"])
        print("fixture %s: smallest |P_j| %.3g, truncated %d, max rhat %.4f" % (name, smallest, ref["truncated"].sum(),
                                                                                 ref["rhat"].max()))
        assert smallest >= 1e-4, (name, smallest)
        assert int(ref["truncated"].sum()) == n_trunc, (name, ref["truncated"])


_PLAN_REF = {}


def _plan_case(name):
    """(X, max_lag, split, the column restatement's summary), computed once"""
    if name not in _PLAN_REF:
        X, max_lag, split = dc.plan_fixture(name)
        _PLAN_REF[name] = (X, max_lag, split, dc.reference_summary_columns(X, max_lag, split))
    return _PLAN_REF[name]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["F", "D"])
def test_column_restatement_equals_the_chain_by_chain_one(name, split):
    """`reference_sums_columns` is the reference of the large histories: it is itself held to the loop over chains, to 1e-12 of
    G[k, 0] (both float64, another order of the additions), and its summary to the loop's."""
    X, max_lag = dc.fixture(name)
    mean, m2, G = dc.reference_sums(X, max_lag, split)
    cmean, cm2, cG = dc.reference_sums_columns(X, max_lag, split)
    g0 = G[:, 0]
    assert cmean.shape == mean.shape and cm2.shape == m2.shape and cG.shape == G.shape
    assert np.max(np.abs(cmean - mean) / (np.abs(mean) + np.sqrt(m2))) < 1e-12
    assert np.max(np.abs(cm2 - m2) / g0) < 1e-12
    assert np.max(np.abs(cG - G) / g0[:, None]) < 1e-12
    a, b = dc.reference_summary(X, max_lag, split), dc.reference_summary_columns(X, max_lag, split)
    assert np.array_equal(a["truncated"], b["truncated"]) and (a["n_steps"], a["n_chains"]) == (b["n_steps"], b["n_chains"])
    for key in ("mean", "sd", "rhat", "ess", "tau"):
        assert np.max(np.abs(a[key] - b[key]) / (np.abs(a[key]) + (a["sd"] if key == "mean" else 0.0))) < 1e-10, key


@pytest.mark.parametrize("name", sorted(dc.PLAN_FIXTURES))
def test_plan_fixtures_keep_every_pair_sum_away_from_zero(name):
    """The condition of `test_fixtures_keep_every_pair_sum_away_from_zero` on the histories of PLAN_FIXTURES, from the
    restatement alone: |P_j| >= 1e-4 up to and including the stopping pair, so `truncated` cannot flip on a rounding of rho
    below 4e-5.  (The seeds were chosen for it: 14 and 15 left one pair of "period257-d257" / "period2-d512" at 1.6e-5 / 5e-5.)"""
    X, max_lag, split, ref = _plan_case(name)
    smallest = min(np.abs(p).min() for p in ref["pairs"])
    print("fixture %s: smallest |P_j| %.3g, truncated %d of %d, max rhat %.4f" % (name, smallest, ref["truncated"].sum(),
                                                                                  X.shape[2], ref["rhat"].max()))
    assert all(len(p) >= 1 for p in ref["pairs"])                       # no degenerate coordinate
    assert smallest >= 1e-4, (name, smallest)


# name -> (column chunks, blocks along x): what tests/diagnostics_case.py states next to PLAN_FIXTURES
PLANS = {"two-chunks-d3": (514, 513), "two-tiles-d3": (259, 258), "period15-d60": (516, 270), "period65-d130": (559, 520),
         "period257-d257": (516, 514), "period2-d512": (600, 512), "one-chunk-d300": (528, 528), "tiny-d300": (24, 24)}


def test_plan_fixtures_reach_their_branch():
    """The workspace of `l2hmc_chain_stats` is nb halves min(d, 256) (max_lag + 1) doubles, so nb, the number of blocks along x,
    is visible without a GPU: the multi-chunk fixtures have nb < ceil(N d / 256) (a block walks chunk b, b + nb, ...), with nb a
    multiple of the period d / gcd(256, d); the one-chunk ones nb = the number of chunks; and "A" .. "F" stay one chunk per
    block, which is why these fixtures exist.  A planner that moves a fixture off its branch fails here."""
    from math import gcd
    from l2hmc_amd import _ffi
    ws = _ffi.lib().l2hmc_chain_stats_workspace_doubles

    def blocks(M, N, d, max_lag, split):
        total = ws(M, N, d, max_lag, int(split))
        per = (2 if split else 1) * min(d, 256) * (max_lag + 1)
        assert total > 0 and total % per == 0
        return total // per, -(-N * d // 256)

    assert set(PLANS) == set(dc.PLAN_FIXTURES)
    for name, (M, N, d, _, max_lag, split) in dc.PLAN_FIXTURES.items():
        nb, nchunks = blocks(M, N, d, max_lag, split)
        assert (nchunks, nb) == PLANS[name], (name, nchunks, nb)
        if nb < nchunks:
            assert nb % (d // gcd(256, d)) == 0, name
    multi = {n for n, (c, b) in PLANS.items() if b < c}
    assert multi == set(PLANS) - {"one-chunk-d300", "tiny-d300"}
    assert {n for n in PLANS if dc.PLAN_FIXTURES[n][2] > 256} == {"period257-d257", "period2-d512", "one-chunk-d300", "tiny-d300"}
    for name in NAMES:
        M, N, phis, _, _, _, max_lag = dc.FIXTURES[name]
        for split in (True, False):
            nb, nchunks = blocks(M, N, len(phis), max_lag, split)
            assert nb == nchunks, (name, split)


def test_numpy_path_holds_more_than_256_coordinates():
    """"tiny-d300" on the numpy path against both restatements, as `test_numpy_path_matches_the_restatement` does."""
    from l2hmc_amd import diagnostics
    X, max_lag, split, ref = _plan_case("tiny-d300")
    slow = dc.reference_summary(X, max_lag, split)
    got = diagnostics.summarize(X, max_lag, split)
    sums = diagnostics.chain_sums(X, max_lag, split)
    for r in (ref, slow):
        mean, m2, G = r["sums"]
        assert np.max(np.abs(sums["mean"] - mean) / (np.abs(mean) + np.sqrt(m2 / (r["n_steps"] - 1)))) < 1e-10
        assert np.max(np.abs(sums["m2"] - m2) / m2) < 1e-10
        assert np.max(np.abs(sums["G"] - G) / G[:, :1]) < 1e-10
        for key in ("mean", "sd", "rhat", "ess"):
            scale = np.abs(r[key]) + (r["sd"] if key == "mean" else 0.0)
            assert np.max(np.abs(got[key] - r[key]) / scale) < 1e-10, key
        assert np.array_equal(got.truncated, r["truncated"])
    assert (got.n_steps, got.n_chains, got.max_lag) == (8, 40, 7)


def test_estimator_recovers_known_ar1_answers():
    """On the restatement alone: the ESS of an AR(1) chain is C Mh (1 - phi) / (1 + phi); chains from one distribution have
    R-hat near 1 and chains from two do not; too few lags are reported."""
    X, max_lag = dc.fixture("A")
    ref = dc.reference_summary(X, max_lag)
    C, Mh = ref["n_chains"], ref["n_steps"]
    assert (C, Mh) == (128, 500)
    for k, phi in enumerate((0.0, 0.5, 0.9)):
        ratio = ref["ess"][k] / (C * Mh * (1 - phi) / (1 + phi))
        print("phi %.2f: ess / expected %.3f, rhat %.4f" % (phi, ratio, ref["rhat"][k]))
        assert 0.8 <= ratio <= 1.2 and ref["rhat"][k] < 1.03
    Y = dc.ar1(1000, 64, [0.5, 0.5], 9)
    Y[:, :32, 1] += 1                                   # half of the chains of coordinate 1 sit one sd away
    shifted = dc.reference_summary(Y, 255)
    assert shifted["rhat"][1] > 1.1 and shifted["rhat"][0] < 1.01, shifted["rhat"]
    assert dc.reference_summary(X, 15)["truncated"][3]  # phi = .97 needs more than 16 lags


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_numpy_path_matches_the_restatement(name, split):
    """`chain_sums` (numpy) + `finish` hold the restatement to 1e-10 relative: both are float64, only the order of the sums
    differs (finish works from sum_c m and sum_c m^2, the form ranks all-reduce)."""
    from l2hmc_amd import diagnostics
    X, max_lag = dc.fixture(name)
    ref = dc.reference_summary(X, max_lag, split)
    sums = diagnostics.chain_sums(X, max_lag, split)
    mean, m2, G = ref["sums"]
    assert sums["n_steps"] == ref["n_steps"] and sums["n_chains"] == ref["n_chains"]
    assert sums["mean"].shape == mean.shape and sums["G"].shape == G.shape
    sd = np.sqrt(m2 / (ref["n_steps"] - 1))
    assert np.max(np.abs(sums["mean"] - mean) / (np.abs(mean) + sd)) < 1e-10
    assert np.max(np.abs(sums["m2"] - m2) / m2) < 1e-10
    assert np.max(np.abs(sums["G"] - G) / G[:, :1]) < 1e-10
    got = diagnostics.finish(sums)
    for key in ("mean", "sd", "rhat", "ess"):
        scale = np.abs(ref[key]) + (ref["sd"] if key == "mean" else 0.0)
        assert np.max(np.abs(got[key] - ref[key]) / scale) < 1e-10, key
    assert np.array_equal(got.truncated, ref["truncated"])
    assert got.n_steps == ref["n_steps"] and got.n_chains == ref["n_chains"] and got.max_lag == max_lag
    assert got.min_ess == got.ess.min() and got.max_rhat == got.rhat.max()
    whole = diagnostics.summarize(X, max_lag, split)
    assert np.array_equal(whole.ess, got.ess) and np.array_equal(whole.rhat, got.rhat)


def test_default_max_lag_and_odd_length():
    from l2hmc_amd import diagnostics
    X, _ = dc.fixture("B")                               # M = 257: Mh = 128, the middle row is dropped
    s = diagnostics.summarize(X)
    assert (s.n_steps, s.n_chains, s.max_lag) == (128, 400, 127)
    X, _ = dc.fixture("A")
    assert diagnostics.summarize(X).max_lag == 255 and diagnostics.summarize(X, split=False).n_steps == 1000


def test_degenerate_coordinates_are_nan_alone():
    from l2hmc_amd import diagnostics
    X, max_lag = dc.fixture("F")
    ref = dc.reference_summary(X, max_lag)
    Y = X.copy()
    Y[:, :, 3] = 2.5                                     # a constant coordinate: W = 0
    Y[40, 7, 11] = np.nan
    Y[5, 0, 12] = np.inf
    with np.errstate(all="raise"):                       # nothing warns, raises or hangs
        got = diagnostics.summarize(Y, max_lag)
    bad = np.zeros(X.shape[2], dtype=bool)
    bad[[3, 11, 12]] = True
    assert np.all(np.isnan(got.rhat[bad])) and np.all(np.isnan(got.ess[bad])) and not got.truncated[bad].any()
    assert np.max(np.abs(got.rhat[~bad] - ref["rhat"][~bad]) / ref["rhat"][~bad]) < 1e-10
    assert np.max(np.abs(got.ess[~bad] - ref["ess"][~bad]) / ref["ess"][~bad]) < 1e-10
    assert got.mean[3] == 2.5 and got.sd[3] == 0.0
    assert np.isnan(got.min_ess) and np.isnan(got.max_rhat)


def test_bad_shapes_raise_value_error():
    from l2hmc_amd import diagnostics
    X = dc.ar1(40, 6, [0.5, 0.1], 0)
    for args, kw in (((X[:7],), {}),                     # Mh = 3
                     ((X[:3],), {"split": False}),
                     ((X[:, :1],), {"split": False}),    # C = 1
                     ((X, 20), {}),                      # max_lag > Mh - 1 = 19
                     ((X, 40), {"split": False}),
                     ((X, -1), {}),
                     ((X[0],), {})):                     # not a history
        with pytest.raises(ValueError):
            diagnostics.chain_sums(*args, **kw)
    assert diagnostics.chain_sums(X, 19)["G"].shape == (2, 20)
    assert diagnostics.chain_sums(X[:, :1], 3)["n_chains"] == 2        # one chain, split: two series


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the new entries (ABI version still 6), and the host refuses
    bad arguments with L2HMC_ERR_ARG and a message before anything is launched."""
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    for name in ("l2hmc_chain_stats_workspace_doubles", "l2hmc_chain_stats"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS
    L = _ffi.lib()
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws = L.l2hmc_chain_stats_workspace_doubles
    assert ws(400, 1000, 25, 99, 1) > 0 and ws(50, 5, 1, 9, 1) == 2 * 10 and ws(8, 1, 512, 3, 1) > 0
    for args, msg in (((7, 10, 2, 2, 1), b">= 4 steps"), ((3, 10, 2, 2, 0), b">= 4 steps"), ((100, 1, 2, 5, 0), b">= 2 chains"),
                      ((100, 8, 2, 50, 1), b"max_lag"), ((100, 8, 2, -1, 1), b"max_lag"), ((100, 8, 513, 5, 1), b"d <= 512"),
                      ((100, 8, 0, 5, 1), b"must be >= 1"), ((100, 0, 2, 5, 1), b"must be >= 1"), ((100, 8, 2, 5, 2), b"split")):
        assert ws(*args) == -1, args
        assert msg in L.l2hmc_last_error(), (args, L.l2hmc_last_error())
        assert L.l2hmc_chain_stats(None, *args, None, None, None, None, None) == -1
    assert L.l2hmc_chain_stats(None, 100, 8, 2, 5, 1, None, None, None, None, None) == -1      # valid shape, NULL pointers
    assert b"required" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(L.l2hmc_chain_stats(None, 100, 8, 2, 5, 1, None, None, None, None, None))
    assert ctypes.sizeof(ctypes.c_double) == 8


def test_package_exports_the_module():
    import l2hmc_amd
    assert l2hmc_amd.diagnostics.summarize is l2hmc_amd.summarize and "diagnostics" in l2hmc_amd.__all__


def test_summary_behaves_like_an_object_and_a_dict():
    """Missing names are AttributeError (hasattr / getattr with a default work); the result pickles and deep-copies."""
    import copy
    import pickle
    from l2hmc_amd import diagnostics
    X, max_lag = dc.fixture("E")
    s = diagnostics.summarize(X, max_lag)
    assert hasattr(s, "ess") and not hasattr(s, "nothing") and getattr(s, "nothing", 7) == 7
    with pytest.raises(AttributeError):
        s.nothing
    for t in (pickle.loads(pickle.dumps(s)), copy.deepcopy(s), copy.copy(s)):
        assert isinstance(t, diagnostics.Summary) and np.array_equal(t.ess, s.ess) and t.max_rhat == s.max_rhat
        assert t["n_chains"] == s.n_chains


def test_new_kernels_use_no_scratch():
    """The diagnostics unit's requirement, from the compiler's listing (tools/kernel_resources.py; skipped when the library
    was not built here): no scratch, and the lag-sum kernel within 256 registers (two waves per SIMD by design)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("chain_stats.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    assert {"chain_moments_kernel", "chain_lagsum_kernel", "chain_lagsum_reduce_kernel"} <= names, names
    for k, vg, sc, _ in rows:
        assert sc == 0 and vg <= 256, (k, vg, sc)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, X, max_lag, out):
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
        s = sharding.diagnostics(X[:, lo:hi], max_lag=max_lag)
        out.put((rank, s, tuple(calls)))                                # the Summary itself crosses the process boundary
        dist.barrier()
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_ranks_reproduce_the_single_process_summary():
    """Chains sharded 23 + 41 over two gloo ranks: ONE all-reduce of [count | sum m | sum m^2 | sum M2 | G], then `finish`,
    equals `summarize` on all 64 chains to 1e-9.  (Split halves of a chain stay on its rank; the estimator does not care which
    series is which.)"""
    import torch.multiprocessing as mp
    from l2hmc_amd import diagnostics
    X, max_lag = dc.fixture("A")
    ctx = mp.get_context("spawn")
    out = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, X, max_lag, out)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(100)
        assert pr.exitcode == 0
    res = dict((r, (s, c)) for r, s, c in (out.get() for _ in range(2)))
    ref = diagnostics.summarize(X, max_lag)
    d = X.shape[2]
    for rank in (0, 1):
        s, calls = res[rank]
        assert calls == (1 + 3 * d + d * (max_lag + 1),), calls
        assert s["n_chains"] == 128 and s["n_steps"] == 500 and s["max_lag"] == max_lag
        for key in ("mean", "sd", "rhat", "ess"):
            scale = np.abs(ref[key]) + (ref["sd"] if key == "mean" else 0.0)
            assert np.max(np.abs(s[key] - ref[key]) / scale) < 1e-9, (rank, key)
        assert np.array_equal(s["truncated"], ref.truncated)
        assert abs(s["min_ess"] - ref.min_ess) < 1e-9 * ref.min_ess and abs(s["max_rhat"] - ref.max_rhat) < 1e-9
