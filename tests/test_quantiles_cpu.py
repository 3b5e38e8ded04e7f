"""CPU: `l2hmc_amd.quantiles` -- the numpy path of `order_statistics` / `quantiles` / `describe` against the restatement of
tests/quantiles_case.py, the C ABI's new entries and their argument validation without a GPU, the compiler's listing of the
order-statistics unit, and the sharded form on gloo."""
import os
import re
import socket

import numpy as np
import pytest

from tests import diagnostics_case as dc
from tests import quantiles_case as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("l2hmc_order_stats_passes", "l2hmc_order_stats_bins", "l2hmc_order_stats_workspace_bytes", "l2hmc_order_stats",
               "l2hmc_order_stats_count", "l2hmc_order_stats_advance", "l2hmc_chain_stats_below")


def _history(name):
    return qc.adversarial() if name == "adversarial" else dc.fixture(name)


@pytest.mark.parametrize("name", ["A", "B", "D", "E", "F", "adversarial"])
def test_order_statistics_and_quantiles_match_the_restatement(name):
    """Order statistics are exact; quantiles are within 1e-15 relative of np.quantile where that is finite."""
    from l2hmc_amd import quantiles
    X, _ = _history(name)
    S, d = X.shape[0] * X.shape[1], X.shape[2]
    for ranks in (qc.standard_ranks(S), qc.rank_table(S, d, seed=1, R=40)):      # 40 ranks: more than one chunk of 32
        want, want_nan = qc.reference_order_statistics(X, ranks)
        for history in (X, qc.draws(X)):                                     # (steps, chains, d) and (S, d)
            got, got_nan = quantiles.order_statistics(history, ranks)
            assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True) and np.array_equal(got_nan, want_nan)
    probs = (0.0, 0.05, 0.25, 0.333, 0.5, 0.95, 1.0)
    got, want = quantiles.quantiles(X, probs), qc.reference_quantiles(X, probs)
    assert got.dtype == np.float64 and got.shape == (len(probs), d)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-15 * np.abs(want[fin]))
    if name == "adversarial":
        assert np.all(np.isnan(got[:, qc.NAN_COORDINATE])) and np.isnan(got).sum() == len(probs)      # NaN alone
        assert got[0, 4] == -np.inf and got[-1, 4] == np.inf and np.all(np.isfinite(got[1:-1, 4]))    # +-inf are values
        assert np.all(got[:, 1] == 2.5)


def test_order_statistics_of_the_plan_fixtures_on_numpy():
    """"copies-d3" (300 x 100 x 3) with its 20-row rank table, and the hostile coordinates of "long-walk-d70" at the standard
    ranks: the numpy path equals the sort, so the fixtures the device tests rest on are what they are said to be."""
    from l2hmc_amd import quantiles
    X = qc.plan_history("copies-d3")
    S, d = 300 * 100, 3
    assert X.shape == (300, 100, 3) and X.dtype == np.float32
    for ranks in (qc.standard_ranks(S), qc.rank_table(S, d, seed=1, R=20)):
        want, want_nan = qc.reference_order_statistics(X, ranks)
        got, got_nan = quantiles.order_statistics(X, ranks)
        assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got_nan, want_nan) and not got_nan.any()
    probs = (0.05, 0.5, 0.95)
    got, want = quantiles.quantiles(X, probs), qc.reference_quantiles(X, probs)
    assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want))
    Y = qc.plan_history("long-walk-d70")
    S = 140 * 1000
    want, want_nan = qc.reference_order_statistics(Y, qc.standard_ranks(S))
    got, got_nan = quantiles.order_statistics(Y, qc.standard_ranks(S))
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got_nan, want_nan)
    assert want_nan[qc.LONG_WALK_NAN_COORDINATE] == 1 and want_nan.sum() == 1 and np.isnan(want[-1, qc.LONG_WALK_NAN_COORDINATE])
    assert want[0, 4] == -np.inf and want[-1, 4] == want[-2, 4] == np.inf and np.all(want[:, 1] == 2.5)
    assert np.all(want[:, 3] == 0) and np.signbit(Y[:, :, 3]).any() and not np.signbit(Y[:, :, 3]).all()      # a +-0 mix
    assert len(np.unique(Y[:, :, 2])) < 64 and np.all(np.abs(Y[:, :, 7]) < 2.0 ** -126)               # ties; denormals


def test_numpy_radix_select_equals_the_sort():
    """The select the sharded path runs on numpy shards (8-bit digits, four passes, the histograms added between count and
    advance) agrees with np.sort at every rank of the adversarial history, ranks past the end included."""
    from l2hmc_amd import quantiles
    X, _ = qc.adversarial()
    X2 = qc.draws(X)
    S, d = X2.shape
    ranks = qc.rank_table(S, d, seed=4, R=40)
    want, want_nan = qc.reference_order_statistics(X, ranks)
    got, got_nan = quantiles._sharded_select(X2, ranks, lambda t: t)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got_nan, want_nan)
    assert quantiles.HOST_BITS * quantiles.HOST_PASSES == 32


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["A", "E", "F"])
def test_describe_matches_the_restatement(name, split):
    from l2hmc_amd import diagnostics, quantiles
    X, lag = dc.fixture(name)
    ref = qc.reference_describe(X, lag, split)
    got = quantiles.describe(X, qc.PROBS, lag, split)
    assert isinstance(got, diagnostics.Summary)
    assert np.all(np.abs(got.quantiles - ref["quantiles"]) <= 1e-15 * np.abs(ref["quantiles"]))
    assert np.array_equal(got.probs, qc.PROBS) and got.n_nan.sum() == 0
    for key in ("ess_quantile", "ess_tail", "mcse_mean", "mcse_quantile"):
        assert got[key].shape == ref[key].shape, key
        assert np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key])) < 1e-10, key
    assert np.array_equal(got.truncated_quantile, ref["truncated_quantile"])
    base = diagnostics.summarize(X, lag, split)                               # summarize's entries, unchanged
    for key in base:
        assert np.array_equal(got[key], base[key], equal_nan=True), key


def test_tail_probabilities_are_added_when_missing_and_degenerate_coordinates_are_nan_alone():
    from l2hmc_amd import quantiles
    X, lag = qc.adversarial()
    got = quantiles.describe(X, (0.5,), lag)
    assert got.quantiles.shape == (1, 17) == got.ess_quantile.shape == got.mcse_quantile.shape and got.ess_tail.shape == (17,)
    full = quantiles.describe(X, qc.PROBS, lag)
    assert np.array_equal(got.ess_tail, full.ess_tail, equal_nan=True)
    assert np.array_equal(got.quantiles[0], full.quantiles[1], equal_nan=True)
    assert np.array_equal(full.ess_tail, np.minimum(full.ess_quantile[0], full.ess_quantile[2]), equal_nan=True)
    bad = np.zeros(17, dtype=bool)
    bad[[1, qc.NAN_COORDINATE]] = True                                        # the constant (its indicator never varies), the NaN
    assert np.all(np.isnan(full.ess_quantile[:, bad])) and np.all(np.isnan(full.mcse_quantile[:, bad]))
    assert np.all(np.isnan(full.ess_tail[bad])) and full.n_nan[qc.NAN_COORDINATE] == 1 and full.n_nan.sum() == 1
    clean = [0, 12, 13, 14, 15, 16]
    assert np.all(full.ess_quantile[:, clean] > 0) and np.all(full.mcse_quantile[:, clean] > 0)
    assert np.all(full.ess_quantile[:, 4] > 0) and np.all(np.isfinite(full.mcse_quantile[:, 4]))     # +-inf: ordinary values


def test_bad_shapes_and_probabilities_raise_value_error():
    from l2hmc_amd import quantiles
    X = dc.ar1(40, 6, [0.5, 0.1], 0)
    for probs in ((-0.1,), (1.5,), (0.5, float("nan")), (), ((0.1, 0.2),)):
        with pytest.raises(ValueError):
            quantiles.quantiles(X, probs)
        with pytest.raises(ValueError):
            quantiles.describe(X, probs)
    for bad in (X[0, 0], X[None], X[:0]):
        with pytest.raises(ValueError):
            quantiles.quantiles(bad, (0.5,))
    with pytest.raises(ValueError):
        quantiles.describe(X[0], (0.5,))                                      # (S, d) is not a history of chains
    with pytest.raises(ValueError):
        quantiles.describe(X[:7])                                             # the shapes `summarize` refuses
    for ranks in ([240], [-1], [0.5], np.zeros((2, 3), dtype=np.int64), np.zeros((0,), dtype=np.int64)):
        with pytest.raises(ValueError):
            quantiles.order_statistics(X, ranks)
    assert quantiles.order_statistics(X, [239])[0].shape == (1, 2)


def test_package_exports_the_module():
    import l2hmc_amd
    assert l2hmc_amd.quantiles.describe is l2hmc_amd.describe
    assert "quantiles" in l2hmc_amd.__all__ and "describe" in l2hmc_amd.__all__


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the new entries (ABI version still 6); the host refuses bad
    arguments with L2HMC_ERR_ARG and a message that names the entry and the limit, before anything is launched."""
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS, name
    L = _ffi.lib()
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    passes, bins = L.l2hmc_order_stats_passes(), L.l2hmc_order_stats_bins()
    assert passes >= 1 and bins >= 2 and bins & (bins - 1) == 0
    assert passes * (bins.bit_length() - 1) >= 32
    ws = L.l2hmc_order_stats_workspace_bytes
    assert ws(25, 6) >= 25 * 6 * (bins * 8 + 8 + 4) and ws(1, 1) > 0 and ws(512, 32) > 0
    for args, msg in (((513, 4), b"d <= 512"), ((0, 4), b"must be >= 1"), ((25, 0), b"1 <= n_ranks <= 32"),
                      ((25, 33), b"1 <= n_ranks <= 32")):
        assert ws(*args) == -1, args
        assert msg in L.l2hmc_last_error() and b"l2hmc_order_stats_workspace_bytes" in L.l2hmc_last_error(), L.l2hmc_last_error()
    one = 0x1000                                                              # a non-NULL pointer nothing dereferences: refused first
    for (S, d, R), msg in (((100, 513, 4), b"d <= 512"), ((100, 25, 0), b"n_ranks"), ((100, 25, 33), b"n_ranks"),
                           ((0, 25, 4), b"must be >= 1"), ((1 << 40, 25, 4), b"too large")):
        assert L.l2hmc_order_stats(one, S, d, one, R, one, one, one, None) == -1
        assert msg in L.l2hmc_last_error() and b"l2hmc_order_stats:" in L.l2hmc_last_error(), L.l2hmc_last_error()
        assert L.l2hmc_order_stats_count(one, S, d, R, 0, one, one, one, None) == -1
        assert msg in L.l2hmc_last_error() and b"l2hmc_order_stats_count:" in L.l2hmc_last_error()
    for p in (-1, passes):
        assert L.l2hmc_order_stats_count(one, 100, 25, 4, p, one, one, one, None) == -1
        assert b"pass" in L.l2hmc_last_error()
        assert L.l2hmc_order_stats_advance(one, one, one, 25, 4, p, one, None) == -1
        assert b"pass" in L.l2hmc_last_error() and b"l2hmc_order_stats_advance:" in L.l2hmc_last_error()
    assert L.l2hmc_order_stats_advance(one, one, one, 513, 4, 0, None, None) == -1 and b"d <= 512" in L.l2hmc_last_error()
    for call in (lambda: L.l2hmc_order_stats(None, 100, 25, None, 4, None, None, None, None),
                 lambda: L.l2hmc_order_stats(one, 100, 25, one, 4, one, one, None, None),
                 lambda: L.l2hmc_order_stats_count(None, 100, 25, 4, 0, None, None, None, None),
                 lambda: L.l2hmc_order_stats_count(one, 100, 25, 4, 1, None, one, None, None),      # prefix, pass > 0
                 lambda: L.l2hmc_order_stats_count(one, 100, 25, 4, 0, None, one, None, None),      # n_nan, pass 0
                 lambda: L.l2hmc_order_stats_advance(None, None, None, 25, 4, 0, None, None),
                 lambda: L.l2hmc_order_stats_advance(one, one, one, 25, 4, passes - 1, None, None),   # values, last pass
                 lambda: L.l2hmc_chain_stats_below(None, 100, 8, 2, 5, 1, None, None, None, None, None, None),
                 lambda: L.l2hmc_chain_stats_below(one, 100, 8, 2, 5, 1, None, one, one, one, one, None)):
        assert call() == -1
        assert b"required" in L.l2hmc_last_error(), L.l2hmc_last_error()
    for args, msg in (((7, 10, 2, 2, 1), b">= 4 steps"), ((100, 8, 513, 5, 1), b"d <= 512"), ((100, 8, 2, 50, 1), b"max_lag")):
        assert L.l2hmc_chain_stats_below(one, *args, one, one, one, one, one, None) == -1
        assert msg in L.l2hmc_last_error() and b"l2hmc_chain_stats_below" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(L.l2hmc_order_stats(None, 100, 25, None, 4, None, None, None, None))


def test_order_statistics_kernels_use_no_scratch():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of the
    order-statistics unit spills -- the per-thread prefixes are registers with compile-time indices -- and the indicator
    kernels of the chain-sums unit exist under their own names."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    res = kr.resources()
    rows = res.get("order_stats.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    assert "radix_advance_kernel" in names and any(k.startswith("order_count_kernel<") for k in names), names
    for k, vg, sc, _ in rows:
        assert sc == 0 and vg <= 256, (k, vg, sc)
    assert {"chain_moments_below_kernel", "chain_lagsum_below_kernel"} <= {k for k, _, _, _ in res["chain_stats.s"]}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, X, max_lag, out):
    import torch.distributed as dist
    from l2hmc_amd import quantiles, sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls, selects = [], []
    real, real_select = dist.all_reduce, quantiles._select
    dist.all_reduce = lambda t, *a, **k: (calls.append(int(t.numel())), real(t, *a, **k))[1]

    def counted_select(*a, **k):
        before = len(calls)
        res = real_select(*a, **k)
        selects.append(len(calls) - before)
        return res
    quantiles._select = counted_select
    try:
        lo, hi = (0, 23) if rank == 0 else (23, 64)                     # ragged shards
        s = sharding.describe(X[:, lo:hi], qc.PROBS, max_lag=max_lag)
        out.put((rank, s, tuple(calls), tuple(selects)))
        dist.barrier()
    finally:
        dist.all_reduce, quantiles._select = real, real_select
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_ranks_reproduce_the_single_process_description():
    """Chains sharded 23 + 41 over two gloo ranks: the quantiles (and the MCSE, a difference of order statistics at positions
    derived from the reduced ess) equal `describe` on all 64 chains bit for bit when the ess agree; `ess_*` to 1e-10; every
    `order_statistics` call costs at most passes all-reduces, and the whole description one more for [S_local]."""
    import torch.multiprocessing as mp
    from l2hmc_amd import quantiles
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
    res = dict((r, (s, c, n)) for r, s, c, n in (out.get() for _ in range(2)))
    ref = quantiles.describe(X, qc.PROBS, max_lag)
    d, passes = X.shape[2], quantiles.HOST_PASSES
    for rank in (0, 1):
        s, calls, selects = res[rank]
        assert len(selects) == 2 and all(n <= passes for n in selects), selects      # + the one of [S_local]: passes + 1
        assert calls.count(1) == 1                                                   # [S_local], once
        chain_sums = [c for c in calls if c == 1 + 3 * d + d * (max_lag + 1)]
        assert len(chain_sums) == 1 + len(qc.PROBS) and len(calls) == 1 + sum(selects) + len(chain_sums), calls
        assert np.array_equal(s["quantiles"].view(np.int64), ref.quantiles.view(np.int64))
        assert np.array_equal(s["n_nan"], ref.n_nan) and np.array_equal(s["truncated_quantile"], ref.truncated_quantile)
        for key in ("ess_quantile", "ess_tail", "ess", "mcse_mean"):
            assert np.max(np.abs(s[key] - ref[key]) / np.abs(ref[key])) < 1e-10, (rank, key)
        assert s["n_chains"] == 128 and s["n_steps"] == 500 and s["max_lag"] == max_lag
    assert np.array_equal(res[0][0]["mcse_quantile"], res[1][0]["mcse_quantile"])    # every rank ends with the same table
