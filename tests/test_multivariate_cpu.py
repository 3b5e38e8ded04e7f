"""CPU: `l2hmc_amd.multivariate` -- the numpy path of `covariance` / `multi_ess` against the two-pass restatement of
tests/multivariate_case.py, the C ABI's new entries and their argument validation without a GPU, the compiler's listing of
the moment-sums unit, and the sharded form on gloo."""
import os
import re
import socket

import numpy as np
import pytest

from tests import diagnostics_case as dc
from tests import multivariate_case as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("l2hmc_moment_sums_workspace_doubles", "l2hmc_moment_sums")


@pytest.mark.parametrize("name", ["A", "B", "C", "E", "F", "G"])
def test_numpy_path_matches_the_restatement(name):
    """Matrices to 1e-12 of sqrt(P_ii P_jj), multi_ess to 1e-10."""
    from l2hmc_amd import diagnostics, multivariate
    X = mc.history(name)
    b = mc.default_batch(X.shape[0])
    ref = mc.reference(X, b)
    got = multivariate.multi_ess(X)
    assert isinstance(got, diagnostics.Summary)
    n, d = ref["n_draws"], X.shape[2]
    scale = np.sqrt(np.outer(np.diag(ref["P"]), np.diag(ref["P"])))
    assert got.n_draws == n and got.batch_size == b and got.n_batches == ref["n_batches"] and not got.degenerate.any()
    assert np.max(np.abs(got.cov * (n - 1) - ref["P"]) / scale) < 1e-12
    qscale = np.sqrt(np.outer(np.diag(ref["Q"]), np.diag(ref["Q"])))
    assert np.max(np.abs(got.cov_asymptotic * (ref["n_batches"] - 1) / b - ref["Q"]) / qscale) < 1e-12
    assert np.max(np.abs(got.mean - ref["mean"]) / ref["sd"]) < 1e-12
    assert np.max(np.abs(got.corr - ref["corr"])) < 1e-12 and np.all(np.diag(got.corr) == 1.0)
    assert np.max(np.abs(got.sd - ref["sd"]) / ref["sd"]) < 1e-12
    assert np.max(np.abs(got.ess_batch - ref["ess_batch"]) / ref["ess_batch"]) < 1e-10
    assert abs(got.multi_ess - ref["multi_ess"]) / ref["multi_ess"] < 1e-10
    assert got.cov.shape == (d, d) == got.cov_asymptotic.shape and np.array_equal(got.cov, got.cov.T)
    cov = multivariate.covariance(X)
    for key in ("mean", "cov", "corr", "sd", "degenerate"):
        assert np.array_equal(cov[key], got[key]), key
    assert "multi_ess" not in cov and cov.n_draws == n
    flat = multivariate.covariance(X.reshape(-1, d))                           # (S, d)
    assert np.max(np.abs(flat.cov * (n - 1) - ref["P"]) / scale) < 1e-12


# name -> (chunks of 16 chains, blocks along x, step segments): what tests/multivariate_case.py states next to PLAN_FIXTURES
PLANS = {"two-chunks-d17": (258, 256, 1), "two-chunks-d70": (257, 256, 1)}
PLANS.update({"panel-d%d" % d: (3, 3, 6) for d in (40, 64, 65, 96, 113, 128)})


def test_plan_fixtures_reach_their_branch():
    """The workspace of `l2hmc_moment_sums` is stride nbx nseg npanel doubles with, as csrc/moment_sums.hip's header says,
    stride = (P 256 + 4 x 64) doubles per accumulator set (two sets with batches), P the pairs of the largest panel, so the
    number of blocks per panel is visible without a GPU.  The two-chunk fixtures have nbx = 256 < ceil(chains / 16): block 0
    (and 1) walks a second chunk; the panel fixtures 3 chunks in 3 blocks x 6 segments; and the older fixtures never more blocks
    than chunks along x.  Both with batches and without."""
    from l2hmc_amd import _ffi
    ws = _ffi.lib().l2hmc_moment_sums_workspace_doubles

    def blocks(steps, chains, d, batch):
        T = -(-d // 16)
        pairs, npanel = (T * (T + 1) // 2, 1) if T <= 4 else (max(10, 4 * (T - 4)), 3)
        per = (pairs * 256 + 4 * 64) * (2 if batch else 1) * npanel
        total = ws(steps, chains, d, batch)
        assert total > 0 and total % per == 0
        return total // per

    assert set(PLANS) == set(mc.PLAN_FIXTURES)
    for name, (steps, chains, d, batch, _) in mc.PLAN_FIXTURES.items():
        nchunks, nbx, nseg = PLANS[name]
        assert nchunks == -(-chains // 16)
        assert blocks(steps, chains, d, batch) == nbx * nseg, name
        if nbx < nchunks:
            assert nbx == 256 and blocks(steps, chains, d, 0) == 256, name              # batch 0: the same walk
        else:
            assert blocks(steps, chains, d, 0) == nbx * min(-(-256 // nbx), steps), name  # segments of single rows
    rem = {name: steps % batch for name, (steps, _, _, batch, _) in mc.PLAN_FIXTURES.items()}     # leading rows in no batch
    assert rem["two-chunks-d17"] == 1 and rem["two-chunks-d70"] == 0 and rem["panel-d65"] == 4
    for name in ("A", "B", "C", "E", "F", "G"):
        steps, chains, d = mc.history(name).shape
        nchunks = -(-chains // 16)
        assert nchunks <= 256 and blocks(steps, chains, d, mc.default_batch(steps)) % nchunks == 0, name   # nbx = nchunks


def test_numpy_path_matches_the_restatement_at_five_tiles():
    """"panel-d65" (40 x 33 x 65, batch 6, four leading rows in no batch) on the numpy path, as
    `test_numpy_path_matches_the_restatement` does."""
    from l2hmc_amd import multivariate
    X = mc.history("panel-d65")
    ref = mc.reference(X, 6)
    got = multivariate.multi_ess(X, 6)
    n = ref["n_draws"]
    scale = np.sqrt(np.outer(np.diag(ref["P"]), np.diag(ref["P"])))
    qscale = np.sqrt(np.outer(np.diag(ref["Q"]), np.diag(ref["Q"])))
    assert (got.n_draws, got.batch_size, got.n_batches) == (1320, 6, 198) and not got.degenerate.any()
    assert np.max(np.abs(got.cov * (n - 1) - ref["P"]) / scale) < 1e-12
    assert np.max(np.abs(got.cov_asymptotic * (198 - 1) / 6 - ref["Q"]) / qscale) < 1e-12
    assert np.max(np.abs(got.mean - ref["mean"]) / ref["sd"]) < 1e-12
    assert np.max(np.abs(got.ess_batch - ref["ess_batch"]) / ref["ess_batch"]) < 1e-10
    assert abs(got.multi_ess - ref["multi_ess"]) / ref["multi_ess"] < 1e-10


@pytest.mark.parametrize("name", sorted(mc.PLAN_FIXTURES))
def test_both_covariances_are_symmetric_bit_for_bit(name):
    """`finish` takes the raw moments apart entry by entry: (i, j) and (j, i) must go through the same additions in the same
    order.  (Q = batch_cross - mu sb^T - sb mu^T + A mu mu^T subtracted one term after the other did not: "panel-d65" and
    "panel-d128" had 4 and 2 entries of `cov_asymptotic` one ulp from their mirror image.)"""
    from l2hmc_amd import multivariate
    got = multivariate.multi_ess(mc.history(name), mc.PLAN_FIXTURES[name][3])
    assert np.array_equal(got.cov, got.cov.T) and np.array_equal(got.cov_asymptotic, got.cov_asymptotic.T)
    assert np.array_equal(got.corr, got.corr.T)


def test_raw_sums_and_batch_edges():
    from l2hmc_amd import multivariate
    X = mc.history("B")                                                        # 257 steps: batch rows start at row 1
    s = multivariate.moment_sums(X, 16)
    ref = mc.reference(X, 16)
    assert s["n_draws"] == 257 * 200 and s["n_batches"] == 16 * 200 and s["batch_size"] == 16
    for key in ("sum", "cross", "batch_sum", "batch_cross"):
        assert np.max(np.abs(np.asarray(s[key], dtype=np.float64) - ref[key]) / np.max(np.abs(ref[key]))) < 1e-12, key
    none = multivariate.moment_sums(X, 0)
    assert none["batch_sum"] is None and none["batch_cross"] is None and none["n_batches"] == 0
    one = multivariate.multi_ess(X, 1)                                         # Sigma == Lambda
    assert abs(one.multi_ess / one.n_draws - 1) < 1e-9
    whole = multivariate.multi_ess(X, 257)
    assert whole.n_batches == 200 and np.isfinite(whole.multi_ess)


def test_bad_shapes_and_batch_sizes_raise_value_error():
    from l2hmc_amd import multivariate
    X = mc.history("E")
    for bad in (0, -1, 51, 2.5):
        with pytest.raises(ValueError):
            multivariate.multi_ess(X, bad)
    with pytest.raises(ValueError):
        multivariate.multi_ess(X.reshape(-1, 1))                               # needs a history of chains
    with pytest.raises(ValueError):
        multivariate.moment_sums(X.reshape(-1, 1), 5)
    for bad in (X[0, 0], X[None], X[:0]):
        with pytest.raises(ValueError):
            multivariate.covariance(bad)


def test_too_few_batches_are_refused_and_covariance_is_not():
    """Fixture "D": d = 130, 64 steps x 16 chains, default batch 8 -> 128 batches <= d: Sigma would be singular."""
    from l2hmc_amd import multivariate
    X = mc.history("D")
    with pytest.raises(ValueError, match="n_batches = 128"):
        multivariate.multi_ess(X)
    c = multivariate.covariance(X)
    ref = mc.reference(X, 0)
    assert c.cov.shape == (130, 130) and not c.degenerate.any()
    assert np.max(np.abs(c.cov - ref["cov"]) / np.outer(ref["sd"], ref["sd"])) < 1e-12


def test_degenerate_coordinates_on_numpy():
    from tests import quantiles_case as qc
    from l2hmc_amd import multivariate
    X, _ = qc.adversarial()
    got = multivariate.multi_ess(X)
    assert np.array_equal(np.flatnonzero(got.degenerate), [1, 3, 4, 11]) and np.isnan(got.multi_ess)
    bad = np.zeros((17, 17), dtype=bool)
    bad[[4, 11], :] = True
    bad[:, [4, 11]] = True
    assert np.array_equal(np.isnan(got.cov), bad)
    deg = np.zeros((17, 17), dtype=bool)
    deg[[1, 3, 4, 11], :] = True
    deg[:, [1, 3, 4, 11]] = True
    assert np.array_equal(np.isnan(got.corr), deg)


def test_package_exports_the_module():
    import l2hmc_amd
    assert l2hmc_amd.multivariate.covariance is l2hmc_amd.covariance
    assert l2hmc_amd.multivariate.multi_ess is l2hmc_amd.multi_ess
    assert {"multivariate", "covariance", "multi_ess"} <= set(l2hmc_amd.__all__)
    assert callable(l2hmc_amd.sharding.multivariate) if hasattr(l2hmc_amd, "sharding") else True


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the new entries (ABI version still 6); the host refuses bad
    arguments with L2HMC_ERR_ARG and a message that names the entry and the limit, before anything is launched."""
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS, name
    L = _ffi.lib()
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws = L.l2hmc_moment_sums_workspace_doubles
    assert ws(1000, 4096, 25, 31) > 0 and ws(50, 5, 1, 0) > 0 and ws(64, 32, 128, 8) > 0
    assert ws(1000, 4096, 25, 0) * 2 == ws(1000, 4096, 25, 31)                # no batches: one accumulator set
    assert ws(1000, 4096, 128, 31) * 8 <= 64 << 20                            # the header's "53 MB at most"
    one = 0x1000                                                              # a non-NULL pointer nothing dereferences: refused first
    refusals = (((100, 8, 129, 5), b"d <= 128"), ((100, 8, 0, 5), b"d <= 128"), ((0, 8, 25, 0), b"must be >= 1"),
                ((100, 0, 25, 5), b"must be >= 1"), ((100, 8, 25, -1), b"batch"), ((100, 8, 25, 101), b"batch"),
                ((100, 1 << 40, 25, 5), b"too large"), (((1 << 31) + 1, 8, 25, 5), b"too large"))
    for args, msg in refusals:
        assert ws(*args) == -1, args
        assert msg in L.l2hmc_last_error() and b"l2hmc_moment_sums_workspace_doubles:" in L.l2hmc_last_error(), L.l2hmc_last_error()
        assert L.l2hmc_moment_sums(one, *args, one, one, one, one, one, None) == -1, args
        assert msg in L.l2hmc_last_error() and b"l2hmc_moment_sums:" in L.l2hmc_last_error(), L.l2hmc_last_error()
    for call in (lambda: L.l2hmc_moment_sums(None, 100, 8, 25, 5, one, one, one, one, one, None),
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 5, None, one, one, one, one, None),
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 5, one, None, one, one, one, None),
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 5, one, one, one, one, None, None),
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 5, one, one, None, one, one, None),   # batch outputs missing
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 5, one, one, one, None, one, None)):
        assert call() == -1
        assert b"required" in L.l2hmc_last_error() and b"l2hmc_moment_sums:" in L.l2hmc_last_error(), L.l2hmc_last_error()
    for call in (lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 0, one, one, one, None, one, None),   # given with batch = 0
                 lambda: L.l2hmc_moment_sums(one, 100, 8, 25, 0, one, one, None, one, one, None)):
        assert call() == -1
        assert b"must be NULL when batch = 0" in L.l2hmc_last_error(), L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(L.l2hmc_moment_sums(None, 100, 8, 25, 0, None, None, None, None, None, None))


def test_moment_kernels_use_no_scratch():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of the
    moment-sums unit spills -- 16 tile pairs x 2 sets of float64 accumulators are 256 of a lane's 512 registers -- and the
    MFMA kernel exists under its name, with the f64 matrix instruction in it."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("moment_sums.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    names = {k for k, _, _, _ in rows}
    assert "moment_reduce_kernel" in names, names
    assert {"moment_panel_kernel<%d, %d, true>" % (t, t) for t in (1, 2, 3, 4)} <= names, names
    assert {"moment_panel_kernel<4, %d, false>" % t for t in (1, 2, 3, 4)} <= names, names
    for k, vg, sc, _ in rows:
        assert sc == 0 and vg <= 512, (k, vg, sc)
    text = open(os.path.join(kr.ASM, "moment_sums.s")).read()
    assert "v_mfma_f64_16x16x4_f64" in text or "v_mfma_f64_16x16x4f64" in text


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, X, out):
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
        s = sharding.multivariate(X[:, lo:hi])
        out.put((rank, dict(s), tuple(calls)))
        dist.barrier()
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_ranks_reproduce_the_single_process_value():
    """Chains sharded 23 + 41 over two gloo ranks: ONE all-reduce of 2 (1 + d + d^2) numbers (two float64 each), and every result within 1e-12
    of `multi_ess` on all 64 chains."""
    import torch.multiprocessing as mp
    from l2hmc_amd import multivariate
    X = np.array(mc.history("A"))
    ctx = mp.get_context("spawn")
    out = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, X, out)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(100)
        assert pr.exitcode == 0
    res = dict((r, (s, c)) for r, s, c in (out.get() for _ in range(2)))
    ref = multivariate.multi_ess(X)
    d = X.shape[2]
    for rank in (0, 1):
        s, calls = res[rank]
        assert calls == (2 * 2 * (1 + d + d * d),), calls          # every number as head and rest
        assert s["n_draws"] == ref.n_draws and s["n_batches"] == ref.n_batches and s["batch_size"] == ref.batch_size
        scale = np.outer(ref.sd, ref.sd)
        assert np.max(np.abs(s["cov"] - ref.cov) / scale) < 1e-12
        assert np.max(np.abs(s["cov_asymptotic"] - ref.cov_asymptotic) / np.sqrt(np.outer(np.diag(ref.cov_asymptotic),
                                                                                           np.diag(ref.cov_asymptotic)))) < 1e-12
        assert abs(s["multi_ess"] - ref.multi_ess) / ref.multi_ess < 1e-12
        assert np.max(np.abs(s["ess_batch"] - ref.ess_batch) / ref.ess_batch) < 1e-12
    assert np.array_equal(res[0][0]["cov"], res[1][0]["cov"])            # every rank ends with the same numbers


def test_flat_draws_are_factored_into_chains():
    """(draws, d) without batches: the kernels fill their lanes with adjacent chains, so the draws are read as
    (draws / c, c, d) with c the largest divisor up to 4096; the sums do not depend on the factorisation."""
    from l2hmc_amd import multivariate
    assert multivariate._layout(np.zeros((400000, 3)), 0) == (100, 4000, 3)
    assert multivariate._layout(np.zeros((8192, 3)), 0) == (2, 4096, 3)
    assert multivariate._layout(np.zeros((7, 3)), 0) == (1, 7, 3)
    assert multivariate._layout(np.zeros((4099, 3)), 0) == (4099, 1, 3)          # a prime
    assert multivariate._layout(np.zeros((5, 4, 3)), 0) == (5, 4, 3)
    X = mc.history("F")
    a, b = multivariate.covariance(X), multivariate.covariance(X.reshape(-1, X.shape[2]))
    assert a.n_draws == b.n_draws and np.array_equal(a.cov, b.cov) and np.array_equal(a.mean, b.mean)
