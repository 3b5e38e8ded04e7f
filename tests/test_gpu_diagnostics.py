"""GPU: the convergence-diagnostic kernels (csrc/chain_stats.hip behind `l2hmc_chain_stats`) against the float64 restatement
of tests/diagnostics_case.py -- raw sums, the finished numbers, bitwise reproducibility, and the histories the library's own
samplers write.

Gates (derived, not tuned).  mean: 1e-10 of |mean| + sd (float64 accumulation of float32 values).  M2 and every G[k, t]: 2e-5
of G[k, 0] -- a chunk of float32 FMAs of at most 64 steps is off by at most 64 * 2^-24 = 3.8e-6 of the sum of |products|, which
is at most G[k, 0] by Cauchy-Schwarz; rounding the centred values adds 2^-23 of the same; a factor 5 on top for the float64
fold.  rhat: 2e-5 relative.  ess: the ceiling is (max_lag + 1) * 4e-5 / tau (every pair off by the bound, the same way), about
1e-2 at max_lag = 255, tau = 1; the gate is ten times the worst deviation measured on the MI355X (profiles/
diagnostics_accuracy.txt: 8.47e-8 over the six fixtures, split and unsplit) or the ceiling, whichever is smaller.

The six fixtures all get one column chunk per block and d <= 130; the histories of diagnostics_case.PLAN_FIXTURES reach the
rest of the plan (several chunks per block, d > 256) under the same derived gates, ess under the ceiling alone."""
import numpy as np
import pytest
import torch

from tests import diagnostics_case as dc

pytestmark = pytest.mark.gpu
NAMES = sorted(dc.FIXTURES)
ESS_MEASURED = 8.47e-8         # worst relative deviation of ess from the restatement, profiles/diagnostics_accuracy.txt
_REF = {}


def _case(name, split, max_lag=None):
    X, lag = dc.fixture(name)
    lag = lag if max_lag is None else max_lag
    key = (name, split, lag)
    if key not in _REF:
        _REF[key] = dc.reference_summary(X, lag, split)
    return X, lag, _REF[key]


def _sums_errors(sums, ref):
    mean, m2, G = ref["sums"]
    sd = np.sqrt(m2 / (ref["n_steps"] - 1))
    got_mean, got_m2, got_G = (sums[k].cpu().numpy() for k in ("mean", "m2", "G"))
    e_mean = np.max(np.abs(got_mean - mean) / (np.abs(mean) + sd))
    g0 = G[:, 0]
    e_m2 = np.max(np.abs(got_m2 - m2).sum(axis=0) / g0)            # every chain's M2 error together, against sum_c M2
    e_G = np.max(np.abs(got_G - G) / g0[:, None])
    return e_mean, e_m2, e_G


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name,max_lag", [(n, None) for n in NAMES] + [("A", 37)])
def test_raw_sums_match_the_restatement(name, max_lag, split):
    from l2hmc_amd import diagnostics
    X, lag, ref = _case(name, split, max_lag)
    sums = diagnostics.chain_sums(torch.as_tensor(X).cuda(), lag, split)
    assert sums["mean"].dtype == torch.float64 and sums["G"].is_cuda
    assert tuple(sums["mean"].shape) == ref["sums"][0].shape and tuple(sums["G"].shape) == (X.shape[2], lag + 1)
    assert (sums["n_steps"], sums["n_chains"]) == (ref["n_steps"], ref["n_chains"])
    e_mean, e_m2, e_G = _sums_errors(sums, ref)
    print("fixture %s max_lag %d split %d: mean %.3g of |mean| + sd, M2 %.3g and G %.3g of G[k, 0]" % (name, lag, split, e_mean,
                                                                                                     e_m2, e_G))
    assert e_mean < 1e-10
    assert e_m2 < 2e-5 and e_G < 2e-5


def ess_gate(max_lag, tau):
    return np.minimum(10 * ESS_MEASURED, (max_lag + 1) * 4e-5 / tau)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_summarize_matches_the_restatement(name, split):
    from l2hmc_amd import diagnostics
    X, lag, ref = _case(name, split)
    got = diagnostics.summarize(torch.as_tensor(X).cuda(), lag, split)
    assert np.array_equal(got.truncated, ref["truncated"])
    e_rhat = np.max(np.abs(got.rhat - ref["rhat"]) / ref["rhat"])
    e_ess = np.abs(got.ess - ref["ess"]) / np.abs(ref["ess"])
    e_sd = np.max(np.abs(got.sd - ref["sd"]) / ref["sd"])
    print("fixture %s split %d: rhat %.3g, sd %.3g, ess %.3g relative (gate %.3g)" % (
        name, split, e_rhat, e_sd, e_ess.max(), ess_gate(lag, ref["tau"]).min()))
    assert e_rhat < 2e-5 and e_sd < 2e-5
    assert np.all(e_ess < ess_gate(lag, ref["tau"]))
    assert np.max(np.abs(got.mean - ref["mean"]) / (np.abs(ref["mean"]) + ref["sd"])) < 1e-10
    assert (got.n_steps, got.n_chains, got.max_lag) == (ref["n_steps"], ref["n_chains"], lag)


PLAN_NAMES = sorted(dc.PLAN_FIXTURES)
_PLAN_REF = {}


def _plan_case(name):
    """(X, max_lag, split, the column restatement's summary) of a history of diagnostics_case.PLAN_FIXTURES, computed once"""
    if name not in _PLAN_REF:
        X, lag, split = dc.plan_fixture(name)
        _PLAN_REF[name] = (X, lag, split, dc.reference_summary_columns(X, lag, split))
    return _PLAN_REF[name]


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_raw_sums_across_chunks_and_wide_histories(name):
    """The branches of the plan "A" .. "F" never take (tests/diagnostics_case.py states each history's plan,
    tests/test_diagnostics_cpu.py pins it): a block that walks two or three column chunks with its 32 float64 sums and its
    coordinate in registers, in the first lag tile and in one that reloads x_t; a ragged last chunk as a block's SECOND chunk;
    d > 256, where a block holds 256 of the coordinates and the reducer skips the blocks that do not hold coordinate k; d = 512.
    Every coordinate has its own phi, mean and sd, so the gates of `test_raw_sums_match_the_restatement` -- unchanged --
    catch a coordinate that slips (orders of magnitude) and a chunk dropped or added twice (>= 1 / 600 of G[k, 0])."""
    from l2hmc_amd import diagnostics
    X, lag, split, ref = _plan_case(name)
    sums = diagnostics.chain_sums(torch.as_tensor(X).cuda(), lag, split)
    assert tuple(sums["mean"].shape) == ref["sums"][0].shape and tuple(sums["G"].shape) == (X.shape[2], lag + 1)
    assert (sums["n_steps"], sums["n_chains"]) == (ref["n_steps"], ref["n_chains"])
    e_mean, e_m2, e_G = _sums_errors(sums, ref)
    print("fixture %s max_lag %d split %d: mean %.3g of |mean| + sd, M2 %.3g and G %.3g of G[k, 0]" % (name, lag, split, e_mean,
                                                                                                     e_m2, e_G))
    assert e_mean < 1e-10
    assert e_m2 < 2e-5 and e_G < 2e-5


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_summarize_across_chunks_and_wide_histories(name):
    """The finished numbers of the same histories.  ess: the derived ceiling (max_lag + 1) * 4e-5 / tau alone -- `ESS_MEASURED`
    was measured on "A" .. "F" and says nothing here (profiles/diagnostics_accuracy.txt has these histories' own figures)."""
    from l2hmc_amd import diagnostics
    X, lag, split, ref = _plan_case(name)
    got = diagnostics.summarize(torch.as_tensor(X).cuda(), lag, split)
    assert np.array_equal(got.truncated, ref["truncated"])
    e_rhat = np.max(np.abs(got.rhat - ref["rhat"]) / ref["rhat"])
    e_ess = np.abs(got.ess - ref["ess"]) / np.abs(ref["ess"])
    e_sd = np.max(np.abs(got.sd - ref["sd"]) / ref["sd"])
    ceiling = (lag + 1) * 4e-5 / ref["tau"]
    print("fixture %s split %d: rhat %.3g, sd %.3g, ess %.3g relative (smallest ceiling %.3g)" % (
        name, split, e_rhat, e_sd, e_ess.max(), ceiling.min()))
    assert e_rhat < 2e-5 and e_sd < 2e-5
    assert np.all(e_ess < ceiling)
    assert np.max(np.abs(got.mean - ref["mean"]) / (np.abs(ref["mean"]) + ref["sd"])) < 1e-10
    assert (got.n_steps, got.n_chains, got.max_lag) == (ref["n_steps"], ref["n_chains"], lag)


def test_two_calls_across_chunks_give_identical_bits():
    """"period65-d130": 520 blocks over 559 chunks, the threads of a coordinate added through LDS after the last chunk."""
    from l2hmc_amd import diagnostics
    X, lag, split, _ = _plan_case("period65-d130")
    Xd = torch.as_tensor(X).cuda()
    a = diagnostics.chain_sums(Xd, lag, split)
    torch.empty(1 << 24, device="cuda").normal_()                  # other work, another workspace address
    b = diagnostics.chain_sums(Xd.clone(), lag, split)
    for k in ("mean", "m2", "G"):
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def test_two_calls_give_identical_bits():
    """Per-block partial sums added in block order, no floating-point atomics: the contract `l2hmc_autocov` has with a
    workspace."""
    from l2hmc_amd import diagnostics
    X, lag = dc.fixture("C")
    Xd = torch.as_tensor(X).cuda()
    a = diagnostics.chain_sums(Xd, lag)
    torch.empty(1 << 24, device="cuda").normal_()                  # other work, another workspace address
    b = diagnostics.chain_sums(Xd.clone(), lag)
    for k in ("mean", "m2", "G"):
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def test_views_and_other_dtypes_are_not_misread():
    from l2hmc_amd import diagnostics
    X, lag = dc.fixture("F")
    Xd = torch.as_tensor(X).cuda()
    want = diagnostics.chain_sums(Xd, lag)

    def same(Y, ref=want):
        got = diagnostics.chain_sums(Y, lag)
        return all(torch.equal(got[k], ref[k]) for k in ("mean", "m2", "G"))
    assert same(Xd.double())                                       # float64 on the device: values are float32-exact
    assert same(Xd.permute(1, 0, 2).contiguous().permute(1, 0, 2))  # the same history, chain-major in memory
    big = torch.zeros((X.shape[0] + 9,) + X.shape[1:], device="cuda")
    big[9:] = Xd
    assert same(big[9:])                                           # a burn-in slice is contiguous: read in place
    assert same(Xd[:, ::2], diagnostics.chain_sums(Xd[:, ::2].contiguous(), lag))
    assert same(Xd[:, :, 3:9], diagnostics.chain_sums(Xd[:, :, 3:9].contiguous(), lag))


def test_degenerate_coordinates_are_nan_alone_on_the_device():
    from l2hmc_amd import diagnostics
    X, lag, ref = _case("F", True)
    Y = X.copy()
    Y[:, :, 3] = 2.5
    Y[40, 7, 11] = np.nan
    Y[95, 0, 12] = np.inf                                          # the last row of a series
    got = diagnostics.summarize(torch.as_tensor(Y).cuda(), lag)
    bad = np.zeros(X.shape[2], dtype=bool)
    bad[[3, 11, 12]] = True
    assert np.all(np.isnan(got.rhat[bad])) and np.all(np.isnan(got.ess[bad]))
    assert np.max(np.abs(got.rhat[~bad] - ref["rhat"][~bad]) / ref["rhat"][~bad]) < 2e-5
    assert np.all(np.abs(got.ess[~bad] - ref["ess"][~bad]) / ref["ess"][~bad] < ess_gate(lag, ref["tau"][~bad]))
    assert got.mean[3] == 2.5 and got.sd[3] == 0.0


def test_device_refuses_what_the_host_refuses():
    from l2hmc_amd import diagnostics
    Xd = torch.as_tensor(dc.ar1(40, 6, [0.5, 0.1], 0)).cuda()
    for args, kw in (((Xd[:7],), {}), ((Xd[:, :1],), {"split": False}), ((Xd, 20), {})):
        with pytest.raises(ValueError):
            diagnostics.chain_sums(*args, **kw)
    wide = torch.zeros((16, 4, 513), device="cuda")
    with pytest.raises(ValueError, match="dim <= 512"):
        diagnostics.chain_sums(wide)
    from l2hmc_amd import _ffi
    assert _ffi.lib().l2hmc_chain_stats_workspace_doubles(16, 4, 513, 3, 1) == -1       # the C ABI refuses it too


VAR = np.linspace(0.25, 4.0, 8)


def _gaussian_hmc():
    """HMC on a zero-mean diagonal Gaussian, variances 0.25 .. 4: eps = 0.6, 3 leapfrog steps (a float64 numpy simulation
    of this configuration accepts 0.885, reaches max R-hat 1.012 after 100 of 400 proposals and truncates no coordinate)."""
    from l2hmc_amd import Dynamics
    from l2hmc_amd import distributions as D
    e = D.Gaussian(np.zeros(8), np.diag(VAR)).get_energy_function()
    dyn = Dynamics(8, e, T=3, eps=0.6, hmc=True)
    dyn.eps_override = 0.6
    return dyn


def _check_known_gaussian(s, label):
    z = np.abs(s.mean) / (s.sd / np.sqrt(s.ess))
    print("%s: max rhat %.4f, min ess %.0f of %d, worst |mean| %.2f standard errors, sd / true in [%.3f, %.3f]" % (
        label, s.max_rhat, s.min_ess, s.n_steps * s.n_chains, z.max(), (s.sd / np.sqrt(VAR)).min(), (s.sd / np.sqrt(VAR)).max()))
    assert s.max_rhat < 1.05
    assert np.all(s.ess > 0) and np.all(z < 5)
    assert np.all(np.abs(s.sd / np.sqrt(VAR) - 1) < 0.1)


def test_reads_the_history_sample_chain_records():
    from l2hmc_amd import diagnostics, sample_chain
    dyn = _gaussian_hmc()
    x0 = torch.as_tensor((np.random.RandomState(0).randn(512, 8) * np.sqrt(VAR)).astype(np.float32)).cuda()
    _, p, hist = sample_chain(x0, dyn, 400, record=True, seed=3)
    accept = float(p.mean())
    print("accept rate %.3f" % accept)
    assert 0.6 < accept < 0.95
    assert tuple(hist.shape) == (400, 512, 8)
    s = diagnostics.summarize(hist[100:])
    assert (s.n_steps, s.n_chains) == (150, 1024)
    _check_known_gaussian(s, "sample_chain")


def test_reads_the_cold_history_of_parallel_tempering():
    from l2hmc_amd import ParallelTempering, diagnostics
    dyn = _gaussian_hmc()
    pt = ParallelTempering(dyn, [1.0, 2.0], 512, seed=5)
    x0 = torch.as_tensor((np.random.RandomState(1).randn(1024, 8) * np.sqrt(VAR)).astype(np.float32)).cuda()
    o = pt.run(x0, 400, 1, record_cold=True)
    assert tuple(o["cold_hist"].shape) == (400, 512, 8)
    s = diagnostics.summarize(o["cold_hist"][100:])
    _check_known_gaussian(s, "cold rung")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
def test_history_on_another_device_is_read_there():
    """Every statistic launches on the device its history lies on, whichever device is current, and leaves the current
    device alone: the results for a history on cuda:1 equal those for the same history on cuda:0 bit for bit."""
    from l2hmc_amd import diagnostics, func_utils, multivariate, predictive, quantiles
    X = dc.ar1(16, 4, [0.5, 0.1, 0.8], 0).astype(np.float32)
    rng = np.random.RandomState(1)
    rows, y = 0.2 * rng.randn(5, 3), (rng.rand(5) < 0.5).astype(np.float64)
    calls = (lambda H: diagnostics.summarize(H), lambda H: quantiles.order_statistics(H, np.arange(0, 64, 9)),
             lambda H: multivariate.covariance(H), lambda H: predictive.waic(H, rows, y),
             lambda H: func_utils.acl_spectrum(H, 1.7))

    def raw(v):
        if isinstance(v, dict):
            return [(k, raw(v[k])) for k in sorted(v)]
        if isinstance(v, tuple):
            return [raw(e) for e in v]
        return np.asarray(v).tobytes()
    torch.cuda.set_device(0)
    here, there = torch.as_tensor(X).to("cuda:0"), torch.as_tensor(X).to("cuda:1")
    for i, call in enumerate(calls):
        assert raw(call(there)) == raw(call(here)), i
        assert torch.cuda.current_device() == 0, i
