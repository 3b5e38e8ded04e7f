"""GPU: exact order statistics on the device (csrc/order_stats.hip behind `l2hmc_order_stats`), the indicator form of the chain
sums (`l2hmc_chain_stats_below`) and `quantiles.describe` on top of them, against the restatement of tests/quantiles_case.py.

Shapes: the smallest at which the count pass's plan can go wrong.  The plan (csrc/order_stats.hip, `order_stats_plan`): a group
is sg <= 64 / rg coordinates x rg ranks (rg = 1 in pass 0, otherwise the power of two with the fewest groups), ngk coordinate
and ngr rank groups; a block step is rpc = 256 // sg rows, the LDS histogram has min(64 // (sg rg), rpc) copies; nb =
max(1024 // (ngk ngr), 64) blocks along x, at most ceil(S / rpc), and a block walks ceil(S / rpc) / nb steps -- 8 or more enter
the software-pipelined load loop.  By that plan, for 5 standard ranks / a table of 32:
 - "E" (d = 1, S = 250): one block, one step, 64 copies; later passes rg 8 / 32, 8 / 2 copies;
 - "F" and the adversarial history (d = 17, S = 7392, N d odd): sg 17, 15 rows per step with one idle thread, 3 copies, one
   step; later passes rg 2 x 3 rank groups, 341 blocks and 1 or 2 steps / rg 32, 9 groups of 2 coordinates, one step;
 - "D" (d = 130, S = 1024): 3 groups of 44 (2 idle coordinates), rpc 5, one step; later passes 3 x 5 groups, 68 blocks and 3 or
   4 steps / rg 32, 65 groups of 2, one step;
 - "B" (d = 2, S = 51 400): 32 copies, rpc 128, 402 chunks in 402 blocks -- ONE step per block in every pass (rg 8 / 32);
 - "C" (d = 25, S = 400 000, through `describe` with 3 to 5 ranks only): 39 to 118 steps;
so of these only "C" reaches the pipelined loop, never with a rank table, and none has d > 130.  The histories of
quantiles_case.PLAN_FIXTURES close that; `test_order_statistics_are_exact_where_blocks_walk_far` derives their plans.

Gates.  Order statistics and quantiles: exact / 1e-15.  The indicator sums carry the gates tests/test_gpu_diagnostics.py
derives for the same arithmetic: mean 1e-10 of |mean| + sd, M2 and G 2e-5 of G[k, 0].  ess_quantile: the derived ceiling
(max_lag + 1) * 4e-5 / tau, or ten times the worst deviation measured on the MI355X (profiles/quantiles_accuracy.txt: 2.47e-7
over the six fixtures, split and unsplit, at p = 0.05, 0.5, 0.95), whichever is smaller."""
import numpy as np
import pytest
import torch

from tests import diagnostics_case as dc
from tests import quantiles_case as qc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
ESS_QUANTILE_MEASURED = 2.47e-7          # worst relative deviation of ess_quantile, profiles/quantiles_accuracy.txt
_HIST, _REF = {}, {}


def _history(name):
    if name not in _HIST:
        _HIST[name] = qc.adversarial() if name == "adversarial" else dc.fixture(name)
    return _HIST[name]


def _described(name, split):
    if (name, split) not in _REF:
        X, lag = _history(name)
        _REF[(name, split)] = qc.reference_describe(X, lag, split)
    return _REF[(name, split)]


@pytest.mark.parametrize("name", ["E", "F", "D", "B", "adversarial"])
def test_order_statistics_are_exact(name):
    from l2hmc_amd import quantiles
    X, _ = _history(name)
    Xd = torch.as_tensor(X).cuda()
    S, d = X.shape[0] * X.shape[1], X.shape[2]
    for ranks in (qc.standard_ranks(S), qc.rank_table(S, d, seed=1)):
        want, want_nan = qc.reference_order_statistics(X, ranks)
        got, got_nan = quantiles.order_statistics(Xd, ranks)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got_nan, want_nan)
        ok = want_nan == 0
        assert np.array_equal(got[:, ok], want[:, ok]), np.argwhere(got != want)[:8]
        assert np.all(np.isnan(got[-1, ~ok]))                           # NaNs sort last: rank S - 1 of such a coordinate


@pytest.mark.parametrize("name,table_rows", [("long-walk-d70", 32), ("groups-d512", 3), ("copies-d3", 20)])
def test_order_statistics_are_exact_where_blocks_walk_far(name, table_rows):
    """Bit-exact against np.sort, at the standard ranks (R = 5) and a per-coordinate table, where the plan (module docstring)
    leaves what the other histories reach:
     - "long-walk-d70" (S = 140 000, d = 70), hostile coordinates included.  Pass 0: 2 groups of sg 35, rpc 7, 1 copy, 20 000
       chunks over nb = 512: 39 or 40 steps, four or five rounds of the pipelined loop and a tail.  Later passes, R = 5: rg 2,
       ngk 3 (sg 24, two idle coordinates), ngr 3 (the last with one rank), rpc 10, nb = 113, 123 or 124 steps; R = 32: rg 32,
       ngk 35 groups of sg 2, ngr 1, rpc 128, 1094 chunks over nb = 64, 17 or 18 steps.
     - "groups-d512" (S = 4500, d = 512, the widest the entry accepts).  Pass 0: ngk 8 groups of sg 64, rpc 4, 1125 chunks over
       nb = 128, 8 or 9 steps (one round of the pipelined loop, a tail of 0 or 1).  Later passes: rg 1, ngk 8, ngr 5 / 3, nb = 64,
       17 or 18 steps.
     - "copies-d3" (S = 30 000, d = 3).  Pass 0: sg 3, rpc 85 (thread 255 idle), 21 copies, 63 LDS columns, 353 blocks of one
       step.  Later passes, R = 5: rg 8, 2 copies; R = 20: rg 16, ngr 2 (the second group with 4 of its 16 ranks), 1 copy."""
    from l2hmc_amd import quantiles
    X = qc.plan_history(name)
    Xd = torch.as_tensor(X).cuda()
    S, d = X.shape[0] * X.shape[1], X.shape[2]
    for ranks in (qc.standard_ranks(S), qc.rank_table(S, d, seed=1, R=table_rows)):
        want, want_nan = qc.reference_order_statistics(X, ranks)
        got, got_nan = quantiles.order_statistics(Xd, ranks)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got_nan, want_nan)
        ok = want_nan == 0
        assert np.array_equal(got[:, ok], want[:, ok]), np.argwhere(got != want)[:8]
        assert np.all(np.isnan(got[-1, ~ok]))                           # NaNs sort last: rank S - 1 of such a coordinate
        fin = ~np.isnan(want)
        assert np.array_equal(got[fin], want[fin])                      # and every other rank of it is a value
    assert want_nan.sum() == (1 if name == "long-walk-d70" else 0)


def test_nan_coordinate_is_nan_alone():
    from l2hmc_amd import quantiles
    X, _ = _history("adversarial")
    Xd = torch.as_tensor(X).cuda()
    _, n_nan = quantiles.order_statistics(Xd, [0])
    assert n_nan[qc.NAN_COORDINATE] == 1 and n_nan.sum() == 1
    probs = (0.0, 0.05, 0.333, 0.5, 0.95, 1.0)
    got, want = quantiles.quantiles(Xd, probs), qc.reference_quantiles(X, probs)
    assert np.all(np.isnan(got[:, qc.NAN_COORDINATE]))
    fin = np.isfinite(want)
    fin[:, qc.NAN_COORDINATE] = False
    assert fin.sum() >= 6 * 15
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-15 * np.abs(want[fin]))
    assert got[0, 4] == -np.inf and got[-1, 4] == np.inf                # +-inf are ordinary values


def _passes(L, Xd, ranks):
    """The select pass by pass through the two halves of the C ABI; also the histogram sums after the count of pass 0."""
    from l2hmc_amd import _ffi
    S, d = Xd.shape[0] * Xd.shape[1], Xd.shape[2]
    R, bins, passes = ranks.shape[0], L.l2hmc_order_stats_bins(), L.l2hmc_order_stats_passes()
    remaining = torch.as_tensor(ranks).cuda()
    prefix = torch.zeros((R, d), dtype=torch.int32, device="cuda")
    hist = torch.empty((R, d, bins), dtype=torch.int64, device="cuda")
    n_nan = torch.empty(d, dtype=torch.int64, device="cuda")
    values = torch.empty((R, d), dtype=torch.float32, device="cuda")
    stream = _ffi.current_stream(Xd.device)
    sums0 = None
    for p in range(passes):
        _ffi.check(L.l2hmc_order_stats_count(Xd.data_ptr(), S, d, R, p, prefix.data_ptr(), hist.data_ptr(),
                                             n_nan.data_ptr() if p == 0 else None, stream))
        if p == 0:
            sums0 = hist.sum(dim=2).cpu().numpy()
        _ffi.check(L.l2hmc_order_stats_advance(hist.data_ptr(), remaining.data_ptr(), prefix.data_ptr(), d, R, p,
                                               values.data_ptr() if p == passes - 1 else None, stream))
    return values.cpu().numpy(), n_nan.cpu().numpy(), sums0


def test_pass_by_pass_gives_the_bits_of_the_single_call():
    from l2hmc_amd import _ffi, quantiles
    L = _ffi.lib()
    X, _ = _history("adversarial")
    Xd = torch.as_tensor(X).cuda()
    S, d = X.shape[0] * X.shape[1], X.shape[2]
    ranks = qc.rank_table(S, d, seed=2, R=7)
    values, n_nan, sums0 = _passes(L, Xd, ranks)
    assert np.array_equal(sums0, np.full((7, d), S))                    # after the count of pass 0 every histogram holds S
    whole, whole_nan = quantiles.order_statistics(Xd, ranks)
    assert np.array_equal(values.view(np.uint32), whole.view(np.uint32)) and np.array_equal(n_nan, whole_nan)


def test_two_calls_give_identical_bits():
    from l2hmc_amd import quantiles
    X, _ = _history("B")
    Xd = torch.as_tensor(X).cuda()
    ranks = qc.rank_table(X.shape[0] * X.shape[1], X.shape[2], seed=3)
    a, _ = quantiles.order_statistics(Xd, ranks)
    torch.empty(1 << 24, device="cuda").normal_()                       # other work, another workspace address
    b, _ = quantiles.order_statistics(Xd.clone(), ranks)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_views_and_other_dtypes_are_not_misread():
    from l2hmc_amd import quantiles
    X, _ = _history("F")
    Xd = torch.as_tensor(X).cuda()
    probs = (0.05, 0.5, 0.95)
    want = quantiles.quantiles(Xd, probs)

    def close(got, Y):
        ref = qc.reference_quantiles(Y, probs)
        return np.all(np.abs(got - ref) <= 1e-15 * np.abs(ref))

    def same(Y, ref=want):
        return np.array_equal(quantiles.quantiles(Y, probs), ref)
    assert close(want, X)
    assert same(Xd.double())                                            # float64 on the device: values are float32-exact
    assert same(Xd.permute(1, 0, 2).contiguous().permute(1, 0, 2))      # the same history, chain-major in memory
    big = torch.zeros((X.shape[0] + 9,) + X.shape[1:], device="cuda")
    big[9:] = Xd
    assert same(big[9:])                                                # a burn-in slice is contiguous: read in place
    assert same(Xd.reshape(-1, X.shape[2]))                             # the (S, d) view
    for view, host in ((Xd[:, ::2], X[:, ::2]), (Xd[:, :, 3:9], X[:, :, 3:9])):
        assert same(view, quantiles.quantiles(view.contiguous(), probs)) and close(quantiles.quantiles(view, probs), host)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["A", "C", "F"])
def test_indicator_sums_match_the_restatement(name, split):
    """`l2hmc_chain_stats_below` at the restatement's own thresholds."""
    from l2hmc_amd import diagnostics
    X, lag = _history(name)
    ref = _described(name, split)
    Xd = torch.as_tensor(X).cuda()
    for i, p in enumerate(qc.PROBS):
        below = ref["below"][i]
        sums = diagnostics.chain_sums_below(Xd, ref["quantiles"][i], lag, split)
        mean, m2, G = below["sums"]
        sd = np.sqrt(m2 / (below["n_steps"] - 1))
        got_mean, got_m2, got_G = (sums[k].cpu().numpy() for k in ("mean", "m2", "G"))
        g0 = G[:, 0]
        scale = np.abs(mean) + sd                                       # 0 for a series that never reaches the threshold: exact 0
        e_mean = np.max(np.abs(got_mean - mean) / np.where(scale > 0, scale, 1.0))
        e_m2 = np.max(np.abs(got_m2 - m2).sum(axis=0) / g0)
        e_G = np.max(np.abs(got_G - G) / g0[:, None])
        print("fixture %s split %d p %.2f: mean %.3g of |mean| + sd, M2 %.3g and G %.3g of G[k, 0]" % (name, split, p, e_mean,
                                                                                                    e_m2, e_G))
        assert e_mean < 1e-10
        assert e_m2 < 2e-5 and e_G < 2e-5


@pytest.mark.parametrize("name", ["two-chunks-d3", "period65-d130", "period257-d257"])
def test_indicator_sums_across_chunks(name):
    """`l2hmc_chain_stats_below` where a block walks more than one column chunk (diagnostics_case.PLAN_FIXTURES: d = 3 with the
    ragged chunk as block 0's second, d = 130, and d = 257 where a block holds 256 of the coordinates): a thread's threshold is
    that of its coordinate in EVERY chunk.  The thresholds are the coordinates' own means, -2 .. 2 at sd 0.05 .. 2: under a
    neighbour's threshold an indicator series is another series.  Against the column restatement on the indicator history,
    under the gates of `test_indicator_sums_match_the_restatement`."""
    from l2hmc_amd import diagnostics
    X, lag, split = dc.plan_fixture(name)
    thresholds = dc.spread(X.shape[2])[1]
    mean, m2, G = dc.reference_sums_columns(qc.indicator_history(X, thresholds), lag, split)
    sums = diagnostics.chain_sums_below(torch.as_tensor(X).cuda(), thresholds, lag, split)
    Mh = sums["n_steps"]
    assert (Mh, sums["n_chains"]) == (X.shape[0] // 2, 2 * X.shape[1]) and split
    sd = np.sqrt(m2 / (Mh - 1))
    got_mean, got_m2, got_G = (sums[k].cpu().numpy() for k in ("mean", "m2", "G"))
    g0 = G[:, 0]
    assert np.all(g0 > 0)
    scale = np.abs(mean) + sd                                           # 0 for a series that never reaches the threshold: exact 0
    e_mean = np.max(np.abs(got_mean - mean) / np.where(scale > 0, scale, 1.0))
    e_m2 = np.max(np.abs(got_m2 - m2).sum(axis=0) / g0)
    e_G = np.max(np.abs(got_G - G) / g0[:, None])
    print("fixture %s: mean %.3g of |mean| + sd, M2 %.3g and G %.3g of G[k, 0]" % (name, e_mean, e_m2, e_G))
    assert e_mean < 1e-10
    assert e_m2 < 2e-5 and e_G < 2e-5


def ess_gate(max_lag, tau):
    return np.minimum(10 * ESS_QUANTILE_MEASURED, (max_lag + 1) * 4e-5 / tau)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["A", "C", "F"])
def test_describe_matches_the_restatement(name, split):
    from l2hmc_amd import diagnostics, quantiles
    X, lag = _history(name)
    ref = _described(name, split)
    Xd = torch.as_tensor(X).cuda()
    got = quantiles.describe(Xd, qc.PROBS, lag, split)
    assert np.all(np.abs(got.quantiles - ref["quantiles"]) <= 1e-15 * np.abs(ref["quantiles"]))
    assert np.array_equal(got.probs, qc.PROBS)
    assert np.array_equal(got.truncated_quantile, ref["truncated_quantile"])
    e_ess = np.abs(got.ess_quantile - ref["ess_quantile"]) / ref["ess_quantile"]
    gate = ess_gate(lag, ref["tau_quantile"])
    print("fixture %s split %d: ess_quantile %.3g relative (smallest gate %.3g)" % (name, split, e_ess.max(), gate.min()))
    assert np.all(e_ess < gate)
    assert np.array_equal(got.ess_tail, np.minimum(got.ess_quantile[0], got.ess_quantile[2]))
    # mcse_quantile is a pair of order statistics at positions that are floor / ceil of a function of ess_quantile: the
    # definition evaluated at the ess_quantile the device found must give the very same draws
    X2 = qc.draws(X)
    for k in range(X.shape[2]):
        col = np.sort(X2[:, k])
        for i, p in enumerate(qc.PROBS):
            assert got.mcse_quantile[i, k] == qc.reference_mcse_quantile(col, got.ess_quantile[i, k], p), (i, k)
    e_mcse = np.abs(got.mcse_quantile - ref["mcse_quantile"]) / ref["mcse_quantile"]
    print("mcse_quantile against the restatement's own ess: worst %.3g relative" % e_mcse.max())
    base = diagnostics.summarize(Xd, lag, split)
    for key in base:
        assert np.array_equal(got[key], base[key], equal_nan=True), key
    assert np.array_equal(got.mcse_mean, base.sd / np.sqrt(base.ess)) and got.n_nan.sum() == 0


VAR = np.linspace(0.25, 4.0, 8)


def test_end_to_end_on_a_known_gaussian():
    """HMC on the zero-mean diagonal Gaussian of tests/test_gpu_diagnostics.py (variances 0.25 .. 4, eps = 0.6, 3 leapfrog
    steps), 512 chains, 400 proposals, 100 discarded: the quantiles of every coordinate against -1.6449 sigma, 0, +1.6449 sigma
    in units of their own MCSE."""
    from l2hmc_amd import Dynamics, describe, sample_chain
    from l2hmc_amd import distributions as D
    e = D.Gaussian(np.zeros(8), np.diag(VAR)).get_energy_function()
    dyn = Dynamics(8, e, T=3, eps=0.6, hmc=True)
    dyn.eps_override = 0.6
    x0 = torch.as_tensor((np.random.RandomState(0).randn(512, 8) * np.sqrt(VAR)).astype(np.float32)).cuda()
    _, _, hist = sample_chain(x0, dyn, 400, record=True, seed=3)
    s = describe(hist[100:])
    S = 300 * 512
    want = np.array([-1.6449, 0.0, 1.6449])[:, None] * np.sqrt(VAR)[None, :]
    z = np.abs(s.quantiles - want) / s.mcse_quantile
    print("worst quantile error %.2f mcse; ess_tail %.0f .. %.0f of %d; mcse_quantile %.3g .. %.3g" % (
        z.max(), s.ess_tail.min(), s.ess_tail.max(), S, s.mcse_quantile.min(), s.mcse_quantile.max()))
    assert np.all(s.mcse_quantile > 0)
    assert np.all(z < 5)
    assert np.all(s.ess_tail > 0) and np.all(s.ess_tail <= S)
    assert s.n_nan.sum() == 0 and s.quantiles.shape == (3, 8)
