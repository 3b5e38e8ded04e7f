"""GPU: `l2hmc_loglik_tails` against an exact numpy selection on the same float32 matrix (cutoff, top, n_tail, the tail and its
draws as sets, bit for bit; the three float64 sums within the bound derived in tests/loglik_case.py), the bits it promises,
NaN containment, `l2hmc_chain_stats_exp` against `l2hmc_chain_stats` of the exponentiated history, and the fused routes of
`psis.loo_from_log_lik` / `psis.psis` / `psis.relative_eff_from_log_lik` against the numpy route within the gates of the case
file.  Every shape is named there."""
import numpy as np
import pytest

from tests import lik_stats_case as ls
from tests import loglik_case as lk

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check_raw(ll, lens, got, want_pos=True):
    """`got` of `lk.device_raw` against `lk.select_exact` and `lk.sum_bounds`; returns the worst sum error over its bound."""
    from l2hmc_amd._pareto import loo_tail_len
    S, n = ll.shape
    eff = np.full(n, loo_tail_len(S), dtype=np.int64) if lens is None else lens
    ex = lk.select_exact(ll, eff)
    assert got["flag"] == 0
    assert np.array_equal(_bits(got["cutoff"]), _bits(ex["cutoff"])) and np.array_equal(_bits(got["top"]), _bits(ex["top"]))
    assert np.array_equal(got["n_tail"], ex["n_tail"]) and np.all(got["n_tail"] <= eff)
    stride = got["tail"].shape[1]
    for i in range(n):
        L = int(ex["n_tail"][i])
        assert np.all(np.isposinf(got["tail"][i, L:])), i
        k = lk.keys(got["tail"][i, :L])
        if want_pos:
            assert np.all(got["tail_pos"][i, L:] == -1), i
            assert sorted(zip(k.tolist(), got["tail_pos"][i, :L].tolist())) == ex["pairs"][i], i
        else:
            assert sorted(k.tolist()) == [p[0] for p in ex["pairs"][i]], i
    assert stride == (eff.max() if lens is not None else loo_tail_len(S))
    ref, bound = lk.sum_bounds(ll, ex)
    with np.errstate(all="ignore"):
        worst = float(np.max(np.abs(got["sums"] - ref) / bound))
    assert np.all(np.abs(got["sums"] - ref) <= bound), worst
    return worst


@pytest.mark.parametrize("S,n", lk.GPU_SHAPES)
def test_raw_output_is_the_exact_selection(S, n):
    """One tail length (tail_len_col = NULL) and per-column lengths that include 0, 1, 4, 5 and S // 5, the latter once more
    without tail_pos; column 0 has the tie block at its cutoff."""
    ll = lk.matrix(S, n)
    lens = lk.lengths_for(S, n)
    w0 = _check_raw(ll, None, lk.device_raw(ll))
    w1 = _check_raw(ll, lens, lk.device_raw(ll, lens))
    _check_raw(ll, lens, lk.device_raw(ll, lens, want_pos=False), want_pos=False)
    print("(%d, %d) worst sum error / bound: %.3g (one length), %.3g (per column)" % (S, n, w0, w1))


def test_signed_zeros_at_the_cutoff():
    """-0 sorts before +0: with the cutoff at +0 the -0 below it is in the tail, with the cutoff at -0 the +0 above it is not."""
    S, M = 70, 14
    rng = np.random.RandomState(5)
    ll = np.empty((S, 2), dtype=np.float32)
    for j, zeros_from in enumerate((M - 1, M)):               # ranks of (-0, +0): (13, 14) and (14, 15)
        col = np.concatenate([-1.0 - rng.rand(zeros_from), [-0.0, 0.0], 1.0 + rng.rand(S - zeros_from - 2)]).astype(np.float32)
        ll[:, j] = col[rng.permutation(S)]
    lens = np.array([M, M], dtype=np.int64)
    got = lk.device_raw(ll, lens)
    _check_raw(ll, lens, got)
    assert np.array_equal(got["n_tail"], [M, M])
    assert _bits(got["cutoff"]).tolist() == [0x00000000, 0x80000000]
    assert np.signbit(got["tail"][0, :M]).all() and (got["tail"][0, :M] == 0).sum() == 1 and (got["tail"][1, :M] == 0).sum() == 0


def test_bits_do_not_depend_on_the_call():
    """Two calls give identical bits; columns [a, b) alone equal the same columns inside one call; tail_len_col = NULL equals an
    explicit array of equal lengths; 512 columns equal their two halves."""
    from l2hmc_amd._pareto import loo_tail_len
    for S, n, a, b in ((4099, 65, 7, 40), (65609, 3, 1, 2), (70, 512, 256, 512)):
        ll = lk.matrix(S, n)
        lens = lk.lengths_for(S, n)
        one, two = lk.device_raw(ll, lens), lk.device_raw(ll, lens)
        part = lk.device_raw(ll[:, a:b], lens[a:b], explicit_stride=int(lens.max()))
        head = lk.device_raw(ll[:, :a], lens[:a], explicit_stride=int(lens.max()))
        for k in ("cutoff", "top", "n_tail"):
            assert np.array_equal(_bits(one[k]), _bits(two[k])) and np.array_equal(_bits(one[k][a:b]), _bits(part[k])), k
            assert np.array_equal(_bits(one[k][:a]), _bits(head[k])), k
        assert np.array_equal(_bits(one["sums"]), _bits(two["sums"]))
        assert np.array_equal(_bits(one["sums"][:, a:b]), _bits(part["sums"])) and np.array_equal(_bits(one["sums"][:, :a]), _bits(head["sums"]))
        for i in range(a, b):
            L = int(one["n_tail"][i])
            pairs = lambda g, j: sorted(zip(_bits(g["tail"][j, :L]).tolist(), g["tail_pos"][j, :L].tolist()))  # noqa: E731
            assert pairs(one, i) == pairs(two, i) == pairs(part, i - a), i
        M = loo_tail_len(S)
        null, explicit = lk.device_raw(ll), lk.device_raw(ll, np.full(n, M, dtype=np.int64))
        for k in ("cutoff", "top", "n_tail", "sums"):
            assert np.array_equal(_bits(null[k]), _bits(explicit[k])), k
        assert np.array_equal(np.sort(_bits(null["tail"]), axis=1), np.sort(_bits(explicit["tail"]), axis=1))


def test_a_nan_stays_in_its_column():
    """One NaN in one column of three: that column's top and sums are NaN (and its finished numbers), its cutoff, n_tail and
    tail are those of its numbers; the other columns keep the bits they have without it."""
    import torch
    from l2hmc_amd import psis
    S, n = 4099, 3
    ll = lk.matrix(S, n)
    clean = lk.device_raw(ll)
    bad = ll.copy()
    bad[1234, 1] = np.nan
    got = lk.device_raw(bad)
    ex = lk.select_exact(bad, np.full(n, clean["tail"].shape[1], dtype=np.int64))
    assert np.isnan(got["top"][1]) and np.all(np.isnan(got["sums"][:, 1])) and got["flag"] == 0
    assert np.array_equal(_bits(got["cutoff"]), _bits(ex["cutoff"])) and np.array_equal(got["n_tail"], ex["n_tail"])
    assert not np.isnan(got["tail"]).any()
    for k in ("cutoff", "top", "n_tail", "sums"):
        assert np.array_equal(_bits(got[k][..., [0, 2]]), _bits(clean[k][..., [0, 2]])), k
    a = psis.loo_from_log_lik(torch.as_tensor(bad).cuda(), select="fused", r_eff=np.ones(n))
    b = psis.loo_from_log_lik(torch.as_tensor(ll).cuda(), select="fused", r_eff=np.ones(n))
    for k in ("khat", "elpd_loo_i", "lppd_i", "n_eff", "mcse_elpd_loo_i"):
        assert np.isnan(a[k][1]) and np.array_equal(_bits(a[k][[0, 2]]), _bits(b[k][[0, 2]])), k
    p = psis.psis(torch.as_tensor(-bad).cuda(), select="fused")
    assert np.isnan(p.khat[1]) and np.isnan(p.n_eff[1]) and np.all(np.isfinite(p.khat[[0, 2]]))


def test_minus_inf_draws_follow_the_table_of_non_finite_cutoffs():
    """`minus_inf_matrix` (70, 3): two -inf in column 1 are tail members under a finite cutoff, twenty in column 2 make the
    cutoff -inf, the tail empty and body and body_sq NaN (csrc/loglik_tails.hip, the table of its header).  The raw outputs are
    the exact selection, with the draws, and the sums lie inside the repaired `sum_bounds` (NaN exactly where the reference
    is); the finished numbers share the NaN pattern of the numpy route (khat and elpd_loo_i NaN in both columns) and column 0
    stays within the gates."""
    import torch
    from l2hmc_amd import psis
    from l2hmc_amd._pareto import loo_tail_len
    ll = lk.minus_inf_matrix()
    S, n = ll.shape
    M = loo_tail_len(S)
    for lens in (None, lk.lengths_for(S, n), np.array([M, 1, M - 1], dtype=np.int64)):
        got = lk.device_raw(ll, lens)
        eff = np.full(n, M, dtype=np.int64) if lens is None else lens
        ex = lk.select_exact(ll, eff)
        assert got["flag"] == 0
        assert np.array_equal(_bits(got["cutoff"]), _bits(ex["cutoff"])) and np.array_equal(_bits(got["top"]), _bits(ex["top"]))
        assert np.array_equal(got["n_tail"], ex["n_tail"])
        for i in range(n):
            L = int(ex["n_tail"][i])
            assert np.all(np.isposinf(got["tail"][i, L:])) and np.all(got["tail_pos"][i, L:] == -1), i
            assert sorted(zip(lk.keys(got["tail"][i, :L]).tolist(), got["tail_pos"][i, :L].tolist())) == ex["pairs"][i], i
        ref, bound = lk.sum_bounds(ll, ex)
        assert lk.sums_within(got["sums"], ref, bound), (got["sums"], ref, bound)
        if lens is None:
            assert np.isfinite(got["cutoff"][1]) and got["n_tail"][1] == M and np.isneginf(got["tail"][1]).sum() == 2
            assert np.isneginf(got["cutoff"][2]) and got["n_tail"][2] == 0 and np.isfinite(got["top"][2])
            assert np.isnan(got["sums"][:2, 2]).all() and np.isfinite(got["sums"][2, 2]) and np.all(np.isfinite(got["sums"][:, :2]))
    gk, ge, gn, gm = lk.gate(S)
    for r in (None, np.ones(n)):
        a, b = psis.loo_from_log_lik(torch.as_tensor(ll).cuda(), r_eff=r, select="fused"), psis.loo_from_log_lik(ll, r_eff=r)
        keys = ("khat", "elpd_loo_i", "lppd_i") + (("n_eff", "mcse_elpd_loo_i") if r is not None else ())
        for k in keys:
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (k, a[k], b[k])
        assert np.isnan(b.khat[1:]).all() and np.isnan(b.elpd_loo_i[1:]).all() and np.array_equal(a.n_tail, b.n_tail)
        assert abs(a.khat[0] - b.khat[0]) <= gk and abs(a.elpd_loo_i[0] - b.elpd_loo_i[0]) <= ge
        assert np.all(np.abs(a.lppd_i - b.lppd_i) <= ge)
        if r is not None:
            assert _rel(a.n_eff, b.n_eff)[0] <= gn and _rel(a.mcse_elpd_loo_i, b.mcse_elpd_loo_i)[0] <= gm


@pytest.mark.parametrize("fixture", [ls.FIXTURES[0], ls.FIXTURES[2], ls.FIXTURES[8]])
def test_chain_stats_exp_against_the_exponentiated_history(fixture):
    """`l2hmc_chain_stats_exp(X, shift)` against `l2hmc_chain_stats` of Y = exp(X - shift) formed in float64 torch and rounded to
    float32 once: within the raw-sum bounds of lik_stats_case with e = 2^-24 y per value (one float32 rounding of a
    double-precision exp that may differ in its last place from torch's)."""
    import torch
    M, N, d, rho, max_lag, split = fixture
    ll32 = lk.ar1_log_lik(fixture)[1]
    X = torch.as_tensor(ll32).cuda()
    shift = X.reshape(M * N, -1).amax(dim=0).to(torch.float64).contiguous()
    Y = torch.exp(X.to(torch.float64) - shift).to(torch.float32).contiguous()
    got = lk.device_chain_stats(X, max_lag, split, shift)
    ref = lk.device_chain_stats(Y, max_lag, split)
    print("%s bits equal: mean %s m2 %s G %s" % ((fixture,) + tuple(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, ref))))
    y = ls.series_of(Y.cpu().numpy().astype(np.float64), split)
    e = ls.EPS * y
    se2 = (e * e).sum(axis=0)
    bm2 = 2.0 * np.sqrt(ref[1] * se2) + se2
    assert np.all(np.abs(got[0] - ref[0]) <= e.mean(axis=0))
    assert np.all(np.abs(got[1] - ref[1]) <= bm2)
    assert np.all(np.abs(got[2] - ref[2]) <= (bm2.sum(axis=0) + 64 * ls.EPS * ref[2][:, 0])[:, None])


def _rel(a, b):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a) / np.asarray(b) - 1.0)


def _agree(got, ref, S, mc):
    gk, ge, gn, gm = lk.gate(S)
    for k in ("n_tail", "tail_len", "n_draws", "n_rows", "n_bad", "n_above_threshold", "n_underflow") + (("tail_len_row", "n_reff_nan") if mc else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(np.isfinite(got.khat), np.isfinite(ref.khat))
    f = np.isfinite(ref.khat)
    fig = [float(np.max(np.abs(got.khat[f] - ref.khat[f]), initial=0.0)), float(np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i))),
           float(np.max(np.abs(got.lppd_i - ref.lppd_i)))]
    assert fig[0] <= gk and fig[1] <= ge and fig[2] <= ge, fig
    if mc:
        fig += [float(np.max(_rel(got.n_eff, ref.n_eff))), float(np.max(_rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i)))]
        assert fig[3] <= gn and fig[4] <= gm, fig
        assert np.isnan(got.mcse_elpd_loo) == np.isnan(ref.mcse_elpd_loo)
    return fig


@pytest.mark.parametrize("S,n", lk.FINISH_SHAPES)
def test_fused_routes_match_the_numpy_route(S, n):
    """`loo_from_log_lik(select="fused")` and `psis(select="fused")`, with and without r_eff, against the numpy route on the same
    float32 matrix: the integer fields equal, the others within the gates; the wide matrix equals its two halves bit for bit."""
    import torch
    from l2hmc_amd import psis
    ll = lk.matrix(S, n)
    dev = torch.as_tensor(ll).cuda()
    gk, ge, gn, _ = lk.gate(S)
    for r in (None, lk.r_eff_for(n)):
        got = psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        ref = psis.loo_from_log_lik(ll, r_eff=r)
        print("(%d, %d) r_eff %s:" % (S, n, r is not None), " ".join("%.2g" % v for v in _agree(got, ref, S, r is not None)))
        p, q = psis.psis(-dev, r_eff=r, select="fused"), psis.psis(-ll, r_eff=r)
        assert np.array_equal(p.n_tail, q.n_tail) and p.tail_len == q.tail_len and np.array_equal(np.isfinite(p.khat), np.isfinite(q.khat))
        f = np.isfinite(q.khat)
        assert np.max(np.abs(p.khat[f] - q.khat[f]), initial=0.0) <= gk
        for key in ("n_bad", "n_above_threshold", "n_draws") + (("tail_len_row", "r_eff") if r is not None else ()):
            assert np.array_equal(p[key], q[key]), key
        assert p.log_weights.is_cuda and np.max(np.abs(p.log_weights.cpu().numpy() - q.log_weights)) <= ge
        assert np.max(_rel(p.n_eff, q.n_eff)) <= gn and np.max(np.abs(p.log_sum - q.log_sum)) <= ge
        k = psis.psis(-dev, weights=False, r_eff=r, select="fused")         # (its own sort: no positions are gathered)
        assert np.max(np.abs(k.khat[f] - q.khat[f]), initial=0.0) <= gk and np.array_equal(np.isfinite(k.khat), f)
        assert np.array_equal(k.n_tail, q.n_tail) and "log_weights" not in k
        if n == 1:                                              # one set of weights: (S,) in, (S,) out
            one, ref1 = psis.psis(-dev[:, 0], r_eff=r, select="fused"), psis.psis(-ll[:, 0], r_eff=r)
            assert tuple(one.log_weights.shape) == (S,) and np.max(np.abs(one.log_weights.cpu().numpy() - ref1.log_weights)) <= ge
            assert np.array_equal(one.n_tail, ref1.n_tail) and np.max(np.abs(one.khat[f] - ref1.khat[f]), initial=0.0) <= gk
            assert np.max(_rel(one.n_eff, ref1.n_eff)) <= gn
        if (S, n) == lk.WIDE:
            halves = [psis.loo_from_log_lik(dev[:, a:b].contiguous(), r_eff=None if r is None else r[a:b], select="fused")
                      for a, b in ((0, 256), (256, 513))]
            for key in ("khat", "elpd_loo_i", "lppd_i", "n_tail") + (("n_eff", "mcse_elpd_loo_i") if r is not None else ()):
                assert np.array_equal(_bits(got[key].astype(np.float64)), _bits(np.concatenate([h[key] for h in halves]).astype(np.float64))), key
    topk = psis.loo_from_log_lik(dev)                            # the default route keeps serving the same matrix
    fused = psis.loo_from_log_lik(dev, select="fused")
    assert np.array_equal(topk.n_tail, fused.n_tail) and np.max(np.abs(topk.elpd_loo_i - fused.elpd_loo_i)) <= ge


def test_a_column_does_not_depend_on_its_group_on_the_device():
    """With per-column tail lengths (184 .. 496 at S = 4099) the columns [32, 65) alone give the bits they have inside the whole
    call, whose tail stride is another: `loo_from_log_lik(select="fused")` and `psis(select="fused")`."""
    import torch
    from l2hmc_amd import psis
    S, n, a = lk.GROUP_CASE
    dev = torch.as_tensor(lk.matrix(S, n)).cuda()
    r = lk.r_eff_for(n)
    lens = lk.tail_lengths(r, S)
    assert lens[a:].max() < lens.max()
    part_ll = dev[:, a:].contiguous()
    whole, part = psis.loo_from_log_lik(dev, r_eff=r, select="fused"), psis.loo_from_log_lik(part_ll, r_eff=r[a:], select="fused")
    for k in ("khat", "elpd_loo_i", "lppd_i", "n_eff", "mcse_elpd_loo_i", "n_tail", "tail_len_row"):
        assert np.array_equal(whole[k][a:], part[k]), k
    pw, pp = psis.psis(-dev, r_eff=r, select="fused"), psis.psis(-part_ll, r_eff=r[a:], select="fused")
    for k in ("khat", "n_eff", "log_sum", "n_tail"):
        assert np.array_equal(pw[k][a:], pp[k]), k
    assert torch.equal(pw.log_weights[:, a:], pp.log_weights)


def test_a_nan_cutoff_gathers_every_number_as_the_numpy_route_counts():
    """A column with fewer than M + 1 numbers: the cutoff is a NaN, n_tail counts every number on both routes, the column's
    finished numbers are NaN and the other columns are served."""
    import torch
    from l2hmc_amd import psis
    few = lk.matrix(70, 3)
    few[5:, 1] = np.nan
    got = psis.loo_from_log_lik(torch.as_tensor(few).cuda(), r_eff=np.ones(3), select="fused")
    ref = psis.loo_from_log_lik(few, r_eff=np.ones(3))
    assert np.array_equal(got.n_tail, ref.n_tail) and got.n_tail[1] == 5
    assert np.isnan(got.khat[1]) and np.isnan(got.elpd_loo_i[1]) and np.all(np.isfinite(got.elpd_loo_i[[0, 2]]))


@pytest.mark.parametrize("fixture", lk.AR1_FIXTURES[:3])
def test_auto_relative_eff_on_a_device_history(fixture):
    """`relative_eff_from_log_lik` of a float32 device history against the numpy route: within K_REFF delta_i on the rows away
    from a truncation boundary; `loo_from_log_lik(r_eff="auto", select="fused")` equals the call with that r_eff given, and
    agrees with the numpy route given the same r_eff."""
    import torch
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split = fixture
    _, ll32, W, X, _ = lk.ar1_log_lik(fixture)
    dev = torch.as_tensor(ll32).cuda()
    _, near, _ = ls.sensitivity(fixture)
    keep = ~near
    di, _ = ls.delta(W, X)
    e = psis.relative_eff_from_log_lik(dev, max_lag=max_lag, split=split)
    ref = psis.relative_eff_from_log_lik(ll32, max_lag=max_lag, split=split)
    worst = float(np.max((_rel(e.r_eff, ref.r_eff) / (ls.K_REFF * di))[keep]))
    print("%s r_eff worst relative error / (K_REFF delta_i) %.3g" % (fixture, worst))
    assert worst <= 1.0 and np.array_equal(e.truncated[keep], ref.truncated[keep]) and e.n_nan == 0
    auto = psis.loo_from_log_lik(dev, r_eff="auto", select="fused", max_lag=max_lag, split=split)
    given = psis.loo_from_log_lik(dev, r_eff=e.r_eff, select="fused")
    for k in ("r_eff", "elpd_loo_i", "khat", "n_eff", "mcse_elpd_loo_i"):
        assert np.array_equal(_bits(auto[k]), _bits(given[k])), k
    print(" ".join("%.2g" % v for v in _agree(auto, psis.loo_from_log_lik(ll32, r_eff=e.r_eff), M * N, True)))


def test_refusals_on_the_device():
    """A float64 device matrix with select="fused" is refused and told of "topk"; `topk` with r_eff is told of "fused"."""
    import torch
    from l2hmc_amd import psis
    ll = torch.as_tensor(lk.matrix(70, 3)).cuda()
    for fn in (psis.loo_from_log_lik, psis.psis):
        with pytest.raises(ValueError, match='select="topk"'):
            fn(ll.double(), select="fused")
        with pytest.raises(ValueError, match='select="fused"'):
            fn(ll, r_eff=np.ones(3))
