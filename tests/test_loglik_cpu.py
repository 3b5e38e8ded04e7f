"""CPU: PSIS-LOO of any likelihood with relative efficiencies -- the numpy route of `psis.loo_from_log_lik(r_eff=)`,
`psis.psis(r_eff=)` and `psis.relative_eff_from_log_lik` against the restatement of tests/loglik_case.py and against the
logistic-regression route of `predictive` (two independent host routes), the refusals, the argument validation of
`l2hmc_loglik_tails` and `l2hmc_chain_stats_exp`, and the compiler's listing of the new kernels."""
import os
import re

import numpy as np
import pytest

from tests import lik_stats_case as ls
from tests import loglik_case as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a) / np.asarray(b) - 1.0)


def _khat_diff(a, b):
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), (a, b)
    both = np.isfinite(a)
    return float(np.max(np.abs(a[both] - b[both]), initial=0.0))


@pytest.mark.parametrize("S,n", lk.FINISH_SHAPES)
def test_numpy_route_matches_the_restatement(S, n):
    """With one tail length and with r_eff: n_tail and tail_len_row equal, khat, elpd_loo_i, lppd_i, n_eff, mcse within the
    gates; `psis(r_eff=)` gives the restatement's log weights and the same n_eff as `loo_from_log_lik`."""
    from l2hmc_amd import diagnostics, psis
    from l2hmc_amd._pareto import loo_tail_len
    ll = lk.matrix(S, n).astype(np.float64)
    gk, ge, gn, gm = lk.gate(S)
    for r in (None, lk.r_eff_for(n)):
        got = psis.loo_from_log_lik(ll, r_eff=r)
        lens = np.full(n, loo_tail_len(S)) if r is None else lk.tail_lengths(r, S)
        ref = lk.restate(ll, lens, r)
        assert isinstance(got, diagnostics.Summary) and np.array_equal(got.n_tail, ref["n_tail"])
        dk, de = _khat_diff(got.khat, ref["khat"]), float(np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])))
        print("(%d, %d) r_eff %s: khat %.2g elpd %.2g" % (S, n, r is not None, dk, de))
        assert dk <= gk and de <= ge and np.max(np.abs(got.lppd_i - ref["lppd_i"])) <= ge
        assert got.tail_len == lens.max() and got.n_draws == S and got.n_rows == n
        if r is None:
            assert "n_eff" not in got and "mcse_elpd_loo" not in got
            continue
        assert np.array_equal(got.tail_len_row, lens) and np.array_equal(got.r_eff, r) and got.n_reff_nan == 0
        dn, dm = float(np.max(_rel(got.n_eff, ref["n_eff"]))), float(np.max(_rel(got.mcse_elpd_loo_i, ref["mcse"])))
        print("        n_eff %.2g mcse %.2g" % (dn, dm))
        assert dn <= gn and dm <= gm and got.min_n_eff == got.n_eff.min()
        total = np.sqrt(np.sum(got.mcse_elpd_loo_i ** 2))
        assert (np.isnan(got.mcse_elpd_loo) if np.any(got.khat > 0.7) else got.mcse_elpd_loo == total)
        ps = psis.psis(-ll, r_eff=r)
        assert np.array_equal(ps.n_tail, ref["n_tail"]) and np.array_equal(ps.tail_len_row, lens) and np.array_equal(ps.r_eff, r)
        assert _khat_diff(ps.khat, ref["khat"]) <= gk
        assert np.max(np.abs(ps.log_weights - ref["log_weights"])) <= ge and np.max(_rel(ps.n_eff, ref["n_eff"])) <= gn
        if n == 1:                                              # one set of weights: (S,) in, (S,) out
            flat = psis.psis(-ll[:, 0], r_eff=r)
            assert flat.log_weights.shape == (S,) and np.array_equal(flat.log_weights, ps.log_weights[:, 0])
            assert np.array_equal(flat.khat, ps.khat) and np.array_equal(flat.n_eff, ps.n_eff)
    same = psis.loo_from_log_lik(ll, r_eff=np.ones(n))          # r_eff = 1 is the uncorrelated tail length
    base = psis.loo_from_log_lik(ll)
    assert np.array_equal(same.n_tail, base.n_tail) and np.max(np.abs(same.elpd_loo_i - base.elpd_loo_i)) <= ge


@pytest.mark.parametrize("fixture", lk.AR1_FIXTURES)
def test_agrees_with_the_logistic_route_of_predictive(fixture):
    """`loo_from_log_lik(ll64, r_eff=r)` on the float64 logistic log-likelihood against `predictive.loo(W, X, y, r_eff=r)` on the
    host: tail_len_row and n_tail equal, khat, elpd_loo_i, n_eff and mcse within the gates; the history form gives the bits of
    the matrix form."""
    from l2hmc_amd import predictive, psis
    M, N, d, rho, max_lag, split = fixture
    ll, _, W, X, y = lk.ar1_log_lik(fixture)
    r = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split).r_eff
    a = predictive.loo(W, X, y, r_eff=r)
    b = psis.loo_from_log_lik(ll, r_eff=r)
    gk, ge, gn, gm = lk.gate(M * N)
    assert np.array_equal(a.tail_len_row, b.tail_len_row) and np.array_equal(a.n_tail, b.n_tail)
    fig = (_khat_diff(a.khat, b.khat), float(np.max(np.abs(a.elpd_loo_i - b.elpd_loo_i))), float(np.max(_rel(b.n_eff, a.n_eff))),
           float(np.max(_rel(b.mcse_elpd_loo_i, a.mcse_elpd_loo_i))))
    print("%s khat %.2g elpd %.2g n_eff %.2g mcse %.2g" % ((fixture,) + fig))
    assert fig[0] <= gk and fig[1] <= ge and fig[2] <= gn and fig[3] <= gm
    flat = psis.loo_from_log_lik(ll.reshape(M * N, -1), r_eff=r)
    assert np.array_equal(flat.elpd_loo_i, b.elpd_loo_i) and np.array_equal(flat.n_eff, b.n_eff)


@pytest.mark.parametrize("fixture", lk.AR1_FIXTURES)
def test_auto_relative_eff_agrees_with_predictive(fixture):
    """`relative_eff_from_log_lik` and r_eff="auto" on the history form against `predictive.relative_eff`: within K_REFF
    delta_i (relative) on the rows away from a truncation boundary, of which the fixtures have at most 10 %; inside the range
    each fixture was chosen for."""
    from l2hmc_amd import predictive, psis
    M, N, d, rho, max_lag, split = fixture
    ll, _, W, X, y = lk.ar1_log_lik(fixture)
    _, near, _ = ls.sensitivity(fixture)
    assert near.mean() <= ls.EXCLUDED_AT_MOST
    keep = ~near
    di, _ = ls.delta(W, X)
    ref = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
    got = psis.relative_eff_from_log_lik(ll, max_lag=max_lag, split=split)
    worst = float(np.max((_rel(got.r_eff, ref.r_eff) / (ls.K_REFF * di))[keep]))
    print("%s r_eff worst relative error / (K_REFF delta_i) %.3g" % (fixture, worst))
    assert worst <= 1.0 and np.array_equal(got.truncated[keep], ref.truncated[keep])
    lo, hi = ls.R_EFF_RANGE[fixture]
    assert 0.75 * lo <= got.r_eff.min() and got.r_eff.max() <= 1.25 * hi
    for k in ("n_draws", "n_steps", "n_chains", "max_lag", "n_nan"):
        assert got[k] == ref[k], k
    auto = psis.loo_from_log_lik(ll, r_eff="auto", max_lag=max_lag, split=split)
    assert np.array_equal(auto.r_eff, got.r_eff) and np.array_equal(auto.tail_len_row, predictive.tail_len_rows(got.r_eff, M * N))
    const = ll.copy()
    const[:, :, 0] = -0.5                                     # a constant column has no efficiency: NaN, counted, M_i as for 1
    e = psis.relative_eff_from_log_lik(const, max_lag=max_lag, split=split)
    assert np.isnan(e.r_eff[0]) and e.n_nan == 1 and np.array_equal(e.r_eff[1:], got.r_eff[1:])


def test_a_column_does_not_depend_on_its_group():
    """With per-column tail lengths (184 .. 496 at S = 4099) the columns [32, 65) alone give the bits they have inside the whole
    call, where the longest tail -- the stride of every sum over the slots -- is another: `loo_from_log_lik` and `psis`."""
    from l2hmc_amd import psis
    S, n, a = lk.GROUP_CASE
    ll = lk.matrix(S, n).astype(np.float64)
    r = lk.r_eff_for(n)
    lens = lk.tail_lengths(r, S)
    assert lens[a:].max() < lens.max()
    whole, part = psis.loo_from_log_lik(ll, r_eff=r), psis.loo_from_log_lik(ll[:, a:], r_eff=r[a:])
    for k in ("khat", "elpd_loo_i", "lppd_i", "n_eff", "mcse_elpd_loo_i", "n_tail", "tail_len_row"):
        assert np.array_equal(whole[k][a:], part[k]), k
    pw, pp = psis.psis(-ll, r_eff=r), psis.psis(-ll[:, a:], r_eff=r[a:])
    for k in ("khat", "n_eff", "log_sum", "n_tail"):
        assert np.array_equal(pw[k][a:], pp[k]), k
    assert np.array_equal(pw.log_weights[:, a:], pp.log_weights)


def test_one_order_for_signed_zeros_and_nan_cutoffs():
    """With r_eff every numpy route orders -0 before +0, as the device does: a (-0, +0) pair at ranks (13, 14) of the
    log-likelihoods with M = 14 puts the -0 in the tail (n_tail 14), at ranks (14, 15) it does not (the cutoff is the -0 and
    nothing equals it); `psis` of the negated column agrees.  A column with fewer than M + 1 numbers has a NaN cutoff and every
    number in its tail, as the kernel gathers it."""
    from l2hmc_amd import psis
    S, M = 70, 14
    r = np.array([9.0 * S / M ** 2])                         # 3 sqrt(S / r) = M
    assert lk.tail_lengths(r, S)[0] == M
    rng = np.random.RandomState(5)
    for zeros_from, want in ((M - 1, M), (M, M)):
        col = np.concatenate([-1.0 - rng.rand(zeros_from), [-0.0, 0.0], 1.0 + rng.rand(S - zeros_from - 2)])[rng.permutation(S)]
        assert psis.loo_from_log_lik(col[:, None], r_eff=r).n_tail[0] == want
        assert psis.psis(-col, r_eff=r).n_tail[0] == want
    plain = np.concatenate([-1.0 - rng.rand(M - 1), [0.0, 0.0], 1.0 + rng.rand(S - M - 1)])   # two +0: a tie at the cutoff
    assert psis.loo_from_log_lik(plain[:, None], r_eff=r).n_tail[0] == M - 1 == psis.psis(-plain, r_eff=r).n_tail[0]
    few = lk.matrix(S, 3).astype(np.float64)
    few[5:, 1] = np.nan
    s = psis.loo_from_log_lik(few, r_eff=np.ones(3))
    assert s.n_tail[1] == 5 and np.isnan(s.khat[1]) and np.isnan(s.elpd_loo_i[1]) and np.all(np.isfinite(s.elpd_loo_i[[0, 2]]))


def test_sum_bounds_of_columns_that_hold_minus_inf():
    """`loglik_case.sum_bounds`: a zero term adds a zero bound.  A 5 x 3 matrix with tail length 2: column 0 finite, column 1
    with one -inf (a tail member under a finite cutoff: its body terms are masked, its lik term is e^-inf = 0), column 2 with
    three -inf (the cutoff is -inf: the -inf draws outside the empty tail give e^(-inf + inf) = NaN in body and body_sq, and lik
    stays finite).  The finite column's bound is what the unrepaired expression gives, bit for bit.  The numpy route of
    `minus_inf_matrix` gives NaN khat and elpd_loo_i in both columns that hold a -inf, and serves the third."""
    from l2hmc_amd import psis
    ll = np.array([[-1.0, -2.0, -np.inf], [-3.0, -np.inf, -1.0], [-0.5, -0.25, -np.inf], [-2.0, -4.0, -np.inf], [-1.5, -1.0, -2.0]],
                  dtype=np.float32)
    lens = np.full(3, 2, dtype=np.int64)
    ex = lk.select_exact(ll, lens)
    assert ex["n_tail"].tolist() == [2, 2, 0] and np.isneginf(ex["cutoff"]).tolist() == [False, False, True]
    ref, bound = lk.sum_bounds(ll, ex)
    assert np.all(np.isfinite(ref[:, :2])) and np.all(np.isfinite(bound[:, :2])) and np.all(bound[:, :2] > 0)
    assert np.isnan(ref[:2, 2]).all() and np.isfinite(ref[2, 2]) and np.isfinite(bound[2, 2])
    ld = np.longdouble
    c, top, x = ld(ex["cutoff"][0]), ld(ex["top"][0]), ll[:, 0].astype(ld)
    out = ~ex["in_tail"][:, 0]
    u = ld(2.0) ** -52 + ld(np.finfo(ld).eps)
    want = [((np.exp(m * (c - x)) * (np.abs(c - x) + 2) * u)[out]).sum() + 5 * ld(2.0) ** -53 * np.exp(m * (c - x))[out].sum() for m in (1, 2)]
    want.append((np.exp(x - top) * (np.abs(x - top) + 2) * u).sum() + 5 * ld(2.0) ** -53 * np.exp(x - top).sum())
    assert np.array_equal(bound[:, 0], np.array(want).astype(np.float64))
    assert abs(ref[2, 1] - (1.0 + np.exp(-0.75) + np.exp(-1.75) + np.exp(-3.75))) <= bound[2, 1]
    assert lk.sums_within(ref, ref, bound) and not lk.sums_within(np.where(np.isnan(ref), 0.0, ref), ref, bound)
    big = lk.minus_inf_matrix()
    s = psis.loo_from_log_lik(big, r_eff=np.ones(3))
    for k in ("khat", "elpd_loo_i"):
        assert np.isnan(s[k][1:]).all() and np.isfinite(s[k][0]), k


def test_refusals():
    """A matrix with "auto", an unknown select or r_eff word, a wrong r_eff shape, the fused route on host data, and -- on a
    device-like input, refused before anything is touched -- `topk` with r_eff (names select="fused") and a float64 matrix with
    `fused` (names select="topk")."""
    import l2hmc_amd
    from l2hmc_amd import psis
    assert l2hmc_amd.relative_eff_from_log_lik is psis.relative_eff_from_log_lik and "relative_eff_from_log_lik" in l2hmc_amd.__all__
    ll = lk.matrix(70, 3).astype(np.float64)
    with pytest.raises(ValueError, match="history form"):
        psis.loo_from_log_lik(ll, r_eff="auto")
    with pytest.raises(ValueError, match="history"):
        psis.relative_eff_from_log_lik(ll)
    with pytest.raises(ValueError, match="auto"):
        psis.loo_from_log_lik(ll, r_eff="yes")
    for fn in (psis.loo_from_log_lik, psis.psis):
        with pytest.raises(ValueError, match="select"):
            fn(ll, select="sort")
        with pytest.raises(ValueError, match='select="topk"'):
            fn(ll.astype(np.float32), select="fused")           # host data
        with pytest.raises(ValueError, match="r_eff"):
            fn(ll, r_eff=np.ones(4))

    class DeviceLike:
        """what `is_device_tensor` is asked about: nothing else of it may be touched before the refusal"""
        def __init__(self, dtype):
            self.shape, self.dtype = (70, 3), dtype

    real = psis.is_device_tensor
    psis.is_device_tensor = lambda a: isinstance(a, DeviceLike) or real(a)
    try:
        for fn in (psis.loo_from_log_lik, psis.psis):
            with pytest.raises(ValueError, match='select="fused"'):
                fn(DeviceLike("torch.float32"), r_eff=np.ones(3))
            with pytest.raises(ValueError, match='select="topk"'):
                fn(DeviceLike("torch.float64"), select="fused")
    finally:
        psis.is_device_tensor = real


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the new entries (ABI version still 6); every L2HMC_ERR_ARG case of
    both is refused with a message before anything is launched; the workspace grows with the columns alone at fixed n_draws."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_loglik_tails_workspace_bytes", "l2hmc_loglik_tails", "l2hmc_chain_stats_exp"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws, tails = L.l2hmc_loglik_tails_workspace_bytes, L.l2hmc_loglik_tails
    assert ws(4099, 65) > 0 and ws(4099, 65) % 8 == 0 and ws(2, 1) > 0 and ws(4096000, 512) > 0
    # the segments depend on n_draws alone: 65 segments of 64 draws at 4099, 2048 at 131072, 2017 of 65 draws at 131073
    fixed = lambda n: (16 + 24 * n + (8 * n + 15) // 16 * 16 + 15) // 16 * 16 + L.l2hmc_order_stats_workspace_bytes(n, 2)  # noqa: E731
    for S, nseg in ((25, 1), (64, 1), (65, 2), (4099, 65), (65609, 1026), (131072, 2048), (131073, 2017), (4096000, 2048)):
        for n in (1, 3, 65, 512):
            assert ws(S, n) == fixed(n) + nseg * 3 * n * 8, (S, n)
    ok = 1 << 12                                             # an aligned non-NULL address: refused before it is touched

    def call(S=100, n=10, stride=20, ptrs=None, lens=ok):
        p = [ok] * 8 if ptrs is None else ptrs               # ll, cutoff, top, n_tail, tail, tail_pos, sums, workspace
        return tails(p[0], S, n, lens, stride, p[1], p[2], p[3], p[4], p[5], p[6], p[7], None)
    for kw, msg in ((dict(S=1), b"n_draws >= 2"), (dict(S=0), b"n_draws >= 2"), (dict(n=0), b"n_cols <= 512"),
                    (dict(n=513), b"n_cols <= 512"), (dict(S=(1 << 40) // 10 + 1), b"too large"), (dict(stride=-1), b"tail_stride"),
                    (dict(stride=100), b"tail_stride"), (dict(S=1 << 30, n=512, stride=(1 << 22) + 1), b"tail too large")):
        assert call(**kw) == -1 and msg in L.l2hmc_last_error(), (kw, L.l2hmc_last_error())
    for S, n in ((1, 10), (100, 0), (100, 513), ((1 << 40) + 1, 1)):
        assert ws(S, n) == -1
    for at in (0, 1, 2, 3, 4, 6, 7):                         # a required pointer NULL (tail_pos and tail_len_col may be)
        p = [ok] * 8
        p[at] = None
        assert call(ptrs=p) == -1 and b"required" in L.l2hmc_last_error(), at
    assert call(stride=0, ptrs=[ok, ok, ok, ok, None, None, ok, None]) == -1 and b"required" in L.l2hmc_last_error()
    for at, off in ((0, 2), (1, 2), (2, 2), (3, 4), (4, 2), (5, 4), (6, 4), (7, 8)):
        p = [ok] * 8
        p[at] = ok + off
        assert call(ptrs=p) == -1 and b"aligned" in L.l2hmc_last_error(), at
    assert call(lens=ok + 4) == -1 and b"aligned" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(call(S=1))
    # l2hmc_chain_stats_exp: the checks of l2hmc_chain_stats, and the shift is required
    cs = L.l2hmc_chain_stats_exp
    for (M, N, d, lag, split), msg in (((0, 4, 3, 1, 0), b">= 1"), ((8, 0, 3, 1, 0), b">= 1"), ((8, 4, 0, 1, 0), b">= 1"),
                                       ((8, 4, 513, 1, 0), b"d <= 512"), ((8, 4, 3, 1, 2), b"split"), ((3, 4, 3, 1, 0), b">= 4 steps"),
                                       ((8, 1, 3, 1, 0), b">= 2 chains"), ((7, 4, 3, 1, 1), b">= 4 steps"), ((8, 4, 3, 8, 0), b"max_lag"),
                                       ((8, 4, 3, -1, 0), b"max_lag"), ((8, (1 << 40) // 3 + 1, 3, 1, 0), b"too large")):
        assert cs(ok, M, N, d, lag, split, ok, ok, ok, ok, ok, None) == -1
        assert msg in L.l2hmc_last_error() and b"l2hmc_chain_stats_exp" in L.l2hmc_last_error(), ((M, N, d, lag, split), L.l2hmc_last_error())
    for at in range(6):
        p = [ok] * 6                                         # X, shift, mean, m2, G, workspace
        p[at] = None
        assert cs(p[0], 8, 4, 3, 1, 0, p[1], p[2], p[3], p[4], p[5], None) == -1 and b"required" in L.l2hmc_last_error(), at


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): the kernels of
    loglik_tails.s and the exp kernels of chain_stats.s use no scratch; the gather stays within the 128 registers (four waves per
    SIMD) its header states and has no LDS; the exp lag-sum kernel within the 256 of its two siblings."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    res = kr.resources()
    rows = res.get("loglik_tails.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    by = {k: (vg, sc) for k, vg, sc, _ in rows}
    assert {"loglik_init_kernel", "loglik_gather_kernel", "chunk_reduce_kernel", "radix_advance_kernel"} <= set(by), by
    header = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "loglik_tails.hip")).read()
    assert "at most 128 registers and no scratch" in header and "FLOAT64 ISSUE BOUND" in header
    for k, (vg, sc) in by.items():
        print("%-24s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0, (k, sc)
    assert by["loglik_gather_kernel"][0] <= 128
    asm = open(os.path.join(kr.ASM, "loglik_tails.s")).read()
    assert all(int(v) == 0 for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", asm))
    cs = {k: (vg, sc) for k, vg, sc, _ in res["chain_stats.s"]}
    for k in ("chain_moments_exp_kernel", "chain_lagsum_exp_kernel"):
        print("%-24s %4d registers, %d bytes of scratch" % ((k,) + cs[k]))
        assert cs[k][1] == 0 and cs[k][0] <= 256, (k, cs[k])
