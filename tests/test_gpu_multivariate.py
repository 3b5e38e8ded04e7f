"""GPU: the raw moments on the float64 matrix pipe (csrc/moment_sums.hip behind `l2hmc_moment_sums`) and
`multivariate.covariance` / `multi_ess` on top of them, against the two-pass restatement of tests/multivariate_case.py.

Shapes: the smallest at which the plan can go wrong -- "E" (d = 1, 5 chains: one tile with 15 dead columns, a ragged chain
group of 1), "B" (d = 2, 257 steps: the batch rows start at row 1), "F" (d = 17, 77 chains: a second tile that is nearly empty,
N d odd, 19 groups and one chain), "C" (d = 25, 400 000 draws: long accumulations, many waves, every block reduces), "G"
(d = 100: 7 tiles, 28 tile pairs in three panels, 4 live columns in the last tile), "A" (means -20 .. 3 at sd 0.05 .. 2: the
cancellation of the raw moments).

Gates.  Sums: |got - ref| <= 1e-10 sqrt(raw_ii raw_jj), raw = the diagonal of `cross` (of `batch_cross` for the batch sums;
for the vector sums the other factor is the count, the raw moment of the constant 1): 2^-53 x the longest chain of additions
(<= the 4e5 rows of "C") = 4.4e-11.  A float64 one-pass evaluation in another summation order sits at <= 4e-5 of that gate on
every fixture, float32 accumulation cannot meet it.  multi_ess: relative error <= 2 B,
B = (sum |P^-1_ij| g_ij + sum |Q^-1_ij| g'_ij) / d the first-order bound of the log-determinants under the entry gates g, g';
the factor 2 covers the second-order terms.  Computed from the restatement, 2 B is 8.9e-8 (E), 1.8e-9 (B), 5.3e-10 (F, the
smallest), 1.9e-6 (C, cond(Sigma) = 3.7e4), 3.4e-8 (G) and 2.1e-6 (A, the largest: the raw moments are 3600 times the
centred ones).

Measured on the MI355X (profiles/multivariate_accuracy.txt, written by tools/multivariate_accuracy.py) -- the worst
deviation of the sums as a fraction of their gate, and of multi_ess, relative:
    E 1.6e-6, 6.6e-14;  B 5.6e-6, 7.2e-16;  F 7.8e-6, 1.5e-16;  C 2.3e-4, 9.8e-12;  G 7.4e-6, 1.3e-15;  A 4.1e-5, 1.5e-12.

Those fixtures have at most 1000 chains (63 chunks of 16: one chunk per block) and T = 1, 2 or 7 tiles; the histories of
multivariate_case.PLAN_FIXTURES reach the rest of the plan under the same gates (their figures are in the same file)."""
import numpy as np
import pytest
import torch

from tests import multivariate_case as mc
from tests import quantiles_case as qc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
FIXTURES = ["E", "B", "F", "C", "G", "A"]
_REF, _DEV = {}, {}


def _reference(name, batch):
    if (name, batch) not in _REF:
        _REF[(name, batch)] = mc.reference(mc.history(name), batch)
    return _REF[(name, batch)]


def _device(name):
    if name not in _DEV:
        _DEV[name] = torch.as_tensor(np.array(mc.history(name))).cuda()
    return _DEV[name]


def _check_sums(got, ref, keep=None):
    """The four sums against the raw form of the restatement, under the gates; returns the worst fraction of a gate."""
    worst = 0.0
    for vec, mat, count in (("sum", "cross", ref["n_draws"]), ("batch_sum", "batch_cross", ref.get("n_batches"))):
        if got[mat] is None:
            continue
        gv, gm = mc.sum_gates(np.diag(ref[mat]), count)
        v, m = got[vec].cpu().numpy(), got[mat].cpu().numpy()
        assert np.array_equal(m.view(np.int64), m.T.copy().view(np.int64)), mat       # bitwise symmetric
        ev, em = np.abs(v - ref[vec]), np.abs(m - ref[mat])
        if keep is not None:
            ev, gv, em, gm = ev[keep], gv[keep], em[np.ix_(keep, keep)], gm[np.ix_(keep, keep)]
        assert np.all(ev <= gv), (vec, np.max(ev / np.where(gv > 0, gv, 1)))
        assert np.all(em <= gm), (mat, np.max(em / np.where(gm > 0, gm, 1)))
        worst = max(worst, float(np.max(ev / np.where(gv > 0, gv, 1.0))), float(np.max(em / np.where(gm > 0, gm, 1.0))))
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_sums_match_the_restatement(name):
    from l2hmc_amd import multivariate
    X = mc.history(name)
    Xd = _device(name)
    for batch in (mc.default_batch(X.shape[0]), 0):
        got = multivariate.moment_sums(Xd, batch)
        ref = _reference(name, batch)
        assert got["n_draws"] == ref["n_draws"] and got["n_batches"] == ref.get("n_batches", 0)
        worst = _check_sums(got, ref)
        print("fixture %s batch %d: worst deviation %.3g of the gate" % (name, batch, worst))


def mess_bound(ref):
    """B of the module docstring, from the restatement alone."""
    _, g = mc.sum_gates(np.diag(ref["cross"]), ref["n_draws"])
    _, gb = mc.sum_gates(np.diag(ref["batch_cross"]), ref["n_batches"])
    d = ref["P"].shape[0]
    return (np.sum(np.abs(np.linalg.inv(ref["P"])) * g) + np.sum(np.abs(np.linalg.inv(ref["Q"])) * gb)) / d


@pytest.mark.parametrize("name", FIXTURES)
def test_multi_ess_matches_the_restatement(name):
    from l2hmc_amd import diagnostics, multivariate
    X = mc.history(name)
    ref = _reference(name, mc.default_batch(X.shape[0]))
    got = multivariate.multi_ess(_device(name))
    assert isinstance(got, diagnostics.Summary) and not got.degenerate.any()
    assert (got.n_draws, got.n_batches, got.batch_size) == (ref["n_draws"], ref["n_batches"], ref["batch_size"])
    B = mess_bound(ref)
    e = abs(got.multi_ess - ref["multi_ess"]) / ref["multi_ess"]
    print("fixture %s: multi_ess %.6g, relative deviation %.3g, bound 2 B = %.3g, cond(Sigma) %.3g" % (
        name, got.multi_ess, e, 2 * B, np.linalg.cond(ref["cov_asymptotic"])))
    assert e <= 2 * B
    _, g = mc.sum_gates(np.diag(ref["cross"]), ref["n_draws"])
    # P = cross - sum sum^T / n: the entry gate, and twice it for the two factors of the mean term
    assert np.all(np.abs(got.cov - ref["cov"]) * (ref["n_draws"] - 1) <= 3 * g)
    assert np.all(np.abs(got.corr - got.cov / np.outer(got.sd, got.sd)) <= 1e-15) and np.all(np.diag(got.corr) == 1.0)
    assert np.all(np.abs(got.sd - ref["sd"]) * (ref["n_draws"] - 1) * 2 * ref["sd"] <= 3 * np.diag(g) * (1 + 1e-6))
    assert np.array_equal(got.cov, got.cov.T) and np.array_equal(got.cov_asymptotic, got.cov_asymptotic.T)


PLAN_NAMES = sorted(mc.PLAN_FIXTURES)


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_sums_and_multi_ess_across_chunks_and_panels(name):
    """The branches of the plan the fixtures above never take (tests/multivariate_case.py states each history's plan,
    tests/test_multivariate_cpu.py pins it): more than 256 chunks of 16 chains, so that a block keeps its accumulators, column
    sums and batch sums across two chunks while the batch in progress, and the leading rows that belong to no batch, start
    again in the second; T = 3 and T = 4 tiles in one panel; the off-diagonal panels <4, 1>, <4, 2>, <4, 4> and second diagonal
    panels of 1, 2 and 4 tiles; d = 64, 65, 128.  Every coordinate has its own phi, mean and sd.  The gates are those of
    `test_sums_match_the_restatement` and `test_multi_ess_matches_the_restatement`, unchanged: every history has fewer than the
    4e5 rows the sum gate allows for, and more batches than coordinates."""
    from l2hmc_amd import multivariate
    steps, chains, d, batch, _ = mc.PLAN_FIXTURES[name]
    X = mc.history(name)
    Xd = _device(name)
    assert X.shape == (steps, chains, d) and steps * chains < 4e5 and (steps // batch) * chains > d
    for b in (batch, 0):
        got = multivariate.moment_sums(Xd, b)
        ref = _reference(name, b)
        assert got["n_draws"] == ref["n_draws"] and got["n_batches"] == ref.get("n_batches", 0)
        worst = _check_sums(got, ref)
        print("fixture %s batch %d: worst deviation %.3g of the gate" % (name, b, worst))
    ref = _reference(name, batch)
    got = multivariate.multi_ess(Xd, batch)
    assert not got.degenerate.any()
    assert (got.n_draws, got.n_batches, got.batch_size) == (ref["n_draws"], ref["n_batches"], batch)
    B = mess_bound(ref)
    e = abs(got.multi_ess - ref["multi_ess"]) / ref["multi_ess"]
    print("fixture %s: multi_ess %.6g, relative deviation %.3g, bound 2 B = %.3g, cond(Sigma) %.3g" % (
        name, got.multi_ess, e, 2 * B, np.linalg.cond(ref["cov_asymptotic"])))
    assert e <= 2 * B
    _, g = mc.sum_gates(np.diag(ref["cross"]), ref["n_draws"])
    assert np.all(np.abs(got.cov - ref["cov"]) * (ref["n_draws"] - 1) <= 3 * g)
    assert np.array_equal(got.cov, got.cov.T) and np.array_equal(got.cov_asymptotic, got.cov_asymptotic.T)


def test_two_calls_across_chunks_give_identical_bits():
    """"two-chunks-d17" (4113 chains, 258 chunks over 256 blocks), with batches."""
    from l2hmc_amd import multivariate
    Xd = _device("two-chunks-d17")
    first = multivariate.moment_sums(Xd, 4)
    torch.empty(1 << 24, device="cuda").normal_()                       # 64 MB of other work, another workspace address
    second = multivariate.moment_sums(Xd.clone(), 4)
    for key in ("sum", "cross", "batch_sum", "batch_cross"):
        assert torch.equal(first[key].view(torch.int64), second[key].view(torch.int64)), key


def test_batch_size_one_and_whole_chain():
    """batch_size = 1: Sigma is Lambda and no row is dropped, multi_ess = n_draws; batch_size = steps: one batch per chain."""
    from l2hmc_amd import multivariate
    Xd = _device("B")
    one = multivariate.multi_ess(Xd, 1)
    assert one.n_batches == one.n_draws == 257 * 200 and abs(one.multi_ess / one.n_draws - 1) <= 1e-9
    whole = multivariate.multi_ess(Xd, 257)
    ref = _reference("B", 257)
    assert whole.n_batches == 200 and abs(whole.multi_ess - ref["multi_ess"]) <= 2 * mess_bound(ref) * ref["multi_ess"]


def test_rotation_invariance_and_theory():
    """The AR(1) history "R" (1024 x 64 x 4, phi = 0, .3, .5, .6) and a fixed orthogonal matrix: multi_ess of the rotated
    history, rounded to float32, equals that of the original to 1e-6 (1.8e-8 in numpy; ess_batch meanwhile moves: its
    minimum is 16 200 before and 23 716 after); and mESS / n is within 5 sqrt(2 / (A d)) = 7.8 % of exp(-mean_k log tau_b(phi_k)), b = 32,
    A = 2048 (numpy: -1.45 %)."""
    from l2hmc_amd import multivariate
    X = mc.history("R")
    R = mc.rotation()
    Y = (X.astype(np.float64) @ R.T).astype(np.float32)
    a = multivariate.multi_ess(_device("R"))
    b = multivariate.multi_ess(torch.as_tensor(Y).cuda())
    print("multi_ess %.6g, rotated %.6g; min ess_batch %.0f -> %.0f" % (a.multi_ess, b.multi_ess, a.ess_batch.min(),
                                                                         b.ess_batch.min()))
    assert abs(a.multi_ess - b.multi_ess) / a.multi_ess <= 1e-6
    assert abs(a.ess_batch.min() - b.ess_batch.min()) / a.ess_batch.min() > 0.25
    assert (a.batch_size, a.n_batches) == (32, 2048)
    theory = np.exp(-np.mean(np.log(mc.theory_tau_batch(mc.ROTATION_HISTORY[2], 32))))
    dev = a.multi_ess / a.n_draws / theory - 1
    print("mESS / n = %.5f, theory %.5f: %+.2f %%" % (a.multi_ess / a.n_draws, theory, 100 * dev))
    assert abs(dev) <= 5 * np.sqrt(2.0 / (2048 * 4))


def test_views_and_other_dtypes_are_not_misread():
    from l2hmc_amd import _ffi, multivariate
    X = mc.history("F")
    Xd = _device("F")
    want = multivariate.multi_ess(Xd)

    def same(Y, ref=want, fn=multivariate.multi_ess):
        got = fn(Y)
        return all(np.array_equal(got[k], ref[k]) for k in ("mean", "cov", "corr") + (("multi_ess", "cov_asymptotic")
                                                                                      if "multi_ess" in ref else ()))
    assert same(Xd.double())                                            # float64 on the device: values are float32-exact
    assert same(Xd.permute(1, 0, 2).contiguous().permute(1, 0, 2))      # the same history, chain-major in memory
    big = torch.zeros((X.shape[0] + 9,) + X.shape[1:], device="cuda")
    big[9:] = Xd
    assert same(big[9:])                                                # a burn-in slice is contiguous: read in place
    ref = _reference("F", 0)
    _, g = mc.sum_gates(np.diag(ref["cross"]), ref["n_draws"])
    for cov in (multivariate.covariance(Xd), multivariate.covariance(Xd.reshape(-1, X.shape[2]))):     # and the (S, d) view
        assert "multi_ess" not in cov and cov.n_draws == ref["n_draws"]
        assert np.all(np.abs(cov.cov - ref["cov"]) * (ref["n_draws"] - 1) <= 3 * g)      # another plan (no batches): the gate
    _check_sums(multivariate.moment_sums(Xd.reshape(-1, X.shape[2])), ref)                 # (S, d): read as (S / c, c, d)
    for view, host in ((Xd[:, ::2], X[:, ::2]), (Xd[:, :, 3:9], X[:, :, 3:9])):
        assert same(view, multivariate.multi_ess(view.contiguous()))
        r = mc.reference(host, mc.default_batch(X.shape[0]))
        got = multivariate.multi_ess(view)
        assert abs(got.multi_ess - r["multi_ess"]) <= 2 * mess_bound(r) * r["multi_ess"]
    first = multivariate.moment_sums(Xd, 9)
    torch.empty(1 << 24, device="cuda").normal_()                       # 64 MB of other work, another workspace address
    second = multivariate.moment_sums(Xd.clone(), 9)
    for key in ("sum", "cross", "batch_sum", "batch_cross"):
        assert torch.equal(first[key].view(torch.int64), second[key].view(torch.int64)), key
    wide = torch.zeros((8, 4, 129), device="cuda")
    with pytest.raises(ValueError, match="128"):
        multivariate.covariance(wide)
    L = _ffi.lib()
    out = torch.empty(129 * 129, dtype=torch.float64, device="cuda")
    assert L.l2hmc_moment_sums(wide.data_ptr(), 8, 4, 129, 0, out.data_ptr(), out.data_ptr(), None, None, out.data_ptr(),
                               None) == -1
    assert b"d <= 128" in L.l2hmc_last_error()


def test_non_finite_and_constant_coordinates_stay_alone():
    """quantiles_case.adversarial(): NaN in coordinate 11, +-inf in 4, constants in 1 and 3."""
    from l2hmc_amd import multivariate
    X, _ = qc.adversarial()
    Xd = torch.as_tensor(X).cuda()
    batch = mc.default_batch(X.shape[0])
    clean = np.array([k for k in range(17) if k not in (4, 11)])
    ref = mc.reference(X[:, :, clean], batch)                                      # the other 15, restated on their own
    got = multivariate.moment_sums(Xd, batch)
    for key in ("sum", "batch_sum"):
        v = got[key].cpu().numpy()
        assert np.array_equal(np.flatnonzero(~np.isfinite(v)), [4, 11]), key
    for key in ("cross", "batch_cross"):
        m = got[key].cpu().numpy()
        bad = np.zeros((17, 17), dtype=bool)
        bad[[4, 11], :] = True
        bad[:, [4, 11]] = True
        assert np.array_equal(~np.isfinite(m), bad), key                            # its own rows and columns, nothing else
    idx = torch.as_tensor(clean).cuda()
    sub = {k: (got[k][idx][:, idx] if got[k].dim() == 2 else got[k][idx]) for k in ("sum", "cross", "batch_sum", "batch_cross")}
    print("adversarial: worst deviation %.3g of the gate" % _check_sums(sub, ref))
    s = multivariate.multi_ess(Xd)
    assert np.array_equal(np.flatnonzero(s.degenerate), [1, 3, 4, 11]) and np.isnan(s.multi_ess)
    bad = np.zeros((17, 17), dtype=bool)
    bad[[4, 11], :] = True
    bad[:, [4, 11]] = True
    assert np.array_equal(np.isnan(s.cov), bad) and np.all(np.isfinite(s.cov[~bad]))
    deg = bad.copy()
    deg[[1, 3], :] = True
    deg[:, [1, 3]] = True
    assert np.array_equal(np.isnan(s.corr), deg)
    _, g = mc.sum_gates(np.diag(ref["cross"]), ref["n_draws"])
    assert np.all(np.abs(s.cov[np.ix_(clean, clean)] - ref["cov"]) * (ref["n_draws"] - 1) <= 3 * g)


SIGMA_STAR_VAR = np.linspace(0.25, 4.0, 8)


def test_end_to_end_on_a_known_dense_gaussian():
    """HMC on a zero-mean 8-dimensional Gaussian with Sigma* = R diag(0.25 .. 4) R^T, R a fixed rotation (no entry of Sigma*
    is zero), eps = 0.6 and 3 leapfrog steps: the accept rate measured on the MI355X is 0.885 (inside the 0.6 .. 0.9 asked
    for; the same step size and length as the quantile test's diagonal target, which has the same spectrum).  512 chains,
    400 proposals, 100 discarded: every entry of `cov` within 5 standard errors of Sigma*,
    se_ij = sqrt((S_ii S_jj + S_ij^2) / min ess_batch) -- measured: 1.46 se at worst, multi_ess 95 472 of 153 600 draws."""
    from l2hmc_amd import Dynamics, multi_ess, sample_chain
    from l2hmc_amd import distributions as D
    R = np.linalg.qr(np.random.RandomState(5).randn(8, 8))[0]
    S = (R * SIGMA_STAR_VAR) @ R.T
    S = (S + S.T) / 2
    assert np.abs(S[~np.eye(8, dtype=bool)]).min() > 1e-3
    e = D.Gaussian(np.zeros(8), S).get_energy_function()
    dyn = Dynamics(8, e, T=3, eps=0.6, hmc=True)
    dyn.eps_override = 0.6
    x0 = torch.as_tensor((np.random.RandomState(0).randn(512, 8) @ np.linalg.cholesky(S).T).astype(np.float32)).cuda()
    _, p, hist = sample_chain(x0, dyn, 400, record=True, seed=3)
    accept = float(p.mean())
    s = multi_ess(hist[100:])
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / s.ess_batch.min())
    z = np.abs(s.cov - S) / se
    print("accept rate %.3f; worst cov error %.2f se; multi_ess %.0f of %d; ess_batch %.0f .. %.0f" % (
        accept, z.max(), s.multi_ess, s.n_draws, s.ess_batch.min(), s.ess_batch.max()))
    assert 0.6 <= accept <= 0.9
    assert s.n_draws == 300 * 512 and (s.batch_size, s.n_batches) == (17, 17 * 512) and not s.degenerate.any()
    assert np.all(z < 5)
    assert np.isfinite(s.multi_ess) and s.multi_ess > 0
