"""GPU: the PSIS kernels (csrc/psis.hip behind `l2hmc_psis_smooth`) against the float64 numpy finish of the same tails, the
device routes of `psis` / `loo_from_log_lik` against their numpy forms on the same float32 matrix, and `loo(finish="kernel")`
against `finish="torch"` and the numpy finish of the same device tails.

Inputs of the kernel tests are tails built directly in numpy (tests/psis_case.py `tails`: GPD quantiles of shape k_true in
{-0.3, 0, 0.3, 0.7, 1.2} laid on the float32 grid of logits) -- no draws, no sampler.  Shapes (`psis_case.KERNEL_CASES`): the
profile kernel's workgroup is 256 threads = 4 waves that stride the tail by 256 and carry 8 theta each, so L = 63 / 64 / 65
and 255 / 256 / 257 are its wave and workgroup boundaries; L = 0, 1, 4 are not fitted, 5 and 6 the smallest fits; M = 769,
6072, 21 467 with 3 rows each (176 theta in 22 blocks at the last); one row; 300 rows at M = 64 (more workgroups than CUs);
tail_len = 0; 65 536 and 65 539 rows at M = 5 -- both sides of the only branch of the plan, the row loop
(tests/test_psis_cpu.py pins every shape to its plan by `l2hmc_psis_plan`).

Gates (tests/psis_case.py `gate`; nothing from the kernel): 100 x the disagreement of two float64 host references measured on
the CPU at tail lengths up to M, at most 1e-9, for khat and for elpd_loo_i.  The selection of `psis` is exact (`torch.topk` on
the float32 values), so only this float64 gate applies there too."""
import numpy as np
import pytest
import torch

from tests import loo_case as lc
from tests import psis_case as pc

pytestmark = pytest.mark.gpu
_REF = {}


def _dev(a):
    return torch.as_tensor(a).cuda()


def _dev_dict(raw):
    return {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in raw.items()}


def _bits(a):
    return (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).tobytes()


def _case(name):
    """The raw dict, its numpy finish and the numpy `smooth_tails` of one kernel case: computed once."""
    if name not in _REF:
        from l2hmc_amd import predictive, psis
        M, rows = pc.KERNEL_CASES[name]
        raw = pc.tails(M, rows, seed=M + len(rows))
        lam, L, lam_c = pc.lam_of(raw)
        _REF[name] = (M, raw, predictive.loo_finish(raw), (lam, L, lam_c), psis.smooth_tails(lam, L, lam_c, weights=True))
    return _REF[name]


def _within(what, got, ref, gate):
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(got[~fin], ref[~fin], equal_nan=True), what
    worst = float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0
    print("%s: |kernel - numpy| %.3g, gate %.3g, share %.3g" % (what, worst, gate, worst / gate if gate else 0.0))
    return worst <= gate


@pytest.mark.parametrize("name", list(pc.KERNEL_CASES))
def test_kernel_finish_matches_the_numpy_finish_of_the_same_tails(name):
    """khat and elpd_loo_i of `loo_finish(finish="kernel")` within the gates of the float64 numpy finish; n_tail, n_bad and
    n_above_threshold equal; `smooth_tails` on the same tails: omega in slot order within the elpd gate of numpy's, -inf in
    the dead slots (which hold NaN on the way in: never read), `out` bit for bit the same with and without `weights`, and two
    calls identical."""
    from l2hmc_amd import predictive, psis
    M, raw, ref, (lam, L, lam_c), (rk, rw, rwl, romega) = _case(name)
    gk, ge = pc.gate(M)
    got = predictive.loo_finish(_dev_dict(raw), finish="kernel")
    ok_k = _within("%s khat" % name, got.khat, ref.khat, gk)
    ok_e = _within("%s elpd_loo_i" % name, got.elpd_loo_i, ref.elpd_loo_i, ge)
    assert ok_k and ok_e
    assert np.array_equal(got.n_tail, ref.n_tail) and got.n_bad == ref.n_bad and got.n_above_threshold == ref.n_above_threshold
    assert np.array_equal(got.lppd_i, ref.lppd_i) or np.max(np.abs(got.lppd_i - ref.lppd_i)) <= 1e-14
    lam_d, L_d, c_d = _dev(lam), _dev(L), _dev(lam_c)
    k, w, wl, omega = psis.smooth_tails(lam_d, L_d, c_d, weights=True)
    assert omega.shape == (len(L), M) and omega.dtype == torch.float64
    assert _within("%s smooth_tails khat" % name, k.cpu().numpy(), rk, gk)
    assert _within("%s lse_w" % name, w.cpu().numpy(), rw, ge) and _within("%s lse_wl" % name, wl.cpu().numpy(), rwl, ge)
    assert _within("%s omega" % name, omega.cpu().numpy(), romega, ge)
    bare = psis.smooth_tails(lam_d, L_d, c_d)
    again = psis.smooth_tails(lam_d, L_d, c_d, weights=True)
    for a, b, c in zip((k, w, wl), bare, again):
        assert _bits(a) == _bits(b) == _bits(c)
    assert _bits(omega) == _bits(again[3])


@pytest.mark.parametrize("name,a,b", [("wave_boundary", 2, 5), ("more_workgroups_than_cus", 130, 131), ("m769", 1, 3)])
def test_rows_of_a_call_equal_the_same_rows_alone(name, a, b):
    from l2hmc_amd import psis
    lam, L, lam_c = (_dev(v) for v in _case(name)[3])
    whole = psis.smooth_tails(lam, L, lam_c, weights=True)
    part = psis.smooth_tails(lam[a:b], L[a:b], lam_c[a:b], weights=True)
    for x, y in zip(whole, part):
        assert _bits(x[a:b]) == _bits(y)


@pytest.mark.parametrize("n_rows", [65536, 65539])
def test_both_sides_of_the_row_loop(n_rows):
    """The grid holds at most 65536 workgroups along the rows; further rows are taken in a loop.  Seven distinct rows at M = 5
    (L = 0, 1, 4, 5 and three more fits) tiled to n_rows: every row has the bits of its copy in a call of the seven alone."""
    from l2hmc_amd import psis
    rows = [(0, 0.0), (1, 0.3), (4, 0.7), (5, 1.2), (5, -0.3), (5, 0.0), (5, 0.7)]
    lam, L, lam_c = (_dev(v) for v in pc.lam_of(pc.tails(5, rows, seed=7)))
    base = psis.smooth_tails(lam, L, lam_c, weights=True)
    reps = -(-n_rows // 7)
    big = psis.smooth_tails(lam.repeat(reps, 1)[:n_rows], L.repeat(reps)[:n_rows], lam_c.repeat(reps)[:n_rows], weights=True)
    for x, y in zip(base, big):
        want = x.repeat(reps, *([1] * (x.dim() - 1)))[:n_rows]
        assert y.shape == want.shape and torch.equal(y.view(torch.int64), want.view(torch.int64))
    assert np.all(np.isfinite(base[0].cpu().numpy()[3:])) and np.all(base[0].cpu().numpy()[:3] == np.inf)


def test_tail_len_zero():
    from l2hmc_amd import psis
    lam = torch.empty((2, 0), dtype=torch.float64, device="cuda")
    k, w, wl, omega = psis.smooth_tails(lam, _dev(np.zeros(2, dtype=np.int64)), _dev(np.array([0.3, -1.0])), weights=True)
    assert np.all(k.cpu().numpy() == np.inf) and np.all(w.cpu().numpy() == -np.inf) and np.all(wl.cpu().numpy() == -np.inf)
    assert omega.shape == (2, 0)


def test_degenerate_rows():
    """Every ratio equal to the cutoff's (every x = 0: the fit is not finite -> khat = +inf and the raw weights), lam_c =
    lam_max over a descending tail (likewise), and every ratio equal above the cutoff (every x equal: whatever the numpy form
    gives, within the gate)."""
    from l2hmc_amd import psis
    lam = np.full((3, 8), 1.5)
    lam[1] = np.linspace(3.0, 1.0, 8)
    L, lam_c = np.array([8, 8, 8], dtype=np.int64), np.array([1.5, 3.0, 0.5])
    ref = psis.smooth_tails(lam, L, lam_c, weights=True)
    got = [v.cpu().numpy() for v in psis.smooth_tails(_dev(lam), _dev(L), _dev(lam_c), weights=True)]
    gk, ge = pc.gate(8)
    assert np.all(got[0][:2] == np.inf) and np.all(ref[0][:2] == np.inf)
    assert np.array_equal(got[3][:2], lam[:2] - lam[:2, :1])                    # the raw weights, exactly
    assert abs(got[1][0] - np.log(8.0)) <= ge and abs(got[2][0] - (np.log(8.0) - 1.5)) <= ge
    for what, g, r, gate in (("khat", got[0], ref[0], gk), ("lse_w", got[1], ref[1], ge), ("lse_wl", got[2], ref[2], ge),
                             ("omega", got[3], ref[3], ge)):
        assert _within("degenerate " + what, g, r, gate)


def test_one_nan_in_one_row_of_three():
    from l2hmc_amd import psis
    lam, L, lam_c = _case("wave_boundary")[3]
    lam, L, lam_c = lam[:3].copy(), L[:3], lam_c[:3]
    clean = psis.smooth_tails(_dev(lam), _dev(L), _dev(lam_c))
    lam[1, 7] = np.nan
    bad = psis.smooth_tails(_dev(lam), _dev(L), _dev(lam_c))
    for c, b in zip(clean, bad):
        c, b = c.cpu().numpy(), b.cpu().numpy()
        assert np.isnan(b[1]) and not np.isnan(c[1])
        assert c[0].tobytes() == b[0].tobytes() and c[2].tobytes() == b[2].tobytes()


def test_an_n_tail_beyond_tail_len_is_an_error():
    from l2hmc_amd import psis
    lam, L, lam_c = _case("smallest_fits")[3]
    with pytest.raises(RuntimeError, match="n_tail"):
        psis.smooth_tails(_dev(lam), _dev(np.array([5, 7, 6], dtype=np.int64)), _dev(lam_c))
    psis.smooth_tails(_dev(lam), _dev(L), _dev(lam_c))                          # the next call is clean again


@pytest.mark.parametrize("S,n,d", lc.FIXTURES + [(70, 35, 5), (4, 3, 2)])
def test_loo_finish_kernel_against_torch_and_numpy_on_the_same_device_tails(S, n, d):
    """khat and elpd_loo_i of `finish="kernel"` within the gate of the numpy finish of the same device tails, and within that
    plus the torch finish's own gate (loo_case.FINISH_*: set at these tail lengths) of `finish="torch"`; n_bad,
    n_above_threshold and n_tail equal; `loo`, `loo_finish(loo_tails)` and the model method agree bit for bit."""
    from l2hmc_amd import LogisticRegression, predictive
    W, X, y = lc.case(S, n, d)
    M = lc.tail_len(S)
    t = predictive.loo_tails(_dev(W), X, y)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in t.items()}
    ker, tor, ref = predictive.loo_finish(t, finish="kernel"), predictive.loo_finish(t), predictive.loo_finish(host)
    gk, ge = pc.gate(M)
    ok = [_within("(%d, %d, %d) khat vs numpy" % (S, n, d), ker.khat, ref.khat, gk),
          _within("(%d, %d, %d) elpd vs numpy" % (S, n, d), ker.elpd_loo_i, ref.elpd_loo_i, ge),
          _within("(%d, %d, %d) khat vs torch" % (S, n, d), ker.khat, tor.khat, gk + lc.FINISH_KHAT),
          _within("(%d, %d, %d) elpd vs torch" % (S, n, d), ker.elpd_loo_i, tor.elpd_loo_i, ge + lc.FINISH_ELPD)]
    assert all(ok)
    for other in (tor, ref):
        assert np.array_equal(ker.n_tail, other.n_tail) and ker.n_bad == other.n_bad
        assert ker.n_above_threshold == other.n_above_threshold and np.max(np.abs(ker.lppd_i - other.lppd_i)) <= 1e-14
    whole = predictive.loo(_dev(W), X, y, finish="kernel")
    model = LogisticRegression(X, y).loo(_dev(W), finish="kernel")
    for k in ("khat", "elpd_loo_i", "n_tail"):
        assert np.array_equal(whole[k], ker[k]) and np.array_equal(model[k], ker[k]), k


def test_loo_finish_kernel_on_the_constant_history_and_in_row_groups():
    """All draws identical: L = 0 on every row, khat = +inf, elpd_loo_i = ll -- as the other finishes have it.  Row groups of
    `loo(finish="kernel")` give the bits of one group."""
    from l2hmc_amd import predictive
    W, X, y = lc.case(300, 50, 128)
    const = lc.degenerate("constant", W)
    ker, tor = predictive.loo(_dev(const), X, y, finish="kernel"), predictive.loo(_dev(const), X, y)
    assert np.all(ker.n_tail == 0) and np.all(ker.khat == np.inf) and ker.n_bad == 50 == tor.n_bad
    assert np.max(np.abs(ker.elpd_loo_i - tor.elpd_loo_i)) <= pc.gate(lc.tail_len(300))[1] + lc.FINISH_ELPD
    ll = -np.logaddexp(0.0, -lc.signed_logits(const[:1], X, y)[0])
    assert np.max(np.abs(ker.elpd_loo_i - ll)) <= 32 * lc.EPS
    one = predictive.loo(_dev(W), X, y, finish="kernel")
    many = predictive.loo(_dev(W), X, y, finish="kernel", max_tail_bytes=4 * lc.tail_len(300) * 13)
    assert np.array_equal(one.elpd_loo_i, many.elpd_loo_i) and np.array_equal(one.khat, many.khat)


@pytest.mark.parametrize("S,n", [(25, 3), (4099, 7), (65609, 4)])
def test_device_psis_and_loo_from_log_lik_match_their_numpy_forms(S, n):
    """On the same float32 matrix, column 0 with a tie block at its cutoff (L < M): n_tail equal; khat and elpd_loo_i within
    the gates; log_weights, log_sum and lppd_i within the elpd gate (the same float64 sums, the same tree); a 1-d input;
    row groups against one call, bit for bit."""
    from l2hmc_amd import psis
    ll = pc.log_lik_case(S, n, seed=S, ties=True)
    M = lc.tail_len(S)
    gk, ge = pc.gate(M)
    lld = _dev(ll)
    ref, got = psis.psis(-ll), psis.psis(-lld)
    assert np.array_equal(got.n_tail, ref.n_tail) and got.n_tail[0] < M and got.tail_len == M and got.n_draws == S
    assert got.log_weights.is_cuda and got.log_weights.dtype == torch.float64 and got.log_weights.shape == (S, n)
    assert _within("(%d, %d) psis khat" % (S, n), got.khat, ref.khat, gk)
    assert _within("(%d, %d) log_weights" % (S, n), got.log_weights.cpu().numpy(), ref.log_weights, ge)
    assert _within("(%d, %d) log_sum" % (S, n), got.log_sum, ref.log_sum, ge)
    assert _within("(%d, %d) log n_eff" % (S, n), np.log(got.n_eff), np.log(ref.n_eff), 2 * ge)
    assert got.n_bad == ref.n_bad and got.n_above_threshold == ref.n_above_threshold
    rl, gl = psis.loo_from_log_lik(ll), psis.loo_from_log_lik(lld)
    ok = [_within("(%d, %d) loo khat" % (S, n), gl.khat, rl.khat, gk), _within("(%d, %d) elpd_loo_i" % (S, n), gl.elpd_loo_i, rl.elpd_loo_i, ge),
          _within("(%d, %d) lppd_i" % (S, n), gl.lppd_i, rl.lppd_i, ge)]
    assert all(ok) and np.array_equal(gl.n_tail, rl.n_tail) and gl.n_bad == rl.n_bad
    one = psis.psis(-lld[:, 1])
    assert one.log_weights.shape == (S,) and _bits(one.log_weights) == _bits(got.log_weights[:, 1].contiguous())
    assert one.khat[0] == got.khat[1] and one.log_sum[0] == got.log_sum[1] and one.n_eff[0] == got.n_eff[1]
    parts = [psis.loo_from_log_lik(lld[:, a:b]) for a, b in ((0, 1), (1, n - 1), (n - 1, n))]
    for k in ("khat", "elpd_loo_i", "lppd_i", "n_tail"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), gl[k]), k
    assert np.array_equal(psis.psis(-lld, weights=False).khat, got.khat)


def test_end_to_end_poisson_regression_as_a_torch_energy():
    """A Poisson regression written as a plain torch callable (n = 40, d = 3), sampled by HMC on the slow path, 256 chains x 40
    proposals: `loo_from_log_lik` of its device log-likelihood matrix is finite, elpd_loo < lppd, and equals the numpy form
    on the same float32 matrix within the gates."""
    from l2hmc_amd import Dynamics, psis, sample_chain
    X, y = pc.poisson_case()
    Xd, yd = _dev(X), _dev(y)
    lfact = torch.lgamma(yd + 1.0)

    def energy(w):
        eta = w @ Xd.T
        return (torch.exp(eta) - yd[None, :] * eta).sum(1) + 0.5 * (w * w).sum(1)

    dyn = Dynamics(3, energy, T=5, eps=0.05, hmc=True, device=Xd.device)
    x0 = _dev((0.1 * np.random.RandomState(5).randn(256, 3)).astype(np.float32))
    _, _, hist = sample_chain(x0, dyn, 40, seed=1, record=True)
    W = hist[10:].reshape(-1, 3)
    eta = W @ Xd.T
    ll = yd[None, :] * eta - torch.exp(eta) - lfact[None, :]                    # (7680, 40) float32, on the device
    got, ref = psis.loo_from_log_lik(ll), psis.loo_from_log_lik(ll.cpu().numpy())
    assert got.n_draws == 30 * 256 and got.n_rows == 40 and got.tail_len == lc.tail_len(7680) == 263
    assert np.all(np.isfinite(got.elpd_loo_i)) and np.all(np.isfinite(got.khat)) and got.elpd_loo < got.lppd
    gk, ge = pc.gate(263)                                    # (the references' disagreement at the measured lengths up to 263)
    ok = [_within("poisson khat", got.khat, ref.khat, gk), _within("poisson elpd_loo_i", got.elpd_loo_i, ref.elpd_loo_i, ge)]
    assert all(ok) and np.array_equal(got.n_tail, ref.n_tail)
    print("poisson: elpd_loo %.3f  lppd %.3f  p_loo %.3f  max khat %.3f" % (got.elpd_loo, got.lppd, got.p_loo, got.khat.max()))
