"""CPU: PSIS of any log ratios -- the numpy paths of `l2hmc_amd.psis` against the row-at-a-time restatement of
tests/psis_case.py, `loo_from_log_lik` of the logistic log-likelihood matrix against `predictive.loo`, the split of
`predictive._loo_rows` against the bits of the commit before it, the `Summary` algebra, refusals, exports, the C ABI's argument
validation, the launch plan of every GPU test shape and the compiler's listing of the new unit."""
import os
import re

import numpy as np
import pytest

from tests import loo_case as lc
from tests import psis_case as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_GATE = 1e-10                                            # float64 against float64, another summation order (test_loo_cpu.py)


def _close(a, b, gate=HOST_GATE):
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], b[~fin], equal_nan=True)
    return not fin.any() or float(np.max(np.abs(a[fin] - b[fin]))) <= gate


@pytest.mark.parametrize("S,n", [(25, 3), (523, 5), (4099, 7)])
def test_numpy_psis_and_loo_match_the_restatement(S, n):
    """`psis(-ll)` and `loo_from_log_lik(ll)` on a float32 matrix with a tie block at column 0's cutoff: khat, log_weights,
    log_sum, log n_eff, elpd_loo_i and lppd_i within 1e-10 of the restatement, n_tail equal and shorter than M where the ties are."""
    from l2hmc_amd import psis
    ll = pc.log_lik_case(S, n, seed=S, ties=True)
    M = lc.tail_len(S)
    got, ref = psis.psis(-ll), pc.restate_psis(-ll)
    assert got.tail_len == M and got.n_draws == S and got.n_tail.dtype == np.int64
    assert np.array_equal(got.n_tail, ref["n_tail"]) and got.n_tail[0] < M and np.all(got.n_tail[1:] == M)
    assert got.log_weights.shape == (S, n) and got.log_weights.dtype == np.float64
    for k in ("khat", "log_weights", "log_sum"):
        assert _close(got[k], ref[k]), k
    assert _close(np.log(got.n_eff), np.log(ref["n_eff"]))
    assert np.all(got.log_weights <= 0.0) and np.all(got.log_weights.max(axis=0) <= 0.0)
    assert np.all(got.n_eff >= 1.0 - 1e-12) and np.all(got.n_eff <= S)
    loo, rl = psis.loo_from_log_lik(ll), pc.restate_loo(ll)
    for k in ("khat", "elpd_loo_i", "lppd_i"):
        assert _close(loo[k], rl[k]), k
    assert np.array_equal(loo.n_tail, rl["n_tail"]) and loo.tail_len == M and loo.n_rows == n
    # float64 input and a CPU tensor go the same way
    import torch
    assert np.array_equal(psis.psis(-ll.astype(np.float64)).khat, got.khat)
    assert np.array_equal(psis.psis(torch.as_tensor(-ll)).log_weights, got.log_weights)


def test_one_dimensional_input_and_weights_off():
    from l2hmc_amd import psis
    ll = pc.log_lik_case(523, 3, seed=9)
    two, one = psis.psis(-ll), psis.psis(-ll[:, 2])
    assert one.log_weights.shape == (523,) and one.khat.shape == (1,) and one.n_eff.shape == (1,)
    assert np.array_equal(one.log_weights, two.log_weights[:, 2]) and one.khat[0] == two.khat[2] and one.log_sum[0] == two.log_sum[2]
    bare = psis.psis(-ll, weights=False)
    assert np.array_equal(bare.khat, two.khat) and np.array_equal(bare.n_tail, two.n_tail)
    assert "log_weights" not in bare and "n_eff" not in bare and bare.n_bad == two.n_bad


def test_row_groups_concatenate_to_one_call_bit_for_bit():
    from l2hmc_amd import psis
    ll = pc.log_lik_case(4099, 7, seed=4099, ties=True)
    one = psis.loo_from_log_lik(ll)
    parts = [psis.loo_from_log_lik(ll[:, a:b]) for a, b in ((0, 3), (3, 4), (4, 7))]
    for k in ("khat", "elpd_loo_i", "lppd_i", "n_tail"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), one[k]), k
    ps = psis.psis(-ll)
    assert np.array_equal(np.concatenate([psis.psis(-ll[:, a:b]).log_weights for a, b in ((0, 3), (3, 7))], axis=1), ps.log_weights)


@pytest.mark.parametrize("S,n,d", [(37, 17, 3), (523, 33, 17), (300, 50, 128)])
def test_loo_from_log_lik_of_the_logistic_matrix_matches_predictive_loo(S, n, d):
    """The generic route on the (S, n) matrix ll = -softplus(-t) against the fused decomposition (tail / body) of
    `predictive.loo` on the same numpy draws: float64 both."""
    from l2hmc_amd import predictive, psis
    W, X, y = lc.case(S, n, d)
    t = lc.signed_logits(W, X, y)
    got, ref = psis.loo_from_log_lik(-np.logaddexp(0.0, -t)), predictive.loo(W, X, y)
    assert np.array_equal(got.n_tail, ref.n_tail) and got.tail_len == ref.tail_len and got.n_draws == S
    for k in ("khat", "elpd_loo_i", "lppd_i", "p_loo_i"):
        assert _close(got[k], ref[k]), k
    assert got.n_bad == ref.n_bad and got.n_above_threshold == ref.n_above_threshold and got.khat_threshold == ref.khat_threshold
    assert abs(got.elpd_loo - ref.elpd_loo) <= 1e-9 and abs(got.se - ref.se) <= 1e-9


def test_the_split_of_loo_rows_keeps_the_bits_of_the_commit_before_it():
    """`predictive.loo` on numpy draws, on `loo_case.FIXTURES` and the three degenerate histories: khat, elpd_loo_i, lppd_i,
    p_loo_i and n_tail bit for bit what the unsplit `_loo_rows` returned (tests/golden/psis/loo_numpy_before_split.npz, recorded
    from the parent commit)."""
    from l2hmc_amd import predictive
    gold = np.load(os.path.join(ROOT, "tests", "golden", "psis", "loo_numpy_before_split.npz"))
    cases = [("f%d_%d_%d" % s, lc.case(*s)) for s in lc.FIXTURES]
    W, X, y = lc.case(300, 50, 128)
    cases += [(kind, (lc.degenerate(kind, W), X, y)) for kind in ("twice", "half", "constant")]
    seen = 0
    for name, (W_, X_, y_) in cases:
        s = predictive.loo(W_, X_, y_)
        for k in ("khat", "elpd_loo_i", "lppd_i", "p_loo_i", "n_tail"):
            assert s[k].dtype == gold[name + "." + k].dtype and s[k].tobytes() == gold[name + "." + k].tobytes(), (name, k)
            seen += 1
    assert seen == len(gold.files) == 50


def test_smooth_tails_numpy_matches_the_restatement_and_the_degenerate_rows():
    """`smooth_tails` on prepared tails (NaN in the dead slots: never read) against `restate_tail`; omega in slot order, -inf in
    the dead slots.  Degenerate rows: L = 0 (-inf, -inf, khat = +inf), L < 5 (raw weights), every ratio equal to the cutoff's
    (x = 0: the fit is not finite -> khat = +inf and the raw weights, lse_w = log L), lam_c = lam_max, and one NaN in one row of
    three: that row NaN, the others bit for bit what they are without it."""
    from l2hmc_amd import psis
    M = 65
    rows = [(65, 0.7), (64, -0.3), (5, 0.0), (4, 0.3), (1, 1.2), (0, 0.0), (33, 1.2)]
    tl = [pc.tail(M, L, k, seed=3 + i) for i, (L, k) in enumerate(rows)]
    lam = np.stack([t["lam"] for t in tl])
    L = np.array([t["L"] for t in tl], dtype=np.int64)
    lam_c = np.array([t["lam_c"] for t in tl])
    khat, lse_w, lse_wl, omega = psis.smooth_tails(lam, L, lam_c, weights=True)
    three = psis.smooth_tails(lam, L, lam_c)
    assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (khat, lse_w, lse_wl)))
    for i, t in enumerate(tl):
        rk, ro, rw, rwl = pc.restate_tail(t["lam"], t["L"], t["lam_c"])
        assert _close(khat[i], rk) and _close(lse_w[i], rw) and _close(lse_wl[i], rwl), i
        assert _close(omega[i, :t["L"]], ro) and np.all(omega[i, t["L"]:] == -np.inf), i
    assert np.all(khat[[3, 4, 5]] == np.inf) and np.all(np.isfinite(khat[[0, 1, 2, 6]]))
    assert lse_w[5] == -np.inf and lse_wl[5] == -np.inf
    assert np.array_equal(omega[3, :4], lam[3, :4] - lam[3, 0])
    # x = 0 everywhere; lam_c = lam_max over a descending tail
    flat = np.full((2, 8), 1.5)
    flat[1] = np.linspace(3.0, 1.0, 8)
    k2, w2, wl2 = psis.smooth_tails(flat, np.array([8, 8]), np.array([1.5, 3.0]))
    assert np.all(k2 == np.inf) and abs(w2[0] - np.log(8.0)) <= 1e-15 and abs(wl2[0] - (np.log(8.0) - 1.5)) <= 1e-15
    assert abs(w2[1] - np.logaddexp.reduce(flat[1] - 3.0)) <= 1e-15
    # one NaN
    bad = lam[:3].copy()
    bad[1, 7] = np.nan
    kb, wb, wlb = psis.smooth_tails(bad, L[:3], lam_c[:3])
    assert np.isnan(kb[1]) and np.isnan(wb[1]) and np.isnan(wlb[1])
    for got, ref in ((kb, khat), (wb, lse_w), (wlb, lse_wl)):
        assert got[0].tobytes() == ref[0].tobytes() and got[2].tobytes() == ref[2].tobytes()


def test_summary_algebra():
    from l2hmc_amd import diagnostics, predictive, psis
    ll = pc.log_lik_case(523, 6, seed=1)
    s = psis.loo_from_log_lik(ll)
    assert isinstance(s, diagnostics.Summary)
    assert s.elpd_loo == float(s.elpd_loo_i.sum()) and s.p_loo == float(s.p_loo_i.sum()) and s.lppd == float(s.lppd_i.sum())
    assert s.looic == -2.0 * s.elpd_loo and np.array_equal(s.p_loo_i, s.lppd_i - s.elpd_loo_i)
    assert abs(s.se - np.sqrt(6 * s.elpd_loo_i.var(ddof=1))) <= 1e-12 * s.se
    assert np.all(s.p_loo_i > 0) and s.elpd_loo < s.lppd and s.n_underflow == 0
    p = psis.psis(-ll)
    assert isinstance(p, diagnostics.Summary)
    assert p.khat_threshold == lc.khat_threshold(523) == s.khat_threshold
    assert p.n_bad == int(np.sum(p.khat > 0.7)) and p.n_above_threshold == int(np.sum(p.khat > p.khat_threshold)) >= p.n_bad
    assert np.array_equal(p.khat, s.khat) and np.array_equal(p.n_tail, s.n_tail)
    w = p.log_weights - p.log_sum[None, :]                   # normalised
    assert np.max(np.abs(np.exp(w).sum(axis=0) - 1.0)) <= 1e-12
    assert np.max(np.abs(p.n_eff - 1.0 / np.square(np.exp(w)).sum(axis=0))) <= 1e-9 * 523
    # the body keeps its raw ratios, the tail never exceeds the largest raw one and keeps its order
    r = -ll.astype(np.float64)
    body = r <= np.sort(r, axis=0)[523 - p.tail_len - 1][None, :]
    assert np.array_equal(p.log_weights[body], (r - r.max(axis=0)[None, :])[body])
    for i in range(6):
        tail = ~body[:, i]
        assert np.all(np.diff(p.log_weights[tail, i][np.argsort(r[tail, i])]) >= 0.0)
    # S < 5: no tail at all, raw weights
    tiny = psis.psis(-ll[:4])
    assert tiny.tail_len == 0 and np.all(tiny.khat == np.inf) and np.all(tiny.n_tail == 0)
    assert np.array_equal(tiny.log_weights, r[:4] - r[:4].max(axis=0)[None, :])
    # a NaN makes its column NaN, quietly, and no other
    nan = ll.copy()
    nan[5, 2] = np.nan
    sn = psis.loo_from_log_lik(nan)
    assert np.isnan(sn.elpd_loo_i[2]) and np.isnan(sn.khat[2]) and np.array_equal(np.delete(sn.elpd_loo_i, 2), np.delete(s.elpd_loo_i, 2))
    assert predictive.loo_tail_len(523) == p.tail_len


def test_bad_arguments_raise_value_error():
    from l2hmc_amd import predictive, psis
    ll = pc.log_lik_case(40, 4, seed=2)
    for bad in (ll[None], ll[:0], ll[:, :0], np.float32(1.0)):
        with pytest.raises(ValueError):
            psis.psis(bad)
        with pytest.raises(ValueError):
            psis.loo_from_log_lik(bad)
    with pytest.raises(ValueError):
        psis.loo_from_log_lik(ll[:, 0])                      # one column per data row
    with pytest.raises(ValueError):
        psis.loo_from_log_lik(ll[:1])
    lam, L, c = np.zeros((3, 5)), np.array([5, 0, 2]), np.zeros(3)
    for args in ((lam[0], L, c), (lam[:0], L[:0], c[:0]), (lam, L[:2], c), (lam, L, c[:2]), (lam, np.array([6, 0, 0]), c),
                 (lam, np.array([-1, 0, 0]), c)):
        with pytest.raises(ValueError):
            psis.smooth_tails(*args)
    # finish="kernel" needs device tails, and says why
    W, X, y = lc.case(40, 6, 3)
    for call in (lambda: predictive.loo(W, X, y, finish="kernel"), lambda: predictive.loo_finish(predictive.loo_tails(W, X, y), finish="kernel")):
        with pytest.raises(ValueError, match="host data"):
            call()
    import l2hmc_amd
    with pytest.raises(ValueError, match="host data"):
        l2hmc_amd.LogisticRegression(X, y).loo(W, finish="kernel")
    with pytest.raises(ValueError, match='"torch" or "kernel"'):
        predictive.loo(W, X, y, finish="numpy")
    a, b = predictive.loo(W, X, y), predictive.loo(W, X, y, finish="torch")
    assert np.array_equal(a.elpd_loo_i, b.elpd_loo_i) and np.array_equal(a.khat, b.khat)


def test_exports():
    import l2hmc_amd
    from l2hmc_amd import psis
    assert l2hmc_amd.psis is psis and l2hmc_amd.loo_from_log_lik is psis.loo_from_log_lik
    assert "psis" in l2hmc_amd.__all__ and "loo_from_log_lik" in l2hmc_amd.__all__
    assert callable(psis.psis) and callable(psis.smooth_tails)


def test_abi_declares_binds_and_validates_without_gpu():
    """include/l2hmc.h, the library and `_ffi.SYMBOLS` agree on the three entries (ABI version still 6); every L2HMC_ERR_ARG
    case is refused with its message before anything is launched; tail_len = 0 is a valid shape."""
    import ctypes
    from l2hmc_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    L = _ffi.lib()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("l2hmc_psis_plan", "l2hmc_psis_workspace_bytes", "l2hmc_psis_smooth"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _ffi.SYMBOLS and hasattr(raw, name)
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    ws, smooth = L.l2hmc_psis_workspace_bytes, L.l2hmc_psis_smooth
    # error word | x (n, M) | profile (n, 30 + floor(sqrt M))
    assert ws(1000, 6072) == 8 + 8 * 1000 * (6072 + 107) and ws(3, 21467) == 8 + 8 * 3 * (21467 + 176)
    assert ws(7, 0) == 8 + 8 * 7 * 31 and ws(1, 1) == 8 + 8 * 32 and ws(1 << 31, 0) > 0 and ws(1 << 20, 2048) > 0
    for (n, M), msg in (((0, 10), b"n_rows >= 1"), ((-3, 10), b"n_rows >= 1"), ((10, -1), b"tail_len >= 0"),
                        (((1 << 31) + 1, 0), b"tail too large"), (((1 << 20) + 1, 2048), b"tail too large"),
                        ((2, (1 << 30) + 1), b"tail too large"), ((1 << 40, 1 << 40), b"tail too large")):
        assert ws(n, M) == -1, (n, M)
        assert msg in L.l2hmc_last_error(), ((n, M), L.l2hmc_last_error())
        assert smooth(None, None, None, n, M, None, None, None, None) == -1
        assert msg in L.l2hmc_last_error() and b"l2hmc_psis_smooth" in L.l2hmc_last_error(), ((n, M), L.l2hmc_last_error())
        assert L.l2hmc_psis_plan(n, M, 0) == -1
    assert smooth(None, None, None, 10, 64, None, None, None, None) == -1                  # valid shape, NULL pointers
    assert b"required" in L.l2hmc_last_error()
    ok = 1 << 12                                             # an aligned non-NULL address: refused before it is touched
    for at in range(5):                                      # each required pointer NULL in turn
        args = [ok, ok, ok, 10, 64, ok, None, ok, None]
        args[(0, 1, 2, 5, 7)[at]] = None
        assert smooth(*args) == -1 and b"required" in L.l2hmc_last_error(), at
    for at in range(6):                                      # each pointer, the optional weights included, misaligned in turn
        args = [ok, ok, ok, 10, 64, ok, ok, ok, None]
        args[(0, 1, 2, 5, 6, 7)[at]] = ok + 4
        assert smooth(*args) == -1 and b"aligned" in L.l2hmc_last_error(), at
    assert smooth(None, ok, ok, 10, 0, ok, None, ok + 4, None) == -1 and b"aligned" in L.l2hmc_last_error()   # lam may be NULL at M = 0
    assert L.l2hmc_psis_plan(10, 64, 9) == -1 and b"what" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(smooth(None, None, None, 10, 64, None, None, None, None))


# every (n_rows, tail_len) tests/test_gpu_psis.py launches the kernels at -> (theta blocks per row, workgroups along the rows)
GPU_SHAPES = {(4, 5): (4, 4), (3, 6): (4, 3), (9, 65): (5, 9), (9, 257): (6, 9), (3, 769): (8, 3), (3, 6072): (14, 3),
              (3, 21467): (22, 3), (1, 64): (5, 1), (300, 64): (5, 300), (2, 0): (4, 2), (65536, 5): (4, 65536),
              (65539, 5): (4, 65536), (3, 8): (4, 3), (3, 65): (5, 3)}


def test_gpu_shapes_sit_in_their_plan():
    """The plan has no branch by L or M -- one kernel family, a thread carries 8 theta, a workgroup 256 threads, the grid is
    (rows, ceil((30 + floor(sqrt M)) / 8)) -- and one by n_rows: at most 65536 workgroups along the rows (fewer when
    rows x theta blocks would pass 2^23), further rows in a loop.  tests/test_gpu_psis.py runs 65536 and 65539 rows: both sides."""
    from l2hmc_amd import _ffi
    plan = _ffi.lib().l2hmc_psis_plan
    for (n, M), (blocks, grid_rows) in GPU_SHAPES.items():
        assert plan(n, M, 2) == 8 and plan(n, M, 3) == 256
        assert plan(n, M, 4) == 30 + int(np.floor(np.sqrt(max(M, 1))))
        assert plan(n, M, 0) == blocks == -(-plan(n, M, 4) // 8), (n, M)
        assert plan(n, M, 1) == grid_rows == min(n, 65536), (n, M)
    assert plan(1 << 20, 2048, 1) == 65536 and plan(1 << 20, 2048, 0) == 10
    big = (1 << 31) // (1 << 20)                             # 2048 rows of a 2^20-slot tail: 1054 theta, 132 blocks
    assert plan(big, 1 << 20, 0) == 132 and plan(big, 1 << 20, 1) == 2048
    assert plan(100000, 21467, 1) == 65536 and plan(2, 1 << 30, 0) == -(-(30 + 32768) // 8) and plan(2, 1 << 30, 1) == 2
    launched = {(len(rows), M) for M, rows in pc.KERNEL_CASES.values()} | set(pc.EXTRA_KERNEL_SHAPES)
    assert launched == set(GPU_SHAPES), launched ^ set(GPU_SHAPES)
    assert all(M in pc.MEASURED for M, _ in pc.KERNEL_CASES.values())        # every gated tail length was measured


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """From the compiler's listing (tools/kernel_resources.py; skipped when the library was not built here): no kernel of
    psis.s uses scratch, the profile and prep kernels stay within the 128 registers of the 4 waves per SIMD the unit's header
    states, the finish kernel within the 256 of its 2, and no kernel's static LDS exceeds 1 KiB."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = kr.resources().get("psis.s")
    if not rows:
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    regs = {k: (vg, sc) for k, vg, sc, _ in rows}
    assert set(regs) == {"psis_prep_kernel", "psis_profile_kernel", "psis_finish_kernel"}, regs
    header = open(os.path.join(ROOT, "l2hmc_amd", "csrc", "psis.hip")).read()
    assert "4 waves per SIMD" in header and "2 waves per SIMD" in header and "No floating-point atomics" in header
    for k, (vg, sc) in regs.items():
        print("%-24s %4d registers, %d bytes of scratch" % (k, vg, sc))
        assert sc == 0 and vg <= (512 // 2 if k == "psis_finish_kernel" else 512 // 4), (k, vg, sc)
    asm = open(os.path.join(kr.ASM, "psis.s")).read()
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", asm)]
    assert len(lds) == 3 and max(lds) <= 1024, lds
    assert not re.search(r"\b(global|flat)_atomic_(add|min|max|pk_add)_f(16|32|64)\b", asm)   # no floating-point atomics
