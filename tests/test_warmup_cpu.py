"""CPU: the warm-up's C ABI (symbols, argument errors -- all refused on the host before any launch), `warmup`'s refusal of
`eps_override`, and the float64 restatement of tests/warmup_case.py ALONE on the two fixtures: the caps the GPU test holds the
library to (accept within 0.03 of the target, the two starting points within a factor 1.05) are first shown to be reachable by
the algorithm itself, so the GPU test cannot hide a failure of the algorithm behind one of the kernels or the reverse."""
import math
import types

import numpy as np
import pytest

from l2hmc_amd import _ffi
from tests import warmup_case as wc

FAKE = 0x1000          # a non-NULL "device pointer" for arguments that are not the subject of a case: never dereferenced,
#                        every call below is refused before any launch


def test_the_four_symbols_resolve():
    L = _ffi.lib()
    for name in ("l2hmc_adapt_workspace_doubles", "l2hmc_adapt_init", "l2hmc_adapt_update", "l2hmc_adapt_finish"):
        assert name in _ffi.SYMBOLS and getattr(L, name).argtypes == _ffi.SYMBOLS[name][1]
    assert L.l2hmc_abi_version() == 6
    from l2hmc_amd.warmup import SINGLE_BLOCK_MAX
    assert L.l2hmc_adapt_workspace_doubles(1) == 0 == L.l2hmc_adapt_workspace_doubles(SINGLE_BLOCK_MAX)
    assert L.l2hmc_adapt_workspace_doubles(SINGLE_BLOCK_MAX + 1) == 17           # chunks of 4096
    assert L.l2hmc_adapt_workspace_doubles(1 << 20) == 256
    assert 0 < L.l2hmc_adapt_workspace_doubles(1 << 40) <= 1024


GOOD_INIT = dict(state=FAKE, alpha=FAKE, search=1, target=0.8, gamma=0.05, t0=10.0, kappa=0.75, lo=math.log(1e-8),
                 hi=math.log(1e3))


@pytest.mark.parametrize("change,message", [
    (dict(state=None), b"state and alpha are required"), (dict(alpha=None), b"state and alpha are required"),
    (dict(search=2), b"search must be 0 or 1"),
    (dict(target=0.0), b"target_accept must lie in (0, 1)"), (dict(target=1.0), b"target_accept must lie in (0, 1)"),
    (dict(target=float("nan")), b"target_accept must lie in (0, 1)"),
    (dict(gamma=0.0), b"must be positive"), (dict(t0=-1.0), b"must be positive"), (dict(kappa=0.0), b"must be positive"),
    (dict(lo=1.0, hi=1.0), b"log_eps_min must be below log_eps_max"), (dict(lo=2.0, hi=1.0), b"log_eps_min must be below"),
])
def test_init_argument_errors(change, message):
    L = _ffi.lib()
    a = dict(GOOD_INIT, **change)
    rc = L.l2hmc_adapt_init(a["state"], a["alpha"], a["search"], a["target"], a["gamma"], a["t0"], a["kappa"], a["lo"], a["hi"],
                            None)
    assert rc == -1
    assert message in L.l2hmc_last_error(), L.l2hmc_last_error()


#   (p, n, mode, sums2, state, alpha)
@pytest.mark.parametrize("args,message", [
    ((None, 64, 3, None, FAKE, FAKE), b"p is required"), ((None, 64, 1, FAKE, None, None), b"p is required"),
    ((FAKE, 64, 3, None, None, FAKE), b"state and alpha are required"),
    ((FAKE, 64, 3, None, FAKE, None), b"state and alpha are required"),
    ((None, 0, 2, FAKE, None, FAKE), b"state and alpha are required"),
    ((FAKE, 0, 3, None, FAKE, FAKE), b"n must be >= 1"), ((FAKE, -5, 1, FAKE, None, None), b"n must be >= 1"),
    ((FAKE, 64, 0, FAKE, FAKE, FAKE), b"mode must be"), ((FAKE, 64, 4, FAKE, FAKE, FAKE), b"mode must be"),
    ((FAKE, 64, -1, FAKE, FAKE, FAKE), b"mode must be"),
    ((FAKE, 64, 1, None, None, None), b"sums2 is required"), ((None, 0, 2, None, FAKE, FAKE), b"sums2 is required"),
    ((FAKE, 65537, 3, None, FAKE, FAKE), b"workspace is required"),
])
def test_update_argument_errors(args, message):
    L = _ffi.lib()
    p, n, mode, sums2, state, alpha = args
    assert L.l2hmc_adapt_update(p, n, mode, sums2, state, alpha, None, None, None) == -1
    assert message in L.l2hmc_last_error(), L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="l2hmc_adapt_update"):
        _ffi.check(L.l2hmc_adapt_update(p, n, mode, sums2, state, alpha, None, None, None))


def test_finish_and_workspace_argument_errors():
    L = _ffi.lib()
    assert L.l2hmc_adapt_finish(None, FAKE, None) == -1 and b"state and alpha are required" in L.l2hmc_last_error()
    assert L.l2hmc_adapt_finish(FAKE, None, None) == -1
    assert L.l2hmc_adapt_workspace_doubles(0) == -1 and b"n must be >= 1" in L.l2hmc_last_error()


def test_warmup_refuses_eps_override():
    import l2hmc_amd
    from l2hmc_amd import sharding
    assert callable(l2hmc_amd.warmup)
    dyn = types.SimpleNamespace(eps_override=0.1)
    with pytest.raises(ValueError, match="eps_override"):
        l2hmc_amd.warmup(np.zeros((4, 2), dtype=np.float32), dyn, 3)
    with pytest.raises(ValueError, match="eps_override"):
        sharding.warmup(np.zeros((4, 2), dtype=np.float32), dyn, 3)


def test_restatement_follows_the_phases():
    """The rules in a hand-checked run: two doublings up, the crossing, two averaging updates, finish."""
    da = wc.DualAveraging(math.log(0.1), target=0.8)
    for a in (0.9, 0.7):
        row = da.update(a)
    assert (da.phase, da.dir) == (0, 1) and abs(da.log_eps - math.log(0.4)) < 1e-15
    row = da.update(0.2)
    assert da.phase == 1 and da.t == 0 and row[1] == row[2] and abs(da.mu - math.log(4.0)) < 1e-15
    da.update(0.2)
    h1 = (0.8 - 0.2) / 11.0
    assert abs(da.H_bar - h1) < 1e-15 and abs(da.log_eps - (math.log(4.0) - h1 / 0.05)) < 1e-14
    assert da.log_eps_bar == da.log_eps                                      # e = 1 at t = 1
    le1 = da.log_eps
    da.update(0.9)
    h2 = (1 - 1 / 12.0) * h1 + (0.8 - 0.9) / 12.0
    le2 = math.log(4.0) - math.sqrt(2.0) / 0.05 * h2
    assert abs(da.log_eps - le2) < 1e-14
    assert abs(da.log_eps_bar - (2 ** -0.75 * le2 + (1 - 2 ** -0.75) * le1)) < 1e-14
    da.finish()
    assert da.phase == 2 and da.log_eps == da.log_eps_bar and da.count == 5
    before = da.state().copy()
    da.update(0.3)                                                           # phase 2 records a only
    after = da.state()
    assert after[7] == 0.3 and after[8] == 6 and np.array_equal(np.delete(after, [7, 8]), np.delete(before, [7, 8]))
    # a clamp that binds ends the search at the clamped value
    da = wc.DualAveraging(math.log(0.3), log_eps_min=math.log(1e-2), log_eps_max=0.0)
    da.update(0.9)
    assert da.phase == 0
    da.update(0.9)
    assert da.phase == 1 and da.log_eps == 0.0 and da.mu == wc.LN10
    # search = 0 starts averaging at once
    da = wc.DualAveraging(math.log(0.3), search=False)
    assert da.phase == 1 and da.mu == math.log(0.3) + wc.LN10
    # non-finite accept probabilities count as 0
    assert wc.window_mean(np.array([0.5, np.nan, np.inf, -np.inf], dtype=np.float32)) == 0.125


@pytest.mark.parametrize("name", ["L", "G"])
def test_restatement_alone_meets_the_caps(name):
    out = [wc.restated_warmup(name, e0, seed=s) for s, e0 in enumerate(wc.EPS0[name])]
    for e0, (eps, acc, trace) in zip(wc.EPS0[name], out):
        print("fixture %s from eps0 %g: eps %.4f, accept %.4f over %d further proposals, %d search updates" % (
            name, e0, eps, acc, wc.N_CHECK, int((trace[:, 3] == 0).sum()) + 1))
        assert abs(acc - wc.TARGET) <= wc.CAP_ACCEPT
    ratio = out[0][0] / out[1][0]
    assert max(ratio, 1.0 / ratio) <= wc.CAP_RATIO, ratio
