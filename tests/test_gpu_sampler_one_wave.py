"""The sampler kernel's one-workgroup-per-CU body (traj_fast_cc_kernel, csrc/traj_fast.hpp: the common-launch body of
traj_fast_kernel<1, 1, 4, ., 1> under __launch_bounds__(256, 1), with both nets' tails loaded once per launch) computes the bits
of the two-wave kernel it stands in for.

L2HMC_FAST_ONE_WAVE=0 / 1 forces either body for a launch that can take both (read at plan time, per call); without it the grid
decides: at most one workgroup per CU -> the new body.  `_ffi.last_kernel()` names the kernel either way (same statements, same
bits: one kernel to its callers, and tests/test_gpu_sampler_boundary.py holds that name against the parent's);
`_ffi.last_kernel(body=True)` names the __global__ function that ran.

Shape: ICG-50 (d = 50, T = 10, in-kernel draws).  H = 10 and 14 are the two compiled hidden widths (KH = 3, 4); 16 / 17 / 40
chains are one tile, a one-chain second tile and a half-filled last tile; n_steps 10 / 2 / 1 are step loop plus peeled last step,
the peel after one trip, and the peel alone; M = 3 crosses two proposal boundaries, where the held tails and the per-proposal
sign of the cS row are used again.
"""
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

SEED = 20240607
NMAX = 40
ENV = "L2HMC_FAST_ONE_WAVE"
OLD = {10: "traj_fast_kernel<1, 1, 4, 3, 1>", 14: "traj_fast_kernel<1, 1, 4, 4, 1>"}
NEW = {10: "traj_fast_cc_kernel<1, 1, 4, 3, 1, 1>", 14: "traj_fast_cc_kernel<1, 1, 4, 4, 1, 1>"}

_cases = {}


def _case(H):
    if H not in _cases:
        g = helpers.synthetic_case("gauss_diag", 50, H=H, N=NMAX, seed=30 + H, eps=0.02)
        _cases[H] = (g, helpers.hip_dynamics(g))
    return _cases[H]


def _launch(H, one_wave, x, n_steps, M, proposal0=0, **kw):
    """(x_next, p, kernel, body) of one common launch with the body forced (None: the planner's own choice)."""
    import torch
    from l2hmc_amd import _ffi
    _, dyn = _case(H)
    old = os.environ.pop(ENV, None)
    try:
        if one_wave is not None:
            os.environ[ENV] = str(int(one_wave))
        want = kw.pop("want", ("p", "x_next"))
        o = dyn.run(helpers.to_dev(x), None, 0, n_steps, want=want, n_proposals=M, rng={"seed": SEED, "proposal0": proposal0})
        torch.cuda.synchronize()
        names = (_ffi.last_kernel(), _ffi.last_kernel(body=True))
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old
    return (helpers.to_np(o["x_next"]), helpers.to_np(o["p"])) + names


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n_steps", [10, 2, 1])
@pytest.mark.parametrize("N", [16, 17, 40])
@pytest.mark.parametrize("H", [10, 14])
def test_bits_of_the_two_wave_kernel(H, N, n_steps, M):
    g, _ = _case(H)
    x = g["x"][:N]
    x0, p0, k0, b0 = _launch(H, 0, x, n_steps, M)
    x1, p1, k1, b1 = _launch(H, 1, x, n_steps, M)
    assert k0 == k1 == b0 == OLD[H] and b1 == NEW[H], (k0, b0, k1, b1)
    assert x0.shape == (N, 50) and np.all(np.isfinite(x0)) and np.all(np.isfinite(p0))
    assert np.any(p0 > 0)
    assert x0.tobytes() == x1.tobytes() and p0.tobytes() == p1.tobytes()
    if M == 3:      # ... and the held tails across proposal boundaries equal a fresh prologue per proposal
        xc = x
        for m in range(M):
            xc, pc, _, bc = _launch(H, 1, xc, n_steps, 1, proposal0=m)
            assert bc == NEW[H]
            assert pc.tobytes() == p1[m].tobytes(), m
        assert xc.tobytes() == x1.tobytes()


@pytest.mark.parametrize("H", [10, 14])
def test_a_chain_beyond_the_f16_range_is_poisoned_the_same_way(H):
    g, _ = _case(H)
    x = g["x"][:NMAX].copy()
    x[21, 7] = 3.0e5                    # beyond L2HMC_F16_STATE_MAX = 2.5e5 (traj_fast.hpp)
    x0, p0, _, b0 = _launch(H, 0, x, 10, 3)
    x1, p1, _, b1 = _launch(H, 1, x, 10, 3)
    assert b0 == OLD[H] and b1 == NEW[H]
    assert np.all(p1[:, 21] == 0.0) and np.array_equal(x1[21], x[21])
    keep = np.arange(NMAX) != 21
    assert np.all(np.isfinite(x1[keep])) and np.all(np.isfinite(p1[:, keep]))
    assert x0.tobytes() == x1.tobytes() and p0.tobytes() == p1.tobytes()


def test_the_grid_selects_the_body():
    """M = 1, n_steps = 2: at most one workgroup per CU -> the one-workgroup-per-CU body; one workgroup more, or a launch that is
    not the common one (x_hist), -> the two-wave kernel."""
    import torch
    g, _ = _case(10)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16 * (cus + 1)
    x = np.tile(g["x"], ((n + NMAX - 1) // NMAX, 1))[:n] + 0.01 * np.random.RandomState(5).randn(n, 50).astype(np.float32)
    xa, pa, ka, ba = _launch(10, None, x[:16 * cus], 2, 1)
    assert (ka, ba) == (OLD[10], NEW[10])
    xb, pb, kb, bb = _launch(10, None, x, 2, 1)
    assert (kb, bb) == (OLD[10], OLD[10])
    # (a chain's result does not depend on its neighbours' tiles: the shared chains agree bit for bit across the two bodies)
    assert xa.tobytes() == xb[:16 * cus].tobytes() and pa.tobytes() == pb[:16 * cus].tobytes()
    _, _, kh, bh = _launch(10, None, x[:NMAX], 2, 1, want=("p", "x_next", "x_hist"))
    assert (kh, bh) == (OLD[10], OLD[10])
    _, _, kh, bh = _launch(10, 1, x[:NMAX], 2, 1, want=("p", "x_next", "x_hist"))       # (forcing does not reach it either)
    assert (kh, bh) == (OLD[10], OLD[10])
