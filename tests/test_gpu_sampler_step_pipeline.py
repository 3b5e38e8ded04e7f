"""The one-workgroup-per-CU body's step loop (traj_fast_cc_kernel, csrc/traj_fast.hpp) with a static exchange buffer per site, the
schedule record in per-wave rows behind one pointer, the next step's XNet input split one step ahead and the log-det adds under
the exchanges' reads (L2HMC_ONE_WAVE_ITEMS bits 1, 2, 3 and 5; profiles/sampler_step_pipeline.txt) computes the bits of the
two-wave kernel, whose code and LDS plan that work leaves alone.

L2HMC_FAST_ONE_WAVE=0 / 1 forces either body (the mechanism of tests/test_gpu_sampler_one_wave.py).  The shapes are those at
which the new addressing can go wrong and the old one could not:
  * n_steps 1 / 2 / 3: the peeled last step alone (the split formed at the proposal's start is its only one), one trip of the
    step loop in front of it (one hand-over of the split formed a step ahead), two trips (the record pointer advanced twice,
    every static buffer used again);
  * step_begin = 3 with 4 steps: a partial trajectory -- the backward lanes' table is stored in the order it is walked, so both
    directions start at row step_begin, and the last step's read-ahead goes towards the pad row;
  * M = 1 / 3, M = 3 also against three chained launches (the exchanges outside the step loop -- the first VNet layer-1 sum, the
    epilogue's reduction -- between the static buffers of two proposals; the state a rejected chain resumes from);
  * 16 / 17 / 40 chains: a full tile, one live chain in a tile, three workgroups;
  * H = 10 / 14: the two compiled hidden widths (KH = 3, 4);
  * d = 50, and d = 20: two of the four waves' tiles are dead (their record blocks hold zero masks);
  * a chain beyond L2HMC_F16_STATE_MAX.
"""
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

SEED = 20240911
NMAX = 40
ENV = "L2HMC_FAST_ONE_WAVE"
OLD = {10: "traj_fast_kernel<1, 1, 4, 3, 1>", 14: "traj_fast_kernel<1, 1, 4, 4, 1>"}
NEW = {10: "traj_fast_cc_kernel<1, 1, 4, 3, 1, 1>", 14: "traj_fast_cc_kernel<1, 1, 4, 4, 1, 1>"}

_cases = {}


def _case(d, H):
    if (d, H) not in _cases:
        g = helpers.synthetic_case("gauss_diag", d, H=H, N=NMAX, seed=50 + d + H, eps=0.02)
        _cases[(d, H)] = (g, helpers.hip_dynamics(g))
    return _cases[(d, H)]


def _launch(d, H, one_wave, x, step_begin, n_steps, M, proposal0=0):
    """(x_next, p, body) of one common launch with the body forced."""
    import torch
    from l2hmc_amd import _ffi
    _, dyn = _case(d, H)
    old = os.environ.pop(ENV, None)
    try:
        os.environ[ENV] = str(int(one_wave))
        o = dyn.run(helpers.to_dev(x), None, step_begin, n_steps, want=("p", "x_next"), n_proposals=M,
                    rng={"seed": SEED, "proposal0": proposal0})
        torch.cuda.synchronize()
        body = _ffi.last_kernel(body=True)
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old
    return helpers.to_np(o["x_next"]), helpers.to_np(o["p"]), body


def _same_bits(d, H, x, step_begin, n_steps, M):
    x0, p0, b0 = _launch(d, H, 0, x, step_begin, n_steps, M)
    x1, p1, b1 = _launch(d, H, 1, x, step_begin, n_steps, M)
    assert b0 == OLD[H] and b1 == NEW[H], (b0, b1)
    assert x0.shape == x.shape and np.all(np.isfinite(x0)) and np.all(np.isfinite(p0)) and np.any(p0 > 0)
    assert x0.tobytes() == x1.tobytes() and p0.tobytes() == p1.tobytes()
    return x1, p1


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("steps", [(0, 1), (0, 2), (0, 3), (3, 4)], ids=["n1", "n2", "n3", "from3_n4"])
@pytest.mark.parametrize("N", [16, 17, 40])
@pytest.mark.parametrize("H", [10, 14])
def test_bits_of_the_two_wave_kernel(H, N, steps, M):
    g, _ = _case(50, H)
    x = g["x"][:N]
    x1, p1 = _same_bits(50, H, x, steps[0], steps[1], M)
    if M == 3:      # ... and every proposal starts from the selected state, as a launch of its own does
        xc = x
        for m in range(M):
            xc, pc, bc = _launch(50, H, 1, xc, steps[0], steps[1], 1, proposal0=m)
            assert bc == NEW[H]
            assert pc.tobytes() == p1[m].tobytes(), m
        assert xc.tobytes() == x1.tobytes()


@pytest.mark.parametrize("steps", [(0, 3), (3, 4), (0, 10)], ids=["n3", "from3_n4", "n10"])
@pytest.mark.parametrize("N", [17, 40])
@pytest.mark.parametrize("H", [10, 14])
def test_dead_tiles_d20(H, N, steps):
    g, _ = _case(20, H)
    _same_bits(20, H, g["x"][:N], steps[0], steps[1], 3)


@pytest.mark.parametrize("H", [10, 14])
def test_a_chain_beyond_the_f16_range(H):
    g, _ = _case(50, H)
    x = g["x"][:NMAX].copy()
    x[21, 7] = 3.0e5                    # beyond L2HMC_F16_STATE_MAX = 2.5e5 (traj_fast.hpp)
    x0, p0, b0 = _launch(50, H, 0, x, 0, 3, 3)
    x1, p1, b1 = _launch(50, H, 1, x, 0, 3, 3)
    assert b0 == OLD[H] and b1 == NEW[H]
    assert np.all(p1[:, 21] == 0.0) and np.array_equal(x1[21], x[21])
    keep = np.arange(NMAX) != 21
    assert np.all(np.isfinite(x1[keep])) and np.all(np.isfinite(p1[:, keep]))
    assert x0.tobytes() == x1.tobytes() and p0.tobytes() == p1.tobytes()
