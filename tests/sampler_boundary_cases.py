"""The launches tests/test_gpu_sampler_boundary.py holds against tests/golden/sampler_boundary_parent.npz.

One place says what a case launches, so that the script that recorded the fixture (run once against the parent commit's
library, named through L2HMC_LIB) and the test that reads it cannot drift apart.  Every case is the smallest shape at which
one piece of the sampler kernel's per-launch / per-proposal work can go wrong: 40 chains are two full 16-chain tiles and one
half-live tile; M = 3 proposals cross two proposal boundaries; n_steps = 0, 1, 2 are the trajectories without a look-ahead
tail, with only the last step, and with one paired and one last step.
"""
import numpy as np

from . import helpers

N = 40
SEED = 20240607
STATE_MAX = 2.5e5           # L2HMC_F16_STATE_MAX (l2hmc_amd/csrc/traj_fast.hpp)

_cache = {}


def _case(name):
    """(golden-shaped dict, variant) of the named geometry, built once."""
    if name not in _cache:
        if name in ("icg50", "icg50_v204", "icg50_poison"):
            g = dict(helpers.load("icg50"))
            g["x"], g["v"] = g["x"][:N].copy(), g["v"][:N].copy()
            if name == "icg50_poison":
                g["x"][5, 7] = 3.0e5                # one chain starts beyond the f16x2 range
        elif name == "h14":
            g = helpers.synthetic_case("gauss_diag", 50, H=14, N=N, seed=3)
        elif name == "d20":
            g = helpers.synthetic_case("gauss_diag", 20, N=N, seed=4)
        elif name == "d80":
            g = helpers.synthetic_case("gauss_diag", 80, N=N, seed=7, eps=0.03)      # (at eps = 0.1 nothing is accepted at d = 80)
        elif name == "d16":
            g = helpers.synthetic_case("gauss_diag", 16, N=N, seed=5)
        elif name == "roughwell8":
            g = helpers.synthetic_case("roughwell_easy", 8, N=N, seed=6)
        else:
            raise ValueError(name)
        _cache[name] = (g, 204 if name == "icg50_v204" else 0)
    return _cache[name]


# name -> (geometry, step_begin, n_steps or None for T, M, draws); draws: "rng" or the banked direction pattern
CASES = {
    "rng_s10_m3": ("icg50", 0, None, 3, "rng"),
    "rng_s1_m3": ("icg50", 0, 1, 3, "rng"),
    "rng_s2_m1": ("icg50", 0, 2, 1, "rng"),
    "rng_s0_m2": ("icg50", 0, 0, 2, "rng"),
    "rng_b3_s4_m3": ("icg50", 3, 4, 3, "rng"),
    "bank_fwd": ("icg50", 0, None, 3, "fwd"),
    "bank_bwd": ("icg50", 0, None, 3, "bwd"),
    "bank_mixed": ("icg50", 0, None, 3, "mixed"),
    "h14_m3": ("h14", 0, None, 3, "rng"),
    "d20_m3": ("d20", 0, None, 3, "rng"),
    "d80_m3": ("d80", 0, None, 3, "rng"),
    "d16_m3": ("d16", 0, None, 3, "rng"),
    "roughwell8_m3": ("roughwell8", 0, None, 3, "rng"),
    "v204_m3": ("icg50_v204", 0, None, 3, "rng"),
    "poison_m3": ("icg50_poison", 0, None, 3, "rng"),
}

# what `l2hmc_last_kernel` must report for the cases whose point is the kernel they reach
KERNELS = {
    "rng_s10_m3": "traj_fast_kernel<1, 1, 4, 3, 1>",
    "bank_mixed": "traj_fast_kernel<1, 1, 4, 3, 1>",
    "h14_m3": "traj_fast_kernel<1, 1, 4, 4, 1>",
    "d20_m3": "traj_fast_kernel<1, 1, 4, 3, 1>",       # (two dimension tiles, one per wave, two waves idle)
    "d80_m3": "traj_fast_kernel<1, 2, 4, 3, 1>",       # two dimension tiles per wave
    "d16_m3": "traj_fast_kernel<1, 1, 1, 3, 1>",
    "roughwell8_m3": "traj_fast_kernel<4, 1, 1, 3, 1>",
    "rng_s0_m2": "traj_kernel<1, 1, 4, 3>",            # (no leapfrog step: the planner sends it to the general kernel)
    "v204_m3": "traj_fast_kernel<1, 1, 4, 3>",
}


def banked_draws(geom, M, pattern):
    """(v (M, N, d), direction (M, N) u8, u (M, N)) as host arrays: the same numbers on every call."""
    g, _ = _case(geom)
    d = int(g["x_dim"])
    rs = np.random.RandomState(11)
    v = rs.randn(M, N, d).astype(np.float32)
    u = rs.rand(M, N).astype(np.float32)
    dr = {"fwd": np.ones((M, N), np.uint8), "bwd": np.zeros((M, N), np.uint8),
          "mixed": (rs.rand(M, N) < 0.5).astype(np.uint8)}[pattern]
    return v, dr, u


def launch(name, x=None, M=None, proposal0=0, m0=0):
    """Run case `name` (optionally from state x, for M proposals starting at proposal index proposal0 / bank row m0).
    Returns (dict of host arrays, kernel name)."""
    import torch
    from l2hmc_amd import _ffi
    geom, step_begin, n_steps, M_case, draws = CASES[name]
    g, variant = _case(geom)
    dyn = helpers.hip_dynamics(g, variant=variant)
    M = M_case if M is None else M
    n_steps = int(g["T"]) if n_steps is None else n_steps
    x = helpers.to_dev(g["x"] if x is None else x)
    sq = (lambda a: a if M > 1 else a[0])
    if draws == "rng":
        o = dyn.run(x, None, step_begin, n_steps, want=("p", "x_next"), n_proposals=M,
                    rng={"seed": SEED, "proposal0": proposal0})
    else:
        v, dr, u = banked_draws(geom, M_case, draws)
        o = dyn.run(x, helpers.to_dev(sq(v[m0:m0 + M])), step_begin, n_steps, direction=helpers.to_dev(sq(dr[m0:m0 + M])),
                    u=helpers.to_dev(sq(u[m0:m0 + M])), want=("x", "v", "logjac", "p", "x_next", "x_hist"), n_proposals=M)
    torch.cuda.synchronize()
    return {k: helpers.to_np(t) for k, t in o.items()}, _ffi.last_kernel()
