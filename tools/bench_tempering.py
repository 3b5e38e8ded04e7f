#!/usr/bin/env python
"""Parallel tempering throughput (GPU box): proposals/s of the ladder kernel (l2hmc_trajectory_ladder, in-kernel swap sweeps)
against (a) scalar-temperature `sample_chain` at the same N on the general kernel (variant 100: the cost of the swaps) and
(b) the automatic fused T = 1 kernel (variant 0: the cost of the general kernel).  MoG-2D and ICG-50 with S/T/Q nets (the
committed fixtures' weights), 4096 ladders x 8 rungs, M in {1, 5} proposals per round.

    python tools/bench_tempering.py [--ladders 4096] [--rungs 8] [--rounds 40] [--reps 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import ParallelTempering, _ffi, geometric_ladder, sample_chain
from tests import helpers


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    return float(np.median(best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=4096)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    K, nl = a.rungs, a.ladders
    N = K * nl
    temps = geometric_ladder(1.0, 10.0, K)
    for case in ("mog2d", "icg50"):
        g = helpers.load(case)
        dyn = helpers.hip_dynamics(g, variant=100)
        rng = np.random.RandomState(0)
        x0 = torch.as_tensor(g["x"][rng.randint(0, g["x"].shape[0], size=N)]).cuda()
        for M in (1, 5):
            P = a.rounds * M                                   # proposals per launch
            pt = ParallelTempering(dyn, temps, nl, seed=1)
            t_lad = timed(lambda: pt.run(x0, a.rounds, M), a.reps)
            k_lad = _ffi.last_kernel()
            dyn.variant, dyn.use_temperature, dyn.temperature = 100, True, 2.0
            t_sca = timed(lambda: sample_chain(x0, dyn, P, seed=1), a.reps)
            k_sca = _ffi.last_kernel()
            dyn.variant, dyn.use_temperature, dyn.temperature = 0, False, 1.0
            t_fus = timed(lambda: sample_chain(x0, dyn, P, seed=1), a.reps)
            k_fus = _ffi.last_kernel()
            dyn.variant = 100
            r = lambda t: N * P / t                              # noqa: E731  chain-proposals per second
            print("%-6s N = %d (%d ladders x %d rungs), M = %d, %d proposals per launch, T = %d leapfrogs:" % (
                case, N, nl, K, M, P, dyn.T))
            print("  ladder      %-34s %8.3f ms  %.3e proposals/s" % (k_lad, 1e3 * t_lad, r(t_lad)))
            print("  scalar T=2  %-34s %8.3f ms  %.3e proposals/s   ladder / scalar = %.3f" % (k_sca, 1e3 * t_sca, r(t_sca), t_sca / t_lad))
            print("  fused  T=1  %-34s %8.3f ms  %.3e proposals/s   ladder / fused  = %.3f" % (k_fus, 1e3 * t_fus, r(t_fus), t_fus / t_lad))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
