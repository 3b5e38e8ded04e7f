"""Parallel tempering on a two-mode mixture (needs a GPU).

MoG-2D with unit-variance modes at x0 = -5 (weight 0.7) and +5 (weight 0.3).  The barrier between them is 12.5 nats at T = 1:
HMC with eps = 0.5 and 10 leapfrog steps, started in the heavy mode, never finds the light one.  A ladder of 8 rungs from T = 1 to
T = 40 (geometric; the barrier is 0.3 nats at the top) swaps states between neighbouring rungs after every proposal, and the cold
rung recovers the weights.  1024 ladders, 1500 rounds; the second half of the cold rung's history is the sample.

    python examples/parallel_tempering.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from l2hmc_amd import Dynamics, ParallelTempering, geometric_ladder, sample_chain, summarize
from l2hmc_amd import distributions as D


def main(n_ladders=1024, rounds=1500, seed=1):
    energy = D.GMM([np.array([-5.0, 0.0]), np.array([5.0, 0.0])], [np.eye(2), np.eye(2)], [0.7, 0.3]).get_energy_function()
    dyn = Dynamics(2, energy, T=10, eps=0.5, hmc=True)
    dyn.eps_override = 0.5
    ladder = geometric_ladder(1.0, 40.0, 8)
    K = len(ladder)
    rng = np.random.RandomState(0)
    x0 = torch.as_tensor((np.array([-5.0, 0.0]) + rng.randn(n_ladders * K, 2)).astype(np.float32)).cuda()

    # every chain starts in the heavy mode; to see what R-hat says about chains that never cross, a tenth of them is also
    # started in the light one: the two groups stay apart and R-hat of x0 is far from 1 however long HMC runs
    xs, _, _ = sample_chain(x0, dyn, rounds, seed=seed)
    print("HMC at T = 1, %d proposals:     fraction in the light mode %.4f (target 0.3)" % (
        rounds, float((xs[:, 0] > 0).float().mean())))
    x_two = x0.clone()
    x_two[::10, 0] += 10.0
    _, _, hist = sample_chain(x_two, dyn, rounds, seed=seed, record=True)
    s = summarize(hist[rounds // 2:])
    print("  started in both modes (1 : 9):  R-hat of x0 %.3f, of x1 %.4f; ESS of x0 %.0f of %d draws" % (
        s.rhat[0], s.rhat[1], s.ess[0], s.n_steps * s.n_chains))

    pt = ParallelTempering(dyn, ladder, n_ladders, seed=seed)
    o = pt.run(x0, rounds, 1, record_cold=True)
    cold = o["cold_hist"][rounds // 2:]
    print("PT, ladder %s:" % ", ".join("%.2f" % t for t in ladder))
    print("  cold rung, second half:        fraction in the light mode %.4f (target 0.3)" % float((cold[..., 0] > 0).float().mean()))
    s = summarize(cold)
    print("  cold rung, second half:        R-hat of x0 %.4f, of x1 %.4f; ESS of x0 %.0f of %d draws" % (
        s.rhat[0], s.rhat[1], s.ess[0], s.n_steps * s.n_chains))
    print("  swap rates by pair:            %s" % " ".join("%.2f" % r for r in o["swap_rate"].tolist()))
    print("  round trips per ladder:        %.1f" % (float(o["round_trips"].sum()) / n_ladders))


if __name__ == "__main__":
    main()
