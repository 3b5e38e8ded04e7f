#!/usr/bin/env python
"""Training at a temperature on the two-mode target of BASELINE config 3 (MoG-2D: components at (+-2, 0), variance 0.1 --
`make("mog2d")` of tools/bench_train.py).  Two samplers from the same initial weights and seed:

  (a) trained at temperature 1 throughout;
  (b) trained on U / temperature with `dynamics.temperature` annealed geometrically from --t0 (8) down to 1 over the first
      two thirds of the steps, then at 1 -- the caller setting the temperature before each step, as a reference user feeds
      its placeholder (dynamics.py:43-47, 203-212).

Both are then sampled at temperature 1 from chains that all start in the right-hand mode; printed: the share of chains
that reached the other mode at least once, the share that sits in it at the end, and the ESS per MH step (func_utils.ESS of
the autocorrelation spectrum).  Nothing is gated: whether tempering helps here is what the run shows.

    python examples/tempered_training.py [--steps 3000] [--chains 200] [--eval-steps 2000] [--t0 8] [--seed 0]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from l2hmc_amd import func_utils, sample_chain  # noqa: E402
from l2hmc_amd.training import Trainer  # noqa: E402
from bench_train import make  # noqa: E402


def train(dyn, x, steps, t0, seed):
    tr = Trainer(dyn, seed=seed)
    anneal = (2 * steps) // 3
    t_start = time.perf_counter()
    for t in range(steps):
        if t0 is not None:
            dyn.use_temperature = True
            dyn.temperature = float(t0 * (1.0 / t0) ** (t / anneal)) if t < anneal else 1.0
        loss, px, x, lr = tr.step(x)
        if t % 500 == 0 or t == steps - 1:
            print("  step %5d  temperature %6.3f  loss %+.3e  accept %.3f" % (
                t, float(dyn.temperature) if dyn.use_temperature else 1.0, float(loss), float(px.mean())))
    torch.cuda.synchronize()
    dyn.use_temperature, dyn.temperature = False, 1.0
    print("  %.1f s, eps = %.4f" % (time.perf_counter() - t_start, float(dyn.eps)))


def evaluate(dyn, n, steps, dev):
    x0 = torch.zeros((n, 2), device=dev)
    x0[:, 0] = 2.0                                              # every chain starts in the right-hand mode
    x0 = x0 + 0.3 * torch.randn((n, 2), device=dev, generator=dyn.generator)
    _, p, hist = sample_chain(x0, dyn, steps, record=True)
    left = hist[:, :, 0] < 0.0
    reached = float(left.any(dim=0).float().mean())
    at_end = float(left[-1].float().mean())
    X = torch.cat([x0[None], hist[:-1]], dim=0)
    ess = float(func_utils.ESS(func_utils.acl_spectrum(X, float(np.sqrt(4.1 + 0.1)))))
    return reached, at_end, ess, float(p.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--eval-steps", type=int, default=2000)
    ap.add_argument("--t0", type=float, default=8.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for label, t0 in (("(a) temperature 1 throughout", None), ("(b) annealed %g -> 1" % args.t0, args.t0)):
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
        dyn, x, _ = make("mog2d", args.chains, dev)              # same weights and draws for both
        print(label)
        train(dyn, x, args.steps, t0, args.seed)
        rows.append((label,) + evaluate(dyn, args.chains, args.eval_steps, dev))
    print("\nsampled at temperature 1, %d chains x %d MH steps, all started at (+2, 0):" % (args.chains, args.eval_steps))
    print("  %-32s %14s %12s %14s %8s" % ("sampler", "reached x < 0", "x < 0 at end", "ESS / MH step", "accept"))
    for label, reached, at_end, ess, acc in rows:
        print("  %-32s %14.3f %12.3f %14.3e %8.3f" % (label, reached, at_end, ess, acc))


if __name__ == "__main__":
    main()
