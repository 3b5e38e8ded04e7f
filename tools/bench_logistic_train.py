#!/usr/bin/env python
"""One optimiser step on the Bayesian logistic-regression target (GPU box): `LogisticTrainer.step` (the tile training kernel's
logistic-regression form, `train_kernel<7>`: Philox fill, gradient kernel, slot reduction with Adam -- three launches) against
what a user had to do without it: `Trainer(Dynamics(d, fn, ...)).step` with the same likelihood as a torch callable (the
GEMM-engine trainer, one host round trip per gradient and one per Hessian-vector product).

    python tools/bench_logistic_train.py [--T 10] [--H 10] [--steps 20] [--reps 5] [--quick] [--out FILE]

Both paths are warmed up, then timed in alternation (fused window, callable window, fused, ...) so that a drift of the shared
host hits both; a window is `steps` optimiser steps ending in a device synchronise.  Reported: the median window per step and
the spread (min .. max) over the windows, and the algorithmic flop count of the data contractions of one step
(2 N chains, per chain (3 T + 1) gradients at 4 n d and 2 T Hessian-vector products at 6 n d) over the fused time as a fraction of
the 157.3 TFLOP/s f32-MFMA peak -- a whole-step rate, not a kernel's share of peak."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, LogisticTrainer, _ffi, layers
from l2hmc_amd.training import Trainer
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_logistic import data  # noqa: E402  (the seeded standardised data set of the sampling benchmark)

F32_MFMA_PEAK = 157.3e12


def window(tr, x, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        _, _, x, _ = tr.step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20, help="fused steps per timed window (the callable path takes a fifth)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="n = 1000, d = 25, 4096 chains only")
    ap.add_argument("--out", default=None, help="also write the report here")
    a = ap.parse_args()
    grid = [(1000, 25, 4096), (1000, 25, 8192), (4096, 25, 4096), (4096, 25, 8192)]
    if a.quick:
        grid = grid[:1]
    lines = []

    def say(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    say("# tools/bench_logistic_train.py  T = %d  H = %d  %d windows of %d steps, alternating; us per optimiser step" % (a.T, a.H, a.reps, a.steps))
    say("# chains = rows of x; a step proposes from x and from z ~ N(0, I): 2 x chains trajectories per step")
    say("%6s %4s %6s  %-16s %10s %19s %11s %21s %8s %9s" % ("n", "d", "chains", "kernel", "fused us", "(min .. max)",
                                                           "callable us", "(min .. max)", "speedup", "f32 roof"))
    for n, d, N in grid:
        X, y = data(n, d, seed=n + d)
        s2, eps = 1.0, 0.5 / np.sqrt(n)

        def make(energy):
            torch.manual_seed(0)
            np.random.seed(0)
            return Dynamics(d, energy, T=a.T, eps=eps, net_factory=layers.stq_network(a.H))
        fused = LogisticTrainer(make(LogisticRegression(X, y, prior_var=s2).get_energy_function()), seed=1)
        Xt, yt = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()

        def fn(w):
            L = w @ Xt.T
            return (torch.nn.functional.softplus(L) - L * yt).sum(1) + 0.5 * (w * w).sum(1) / s2
        slow = Trainer(make(fn), seed=1)
        x0 = torch.as_tensor((0.1 * np.random.RandomState(1).randn(N, d)).astype(np.float32)).cuda()
        xf, xs = x0.clone(), x0.clone()
        s_steps = max(2, a.steps // 5)
        _, xf = window(fused, xf, 3)                                # warm-up of both shapes
        kern = _ffi.last_kernel()
        _, xs = window(slow, xs, 2)
        tf, ts = [], []
        for _ in range(a.reps):
            t, xf = window(fused, xf, a.steps)
            tf.append(t)
            t, xs = window(slow, xs, s_steps)
            ts.append(t)
        mf, ms = float(np.median(tf)), float(np.median(ts))
        flop = 2.0 * N * n * d * ((3 * a.T + 1) * 4.0 + 2 * a.T * 6.0)
        roof = flop / mf / F32_MFMA_PEAK
        say("%6d %4d %6d  %-16s %10.1f (%7.1f .. %7.1f) %11.1f (%8.1f .. %8.1f) %8.1f %8.2f%%"
            % (n, d, N, kern, 1e6 * mf, 1e6 * min(tf), 1e6 * max(tf), 1e6 * ms, 1e6 * min(ts), 1e6 * max(ts), ms / mf, 100 * roof))
        say(json.dumps({"n": n, "d": d, "chains": N, "T": a.T, "H": a.H, "kernel": kern, "lds_bytes": int(fused.lds_bytes),
                        "fused_us_per_step": [1e6 * t for t in tf], "callable_us_per_step": [1e6 * t for t in ts],
                        "flop_per_step": flop, "f32_roof_fraction_whole_step": roof}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
