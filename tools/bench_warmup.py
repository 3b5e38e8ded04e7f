#!/usr/bin/env python
"""What the device-side step-size warm-up costs (GPU box):

    python tools/bench_warmup.py > profiles/warmup_bench.txt

1. one `l2hmc_adapt_update` (mode 3) at windows of n = 4096, 65 536 (the largest single-workgroup window) and 2^20 values
   (block partials + a second kernel): device events around 200 back-to-back updates, after 20 warm-up updates; five repeats,
   median and range.
2. a 100-update warm-up (`warmup`: 100 x [one sampler launch of one proposal + one adaptation kernel], nothing read back)
   against ONE `sample_chain` launch of the same 100 proposals on the same Dynamics -- the persistent loop the warm-up has to
   break up so that the step size can change between proposals.  Device events around each, the two alternated, seven
   repeats after two warm-up rounds; median, range and the ratio of the medians.  Cases: ICG-50 at 4096 chains with the H = 10
   S/T/Q nets (the bench.py workload) and HMC on the logistic regression n = 1000, d = 25 at 4096 chains.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, distributions as D, layers, sample_chain, warmup
from l2hmc_amd.warmup import adapt_init, adapt_update


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_update():
    dev = torch.device("cuda", 0)
    dyn = Dynamics(2, D.Gaussian(np.zeros(2), np.eye(2)).get_energy_function(), T=10, eps=0.1, hmc=True, device=dev)
    reps = 200
    for n in (4096, 65536, 1 << 20):
        p = torch.rand(n, dtype=torch.float32, device=dev) * 0.2 + 0.7
        state = adapt_init(dyn, search=False)
        ws = adapt_update(p, state, dyn.alpha)

        def burst(k):
            for _ in range(k):
                adapt_update(p, state, dyn.alpha, workspace=ws)
        burst(20)
        torch.cuda.synchronize()
        med, lo, hi = spread([timed(lambda: burst(reps)) / reps for _ in range(5)])
        print("l2hmc_adapt_update  n %8d: %7.2f us per update (median of 5 x %d back-to-back; range %.2f - %.2f)" % (
            n, med * 1e6, reps, lo * 1e6, hi * 1e6), flush=True)


def bench_warmup(name, dyn, x0, updates=100):
    alpha0 = dyn.alpha.detach().clone()
    tw, ts = [], []
    for r in range(9):
        with torch.no_grad():
            dyn.alpha.copy_(alpha0)                                 # every warm-up starts from the same step size
        a = timed(lambda: warmup(x0, dyn, updates, seed=1))
        with torch.no_grad():
            dyn.alpha.copy_(alpha0)
        b = timed(lambda: sample_chain(x0, dyn, updates, seed=1))
        if r >= 2:                                                  # two warm-up rounds
            tw.append(a)
            ts.append(b)
    (mw, lw, hw), (ms, ls, hs) = spread(tw), spread(ts)
    print("%-28s %d-update warm-up %8.3f ms (range %.3f - %.3f) = %6.1f us per update;  one sample_chain launch of %d proposals "
          "%8.3f ms (range %.3f - %.3f) = %6.1f us per proposal;  ratio %.2f" % (
              name, updates, mw * 1e3, lw * 1e3, hw * 1e3, mw * 1e6 / updates, updates, ms * 1e3, ls * 1e3, hs * 1e3,
              ms * 1e6 / updates, mw / ms), flush=True)


def main():
    dev = torch.device("cuda", 0)
    print("device: %s" % torch.cuda.get_device_name(0))
    bench_update()
    torch.manual_seed(0)
    np.random.seed(0)
    rng = np.random.RandomState(0)
    var = np.exp(np.linspace(np.log(1e-2), np.log(1e2), 50))
    icg = Dynamics(50, D.Gaussian(np.zeros(50), np.diag(var)).get_energy_function(), T=10, eps=0.1,
                   net_factory=layers.stq_network(10, head_factor=0.03), device=dev)
    x0 = torch.as_tensor(rng.randn(4096, 50) * np.sqrt(var), dtype=torch.float32, device=dev)
    bench_warmup("ICG-50, 4096 chains, L2HMC", icg, x0)
    n, d = 1000, 25
    X = np.concatenate([np.ones((n, 1)), rng.randn(n, d - 1)], axis=1)
    w = np.concatenate([[-1.0], rng.randn(d - 1) * 0.5])
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w))).astype(np.float32)
    lg = Dynamics(d, LogisticRegression(X, y).get_energy_function(), T=10, eps=0.02, hmc=True, device=dev)
    x0 = torch.as_tensor(0.1 * rng.randn(4096, d), dtype=torch.float32, device=dev)
    bench_warmup("logistic 1000 x 25, 4096 ch", lg, x0)


if __name__ == "__main__":
    main()
