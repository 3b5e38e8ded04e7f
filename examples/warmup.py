"""Which step size?  Warm-up by dual averaging on the device (needs a GPU).

Bayesian logistic regression on a seeded synthetic data set (n = 1000 rows, d = 25 features).  HMC with T = 10 leapfrog steps
is started once with a step size far too small (1e-4) and once far too large (2.0); `warmup` finds the step size from either
side -- a doubling search until the mean accept probability crosses 0.5, then dual averaging towards the target -- with one
sampler launch and one small adaptation kernel per update and nothing copied to the host in between.  The adapted `Dynamics`
then samples with `sample_chain`, and `summarize` reports split R-hat and the effective sample size.

    python examples/warmup.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, sample_chain, summarize, warmup


def synthetic(n=1000, d=25, seed=0):
    rng = np.random.RandomState(seed)
    X = np.concatenate([np.ones((n, 1)), rng.randn(n, d - 1)], axis=1)
    w_true = np.concatenate([[-1.0], rng.randn(d - 1) * 0.5])
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w_true))).astype(np.float32)
    return X.astype(np.float32), y


def main(chains=4096, updates=100, proposals=400, target=0.8, seed=1):
    X, y = synthetic()
    d = X.shape[1]
    model = LogisticRegression(X, y, prior_var=1.0)
    x0 = torch.as_tensor((0.1 * np.random.RandomState(2).randn(chains, d)).astype(np.float32)).cuda()
    tuned = None
    for eps0 in (1e-4, 2.0):
        dyn = Dynamics(d, model.get_energy_function(), T=10, eps=eps0, hmc=True)
        sample_chain(x0, dyn, 1, seed=seed)                         # first launch (code objects, the packed data set)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = warmup(x0, dyn, updates, target_accept=target, seed=seed)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        print("from eps %-6g: adapted eps %.4f (accept %.3f in the last window; %d search + %d averaging updates) in %.1f ms" % (
            eps0, info.eps, info.accept, info.n_search, info.n_averaged, 1e3 * t))
        tuned = (dyn, x, info)
    dyn, x, info = tuned
    _, p, hist = sample_chain(x, dyn, proposals, seed=seed, proposal0=info.next_proposal0, record=True)
    s = summarize(hist[proposals // 4:])
    print("sampling at eps %.4f: accept %.3f (target %.2f), min ESS %.0f of %d, max split R-hat %.4f" % (
        info.eps, float(p.mean()), target, s.min_ess, s.n_steps * s.n_chains, s.max_rhat))


if __name__ == "__main__":
    main()
