"""Overdispersed counts: data simulated from a negative-binomial model (NB2, dispersion 1.5), sampled on the fused Poisson
target and on the fused negative-binomial target at three fixed dispersions, and compared by PSIS-LOO -- elpd_loo, the
standard error of the pointwise difference to the best model, and the number of Pareto k-hat above 0.7.  The Poisson model
cannot explain the spread of the counts: its elpd is far below and its importance ratios have heavy tails; the negative
binomial at a dispersion near the truth wins.  Nothing leaves the device between the sampler and the comparison: U and grad U
run inside the trajectory kernel, and `loo` reads the recorded history where it lies.

At the end a few lines on aggregated binary data: `BinomialRegression` on y successes out of m trials per row, against the
same data expanded to one row per trial under `LogisticRegression` -- one posterior, 1 / mean(m) of the data contractions.

    python examples/overdispersed_counts.py [--rows 300] [--chains 256] [--steps 300]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from l2hmc_amd import (BinomialRegression, Dynamics, LogisticRegression, NegativeBinomialRegression, PoissonRegression,  # noqa: E402
                       sample_chain, warmup)


def sample(model, dim, chains, steps, burn_in, dev):
    """HMC on the model's fused energy with a step size adapted in warm-up: the recorded history past burn-in, the accept
    rate and the step size."""
    dyn = Dynamics(dim, model.get_energy_function(fused=True), T=10, eps=1e-3, hmc=True, device=dev)
    x0 = torch.zeros(chains, dim, device=dev)
    xw, info = warmup(x0, dyn, 100, target_accept=0.8, seed=1)
    _, p, hist = sample_chain(xw, dyn, steps, seed=2, proposal0=info.next_proposal0, record=True)
    return hist[burn_in:], float(p.mean()), info.eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--burn-in", type=int, default=100)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    dev = torch.device("cuda")
    X = rng.randn(a.rows, a.dim) * 0.5
    X[:, 0] = 1.0
    exposure = rng.uniform(0.5, 3.0, size=a.rows)
    w_true, phi_true = rng.randn(a.dim) * 0.5 + np.r_[1.0, np.zeros(a.dim - 1)], 1.5
    mu = exposure * np.exp(X @ w_true)
    y = rng.negative_binomial(phi_true, phi_true / (phi_true + mu))
    print("counts: mean %.2f, variance %.2f (a Poisson model has them equal)" % (y.mean(), y.var()))

    models = {"Poisson": PoissonRegression(X, y, offset=np.log(exposure), prior_var=4.0)}
    for phi in (0.5, 1.5, 10.0):
        models["NB phi = %g" % phi] = NegativeBinomialRegression(X, y, phi, offset=np.log(exposure), prior_var=4.0)
    loo = {}
    for name, model in models.items():
        draws, acc, eps = sample(model, a.dim, a.chains, a.steps, a.burn_in, dev)
        loo[name] = model.loo(draws, r_eff="auto")
        print("%-12s eps %.4f  accept %.2f  posterior mean %s" % (name, eps, acc, draws.reshape(-1, a.dim).mean(0).cpu().numpy().round(2)))
    best = max(loo, key=lambda k: loo[k].elpd_loo)
    print("truth: w = %s, phi = %g" % (w_true.round(2), phi_true))
    print("%-12s %10s %8s %22s %12s" % ("model", "elpd_loo", "p_loo", "difference to best (se)", "khat > 0.7"))
    for name, s in loo.items():
        diff = s.elpd_loo_i - loo[best].elpd_loo_i
        print("%-12s %10.1f %8.1f %14.1f (%5.1f) %12d" % (name, s.elpd_loo, s.p_loo, diff.sum(), np.sqrt(len(diff) * diff.var()), s.n_bad))

    # aggregated binary data: y successes out of m trials per row, and the same data one row per trial
    m = rng.randint(1, 21, size=a.rows)
    succ = rng.binomial(m, 1.0 / (1.0 + np.exp(-(X @ (w_true - np.r_[1.0, np.zeros(a.dim - 1)])))))
    agg = BinomialRegression(X, succ, m, prior_var=4.0)
    Xl = np.repeat(X, m, axis=0)
    yl = np.concatenate([np.r_[np.ones(s), np.zeros(t - s)] for s, t in zip(succ, m)])
    d_agg, _, _ = sample(agg, a.dim, a.chains, a.steps, a.burn_in, dev)
    long = LogisticRegression(Xl, yl, prior_var=4.0)
    dyn = Dynamics(a.dim, long.get_energy_function(), T=10, eps=1e-3, hmc=True, device=dev)
    xw, info = warmup(torch.zeros(a.chains, a.dim, device=dev), dyn, 100, target_accept=0.8, seed=1)
    _, _, hist = sample_chain(xw, dyn, a.steps, seed=2, proposal0=info.next_proposal0, record=True)
    print("binomial, %d rows of 1 .. 20 trials:  posterior mean %s" % (a.rows, d_agg.reshape(-1, a.dim).mean(0).cpu().numpy().round(3)))
    print("logistic, %d rows (one per trial):  posterior mean %s" % (len(yl), hist[a.burn_in:].reshape(-1, a.dim).mean(0).cpu().numpy().round(3)))
    print("success probability of the first rows, one new trial each:", agg.predict_mean(d_agg, X=X[:5]).round(3))


if __name__ == "__main__":
    main()
