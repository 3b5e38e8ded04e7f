"""Probit next to logit: binary data simulated from a probit model with a few extreme rows, sampled on the fused logit target
(`BinomialRegression`, one trial) and on the fused probit target (`ProbitRegression`), and compared by PSIS-LOO -- elpd_loo,
the standard error of the pointwise difference and the number of Pareto k-hat above 0.7 -- with the two posterior predictive
means side by side.  The two links agree in the middle and differ in the tails (the logistic density has the heavier ones: its
predictive probabilities at the extreme rows are 1e-3 where the probit's are 1e-5); at the default size the two elpd are within
a standard error of each other, which is the usual finding.  Nothing leaves the device between the sampler and the
comparison: U and grad U run inside the trajectory kernel (energy kinds 9 and 10), and `loo` and `predict_mean` read the
recorded history where it lies; the probit link evaluates log Phi by one float32 erfcx that keeps both tails.

    python examples/probit_regression.py [--rows 400] [--chains 256] [--steps 300]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from l2hmc_amd import BinomialRegression, Dynamics, ProbitRegression, sample_chain, warmup  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--burn-in", type=int, default=100)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    dev = torch.device("cuda")
    X = rng.randn(a.rows, a.dim)
    X[:, 0] = 1.0
    X[: a.rows // 10, 1] *= 3.0                                   # a tenth of the rows far out: where the links differ
    w_true = np.r_[0.3, 1.2, rng.randn(a.dim - 2) * 0.5]
    p_true = torch.special.ndtr(torch.as_tensor(X @ w_true)).numpy()
    y = (rng.uniform(size=a.rows) < p_true).astype(np.float64)
    print("binary data: %d rows, %d successes; linear predictor from %.1f to %.1f" % (a.rows, int(y.sum()), (X @ w_true).min(), (X @ w_true).max()))

    models = {"logit": BinomialRegression(X, y, 1, prior_var=4.0), "probit": ProbitRegression(X, y, prior_var=4.0)}
    loo, mean = {}, {}
    for name, model in models.items():
        draws, acc, eps = sample(model, a.dim, a.chains, a.steps, a.burn_in, dev)
        loo[name] = model.loo(draws, r_eff="auto")
        mean[name] = model.predict_mean(draws)
        print("%-7s eps %.4f  accept %.2f  posterior mean %s" % (name, eps, acc, draws.reshape(-1, a.dim).mean(0).cpu().numpy().round(2)))
    print("truth (probit scale): w = %s   (logit coefficients are about 1.6 to 1.8 times the probit ones)" % w_true.round(2))
    best = max(loo, key=lambda k: loo[k].elpd_loo)
    print("%-7s %10s %8s %24s %12s" % ("model", "elpd_loo", "p_loo", "difference to best (se)", "khat > 0.7"))
    for name, s in loo.items():
        diff = s.elpd_loo_i - loo[best].elpd_loo_i
        print("%-7s %10.1f %8.1f %16.1f (%5.1f) %12d" % (name, s.elpd_loo, s.p_loo, diff.sum(), np.sqrt(len(diff) * diff.var()), s.n_bad))
    order = np.argsort(X @ w_true)
    rows = np.r_[order[:3], order[len(order) // 2 - 1: len(order) // 2 + 2], order[-3:]]
    print("posterior predictive P(y = 1) at the three lowest, three middle and three highest rows:")
    print("  truth  ", p_true[rows].round(4))
    for name in models:
        print("  %-7s" % name, mean[name][rows].round(4))
    print("largest |logit - probit| predictive difference over the rows: %.4f" % np.abs(mean["logit"] - mean["probit"]).max())


if __name__ == "__main__":
    main()
