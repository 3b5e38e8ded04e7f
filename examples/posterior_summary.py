"""What are the coefficients, and how sure are we?  The coefficient table of a Bayesian logistic regression, on the device
(needs a GPU).

One seeded synthetic data set (1000 rows, d = 8 features) is sampled with HMC -- `warmup` finds the step size,
`sample_chain(record=True)` records the history on the device -- and `describe` reads the recorded history where it lies:
per coefficient the mean and sd, the 5 % / 50 % / 95 % quantiles (exact order statistics: a radix select, no sort and no
copy), split R-hat, the effective sample sizes of the mean and of the interval ends (`ess_tail`), and the Monte Carlo standard
errors that say how many digits of the table are worth printing.  Under the table: how the coefficients are related (the
largest entries of the posterior correlation matrix) and what the run is worth as a whole (`multi_ess`, the multivariate
effective sample size), from one more read of the same history.

    python examples/posterior_summary.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, describe, multi_ess, sample_chain, warmup


def synthetic(n=1000, d=8, seed=0):
    rng = np.random.RandomState(seed)
    X = np.concatenate([np.ones((n, 1)), rng.randn(n, d - 1)], axis=1)
    w_true = np.concatenate([[-0.5], rng.randn(d - 1)])
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w_true))).astype(np.float32)
    return X.astype(np.float32), y, w_true


def main(chains=1024, updates=60, proposals=400, seed=1):
    X, y, w_true = synthetic()
    d = X.shape[1]
    model = LogisticRegression(X, y, prior_var=1.0)
    dyn = Dynamics(d, model.get_energy_function(), T=10, eps=0.01, hmc=True)
    x0 = torch.as_tensor((0.1 * np.random.RandomState(seed).randn(chains, d)).astype(np.float32)).cuda()
    x, info = warmup(x0, dyn, updates, target_accept=0.8, seed=seed)
    _, p, hist = sample_chain(x, dyn, proposals, seed=seed, proposal0=info.next_proposal0, record=True)
    s = describe(hist[proposals // 4:])
    print("eps %.4f, accept %.3f, %d draws per coefficient, max split R-hat %.4f" % (
        info.eps, float(p.mean()), s.n_steps * s.n_chains, s.max_rhat))
    print("%4s %8s %8s %8s %8s %8s %8s %7s %8s %8s %9s %9s" % (
        "coef", "true", "mean", "sd", "5%", "50%", "95%", "rhat", "ess", "ess_tail", "mcse_mean", "mcse_5/95"))
    for k in range(d):
        print("%4d %8.3f %8.3f %8.3f %8.3f %8.3f %8.3f %7.4f %8.0f %8.0f %9.4f %9.4f" % (
            k, w_true[k], s.mean[k], s.sd[k], s.quantiles[0, k], s.quantiles[1, k], s.quantiles[2, k], s.rhat[k], s.ess[k],
            s.ess_tail[k], s.mcse_mean[k], max(s.mcse_quantile[0, k], s.mcse_quantile[2, k])))
    inside = (s.quantiles[0] <= w_true) & (w_true <= s.quantiles[2])
    print("%d of %d true coefficients lie inside their 90 %% interval" % (inside.sum(), d))
    m = multi_ess(hist[proposals // 4:])
    pairs = sorted(((abs(m.corr[i, j]), i, j) for i in range(d) for j in range(i + 1, d)), reverse=True)[:5]
    print("largest posterior correlations: " + ", ".join("(%d, %d) %+.3f" % (i, j, m.corr[i, j]) for _, i, j in pairs))
    print("multivariate ESS %.0f of %d draws (%d batches of %d steps); smallest per-coefficient batch-means ESS %.0f" % (
        m.multi_ess, m.n_draws, m.n_batches, m.batch_size, m.ess_batch.min()))


if __name__ == "__main__":
    main()
