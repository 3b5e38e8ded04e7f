#!/usr/bin/env python
"""PSIS-LOO of a model the library has no fused kernel for: a Poisson regression with a log link, written as a plain torch
energy and sampled on the slow path (U and grad U by autograd between the library's kernel launches).  Its pointwise
log-likelihood matrix (draws, rows) -- formed here by two torch expressions, which is what makes this the slow path -- goes
through `l2hmc_amd.loo_from_log_lik`: `torch.topk` finds every row's largest importance ratios, the float64 kernels of
csrc/psis.hip fit the generalised Pareto tails and smooth the weights, and the Pareto k-hat says per row whether the estimate
can be trusted.  A second feature set is compared by elpd_loo.

The draws are Markov chains: the same matrix in its history form (steps, chains, rows) goes through
`loo_from_log_lik(..., r_eff="auto", select="fused")` as well -- `relative_eff_from_log_lik` gives every row's relative
efficiency, the fused selection of csrc/loglik_tails.hip cuts every row's tail at its own length, and the result also says how
many effective draws stand behind each elpd_loo_i and how uncertain elpd_loo is by Monte Carlo (`mcse_elpd_loo`).

The same kernels give any importance weights their diagnostic: the log weights of `ais_estimate` (the `'w'` of its returned
state) go through `l2hmc_amd.psis.psis`, which returns their khat and effective sample size.

    python examples/loo_any_likelihood.py [--chains 512] [--steps 400] [--rows 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from l2hmc_amd import Dynamics, LogisticRegression, loo_from_log_lik, psis, sample_chain  # noqa: E402
from l2hmc_amd import distributions as D  # noqa: E402
from l2hmc_amd.ais import ais_estimate  # noqa: E402


def poisson_energy(X, y, prior_var=1.0):
    """U(w) = sum_i (e^eta_i - y_i eta_i) + |w|^2 / (2 prior_var), eta = X w: minus the log posterior up to a constant."""
    def energy(w):
        eta = w @ X.T
        return (torch.exp(eta) - y[None, :] * eta).sum(1) + 0.5 * (w * w).sum(1) / prior_var
    return energy


def poisson_log_lik(W, X, y):
    """(draws, rows): y eta - e^eta - log y!"""
    eta = W @ X.T
    return y[None, :] * eta - torch.exp(eta) - torch.lgamma(y + 1.0)[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(args.seed)
    n, d = args.rows, 4
    X = torch.as_tensor((0.5 * rng.randn(n, d)).astype(np.float32), device=dev)
    w_true = np.array([0.8, -0.5, 0.3, 0.0])                            # the last feature carries nothing
    y = torch.as_tensor(rng.poisson(np.exp(X.cpu().numpy().astype(np.float64) @ w_true + 0.5)).astype(np.float32), device=dev)
    X1 = torch.cat([X, torch.ones((n, 1), device=dev)], dim=1)            # with an intercept

    results = {}
    for name, feats in (("all features + intercept", X1), ("two features + intercept", X1[:, [0, 1, 4]])):
        k = feats.shape[1]
        dyn = Dynamics(k, poisson_energy(feats, y), T=10, eps=0.01, hmc=True, device=dev)   # a plain callable drops in
        # (T eps = 0.1 against posterior standard deviations of 0.06 .. 0.1: well short of a full period of any direction)
        x0 = torch.as_tensor((0.1 * rng.randn(args.chains, k)).astype(np.float32), device=dev)
        _, p, hist = sample_chain(x0, dyn, args.steps, seed=args.seed + 1, record=True)
        W = hist[args.steps // 2:].reshape(-1, k)                        # the first half is burn-in
        ll = poisson_log_lik(W, feats, y)
        s = loo_from_log_lik(ll)
        results[name] = s
        print("%-26s accept %.2f  draws %d  elpd_loo %9.3f (se %.3f)  p_loo %6.3f  lppd %9.3f" % (
            name, float(p.mean()), s.n_draws, s.elpd_loo, s.se, s.p_loo, s.lppd))
        worst = np.argsort(-s.khat)[:3]
        print("%-26s khat: max %.3f, rows above 0.7: %d, above %.3f: %d;  the three largest: %s" % (
            "", float(s.khat.max()), s.n_bad, s.khat_threshold, s.n_above_threshold,
            ", ".join("row %d khat %.3f (y = %d, elpd_loo_i %.3f)" % (i, s.khat[i], int(y[i]), s.elpd_loo_i[i]) for i in worst)))
        m = loo_from_log_lik(ll.reshape(-1, args.chains, n), r_eff="auto", select="fused")     # the chains, not independent draws
        print("%-26s r_eff=\"auto\": r_eff %.3f .. %.3f, tail lengths %d .. %d (independent draws: %d), elpd_loo %9.3f, "
              "min n_eff %.0f, mcse_elpd_loo %.4f, khat max %.3f" % (
                  "", float(np.nanmin(m.r_eff)), float(np.nanmax(m.r_eff)), int(m.tail_len_row.min()), int(m.tail_len_row.max()),
                  s.tail_len, m.elpd_loo, m.min_n_eff, m.mcse_elpd_loo, float(m.khat.max())))
    a, b = results.values()
    diff = a.elpd_loo_i - b.elpd_loo_i
    print("elpd_loo difference (all - two): %.3f, se of the difference %.3f" % (diff.sum(), np.sqrt(n * diff.var(ddof=1))))

    # any importance weights have a k-hat: annealed importance sampling towards a logistic-regression posterior
    dl, N = 3, 4096
    Xl = rng.randn(100, dl).astype(np.float32)
    yl = (rng.rand(100) < 1.0 / (1.0 + np.exp(-Xl @ np.array([1.0, -1.0, 0.5])))).astype(np.float32)
    final = LogisticRegression(Xl, yl, prior_var=1.0).get_energy_function()
    init = D.Gaussian(np.zeros(dl), np.eye(dl)).get_energy_function()
    for K in (4, 64):
        est, alpha, state = ais_estimate(init, final, K, rng.randn(N, dl).astype(np.float32), step_size=0.1, leapfrogs=5,
                                         x_dim=dl, seed=args.seed, return_state=True)
        w = psis.psis(state["w"])
        print("AIS with %3d anneal steps: log Z estimate %.3f, accept %.2f;  PSIS of its %d log weights: khat %.3f, n_eff %.1f" % (
            K, float(est), float(alpha), N, float(w.khat[0]), float(w.n_eff[0])))


if __name__ == "__main__":
    main()
