"""Bayesian logistic regression (needs a GPU): HMC, a trained L2HMC sampler and parallel tempering on the fused target against
the same likelihood on the slow path.

A seeded synthetic data set of German-credit shape -- n = 1000 rows, d = 25 standardised features (an intercept column and 24
Gaussian ones), labels drawn from a known weight vector -- nothing is read from disk or the network.  The posterior
U(w) = sum_i [softplus(x_i . w) - y_i x_i . w] + |w|^2 / 2 is sampled by HMC (T = 10 leapfrog steps) on
`LogisticRegression(X, y).get_energy_function()` -- U and grad U fused into the trajectory kernel -- and by the same HMC with U
written as a torch callable (U and grad U from torch between launches).  Both report effective samples per second (the
second half of each chain; the smallest per-coordinate ESS and the largest split R-hat, from `diagnostics.summarize` on the
device history); a 4-rung parallel-tempering ladder on the fused target reports the same for its cold rung, with its swap
rates and round trips.  A trained-sampler leg trains the S/T/Q nets on the fused target (`LogisticTrainer`: the training kernel's logistic-regression
form, `train_steps` optimiser steps), then samples with them (`sample_chain` on the same Dynamics) and reports the same
figure, with the training time beside it; which sampler wins depends on the posterior and the training budget.

    python examples/logistic_regression.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from l2hmc_amd import (Dynamics, LogisticRegression, LogisticTrainer, ParallelTempering, geometric_ladder, layers, sample_chain,
                       summarize)


def german_credit_shape(n=1000, d=25, seed=0):
    rng = np.random.RandomState(seed)
    F = rng.randn(n, d - 1)
    F = (F - F.mean(0)) / F.std(0)
    X = np.concatenate([np.ones((n, 1)), F], axis=1)
    w_true = np.concatenate([[-1.0], rng.randn(d - 1) * 0.5])
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w_true))).astype(np.float32)
    return X.astype(np.float32), y, w_true


def run(dyn, x0, M, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, p, hist = sample_chain(x0, dyn, M, seed=seed, record=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(p.mean()), hist[M // 2:]


def main(chains=4096, proposals=400, slow_proposals=40, seed=1, train_steps=500):
    X, y, w_true = german_credit_shape()
    n, d = X.shape
    model = LogisticRegression(X, y, prior_var=1.0)
    eps, T = 0.02, 10
    x0 = torch.as_tensor((0.1 * np.random.RandomState(2).randn(chains, d)).astype(np.float32)).cuda()

    fused = Dynamics(d, model.get_energy_function(), T=T, eps=eps, hmc=True)
    fused.eps_override = eps
    sample_chain(x0, fused, 2, seed=seed)                           # warm-up (packing, code objects)
    t, acc, hist = run(fused, x0, proposals, seed)
    s_f = summarize(hist)                                           # on the device history: it never leaves the GPU
    ess, rhat = s_f.min_ess, s_f.max_rhat
    print("fused  HMC: %d chains x %d proposals in %.3f s, accept %.3f, min ESS %.0f, max R-hat %.4f -> %.0f ESS/s" % (
        chains, proposals, t, acc, ess, rhat, ess / t))
    print("            posterior mean (first 5): %s   true w: %s" % (
        np.array2string(s_f.mean[:5], precision=3), np.array2string(w_true[:5], precision=3)))

    Xt, yt = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()

    def U(w):
        L = w @ Xt.T
        return (torch.nn.functional.softplus(L) - L * yt).sum(1) + 0.5 * (w * w).sum(1)

    slow = Dynamics(d, U, T=T, eps=eps, hmc=True)
    slow.eps_override = eps
    sample_chain(x0, slow, 1, seed=seed)
    ts, accs, hs = run(slow, x0, slow_proposals, seed)
    s_s = summarize(hs)
    ess_s, rhat_s = s_s.min_ess, s_s.max_rhat
    print("slow   HMC: %d chains x %d proposals in %.3f s, accept %.3f, min ESS %.0f, max R-hat %.4f -> %.0f ESS/s" % (
        chains, slow_proposals, ts, accs, ess_s, rhat_s, ess_s / ts))
    print("fused / slow, time per proposal: x %.1f" % ((ts / slow_proposals) / (t / proposals)))

    # a trained sampler on the same fused target: the nets' parameter tensors are the Dynamics' own, so it samples as it is
    torch.manual_seed(seed)
    np.random.seed(seed)
    l2 = Dynamics(d, model.get_energy_function(), T=T, eps=eps, net_factory=layers.stq_network(10))
    tr = LogisticTrainer(l2, seed=seed)
    xt = x0[:1024].clone()
    tr.step(xt)                                                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(train_steps):
        loss, px, xt, _ = tr.step(xt)
    torch.cuda.synchronize()
    tt = time.perf_counter() - t0
    sample_chain(x0, l2, 2, seed=seed)
    tl, accl, hl = run(l2, x0, proposals, seed)
    s_l = summarize(hl)
    ess_l, rhat_l = s_l.min_ess, s_l.max_rhat
    print("fused L2HMC: trained %d steps on 1024 chains in %.2f s (loss %.4g, step size %.4f); %d chains x %d proposals in %.3f s, "
          "accept %.3f, min ESS %.0f, max R-hat %.4f -> %.0f ESS/s (HMC above: %.0f)" % (
              train_steps, tt, float(loss), float(torch.exp(l2.alpha.detach()).reshape(-1)[0]), chains, proposals, tl, accl, ess_l,
              rhat_l, ess_l / tl, ess / t))

    ladder = geometric_ladder(1.0, 4.0, 4)
    ParallelTempering(fused, ladder, chains // 4, seed=seed).run(x0, 2, 1)      # warm-up (the ladder kernel's first launch)
    pt = ParallelTempering(fused, ladder, chains // 4, seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = pt.run(x0, proposals, 1, record_cold=True)
    torch.cuda.synchronize()
    tp = time.perf_counter() - t0
    s_p = summarize(o["cold_hist"][proposals // 2:])
    ess_p, rhat_p = s_p.min_ess, s_p.max_rhat
    print("PT (ladder %s): %.3f s, cold-rung min ESS %.0f, max R-hat %.4f -> %.0f ESS/s, swap rates %s, round trips per ladder %.2f" % (
        ", ".join("%.2f" % v for v in ladder), tp, ess_p, rhat_p, ess_p / tp, " ".join("%.2f" % r for r in o["swap_rate"].tolist()),
        float(o["round_trips"].sum()) / (chains // 4)))


if __name__ == "__main__":
    main()
