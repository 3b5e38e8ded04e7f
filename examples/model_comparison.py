"""Which model predicts better?  WAIC, PSIS-LOO and held-out predictive density on the device (needs a GPU).

One seeded synthetic data set (1200 rows, d = 12 features of which the last one is informative; 1000 rows to fit, 200 held
out) and two Bayesian logistic regressions: every feature, and the informative last feature dropped.  Each is sampled with HMC
-- `warmup` finds the step size, `sample_chain(record=True)` records the history on the device -- and checked with
`summarize` (split R-hat, effective sample size).  Then, from the recorded histories where they lie:

  * `model.waic(history)`: the expected log pointwise predictive density of the rows the model was fitted to, by WAIC, its
    effective number of parameters and standard error;
  * `model.loo(history)`: the same quantity by Pareto-smoothed importance-sampling leave-one-out, with the number of rows whose
    Pareto k-hat says the estimate cannot be trusted (`n_bad`); `r_eff="auto"` accounts for the chains' autocorrelation
    (r_eff_i = ESS / S of every row's likelihood) and adds the Monte Carlo standard error of elpd_loo and the smallest
    importance-sampling effective sample size;
  * `log_predictive_density(history, X_test, y_test)`: the same question answered with the 200 rows neither model has seen.

All three should prefer the full model, by a margin of several standard errors of the difference.

    python examples/model_comparison.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, sample_chain, summarize, warmup
from l2hmc_amd.predictive import log_predictive_density


def synthetic(n=1200, d=12, seed=0):
    rng = np.random.RandomState(seed)
    X = np.concatenate([np.ones((n, 1)), rng.randn(n, d - 1)], axis=1)
    w_true = np.concatenate([[-0.5], rng.randn(d - 2) * 0.5, [1.5]])           # the last feature carries most of the signal
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w_true))).astype(np.float32)
    return X.astype(np.float32), y


def fit(X, y, chains, updates, proposals, seed):
    """(model, recorded history after burn-in, its convergence summary)"""
    d = X.shape[1]
    model = LogisticRegression(X, y, prior_var=1.0)
    dyn = Dynamics(d, model.get_energy_function(), T=10, eps=0.01, hmc=True)
    x0 = torch.as_tensor((0.1 * np.random.RandomState(seed).randn(chains, d)).astype(np.float32)).cuda()
    x, info = warmup(x0, dyn, updates, target_accept=0.8, seed=seed)
    _, p, hist = sample_chain(x, dyn, proposals, seed=seed, proposal0=info.next_proposal0, record=True)
    kept = hist[proposals // 4:]
    s = summarize(kept)
    print("  eps %.4f, accept %.3f, max split R-hat %.4f, min ESS %.0f of %d draws" % (
        info.eps, float(p.mean()), s.max_rhat, s.min_ess, s.n_steps * s.n_chains))
    return model, kept, s


def main(chains=1024, updates=60, proposals=200, n_train=1000, seed=1):
    X, y = synthetic()
    X_train, y_train, X_test, y_test = X[:n_train], y[:n_train], X[n_train:], y[n_train:]
    results = {}
    for name, cols in (("all features", slice(None)), ("last feature dropped", slice(0, X.shape[1] - 1))):
        print("%s (d = %d)" % (name, X_train[:, cols].shape[1]))
        model, kept, _ = fit(X_train[:, cols], y_train, chains, updates, proposals, seed)
        w = model.waic(kept)
        h = log_predictive_density(kept, X_test[:, cols], y_test)
        print("  WAIC %.1f: elpd_waic %.1f (se %.1f), p_waic %.2f, lppd %.1f; %d rows with p_waic_i > 0.4, %d underflowed" % (
            w.waic, w.elpd_waic, w.se, w.p_waic, w.lppd, w.n_high_variance, w.n_underflow))
        o = model.loo(kept, r_eff="auto")
        print("  LOO: elpd_loo %.1f (se %.1f, Monte Carlo se %.3f, min n_eff %.0f), p_loo %.2f; %d rows with khat > 0.7 (n_bad), "
              "%d above the threshold %.2f, max khat %.2f" % (o.elpd_loo, o.se, o.mcse_elpd_loo, o.min_n_eff, o.p_loo, o.n_bad,
                                                               o.n_above_threshold, o.khat_threshold, float(np.max(o.khat))))
        print("  relative efficiency of the rows' likelihoods: r_eff %.3f .. %.3f (%d degenerate), tail lengths %d .. %d" % (
            float(np.nanmin(o.r_eff)), float(np.nanmax(o.r_eff)), o.n_reff_nan, o.tail_len_row.min(), o.tail_len_row.max()))
        print("  held-out lppd of %d rows: %.1f (se %.1f)" % (h.n_rows, h.lppd, h.se))
        results[name] = (w, h)
    (wa, ha), (wb, hb) = results["all features"], results["last feature dropped"]
    diff, n = wa.elpd_i - wb.elpd_i, wa.elpd_i.shape[0]
    print("elpd_waic difference (all - dropped): %.1f, se of the difference %.1f" % (diff.sum(), np.sqrt(n * diff.var(ddof=1))))
    hd = ha.lppd_i - hb.lppd_i
    print("held-out lppd difference:             %.1f, se of the difference %.1f" % (
        hd.sum(), np.sqrt(hd.shape[0] * hd.var(ddof=1))))


if __name__ == "__main__":
    main()
