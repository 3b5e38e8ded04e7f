"""Poisson regression with the fused model criticism: the model of examples/loo_any_likelihood.py, sampled on the same slow
path (a torch-callable energy with an analytic gradient), with `PoissonRegression`'s fused calls in the place of the torch
log-likelihood matrix -- the (draws, rows) matrix is never formed.  `--fused` samples on the fused target instead
(`get_energy_function(fused=True)`: U and grad U inside the trajectory kernel, no torch callback per leapfrog step).

    python examples/poisson_regression.py [--rows 200] [--chains 256] [--steps 200] [--fused]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import l2hmc_amd  # noqa: E402
from l2hmc_amd import Dynamics, PoissonRegression, sample_chain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--burn-in", type=int, default=100)
    ap.add_argument("--fused", action="store_true", help="sample on the fused Poisson target (default: the torch-callable slow path)")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    X = rng.randn(a.rows, a.dim) * 0.5
    X[:, 0] = 1.0
    exposure = rng.uniform(0.5, 3.0, size=a.rows)
    w_true = rng.randn(a.dim) * 0.5
    y = rng.poisson(exposure * np.exp(X @ w_true))
    model = PoissonRegression(X, y, offset=np.log(exposure), prior_var=4.0)

    dev = torch.device("cuda")
    dyn = Dynamics(a.dim, model.get_energy_function(fused=a.fused), T=10, eps=0.02, hmc=True, device=dev)
    x0 = torch.zeros(a.chains, a.dim, device=dev)
    _, _, hist = sample_chain(x0, dyn, a.steps, seed=1, record=True)
    draws = hist[a.burn_in:]                                 # (steps, chains, dim): read where it lies
    print("posterior mean", draws.reshape(-1, a.dim).mean(0).cpu().numpy().round(3), " truth", w_true.round(3))

    w = model.waic(draws)
    print("WAIC: elpd %.2f  p_waic %.2f  se %.2f  high-variance rows %d" % (w.elpd_waic, w.p_waic, w.se, w.n_high_variance))
    e = model.relative_eff(draws)
    s = model.loo(draws, r_eff=e.r_eff)
    print("LOO:  elpd %.2f  p_loo %.2f  se %.2f  khat > 0.7: %d  min n_eff %.0f  mcse %.3g  (r_eff %.2f .. %.2f)"
          % (s.elpd_loo, s.p_loo, s.se, s.n_bad, s.min_n_eff, s.mcse_elpd_loo, np.nanmin(e.r_eff), np.nanmax(e.r_eff)))
    mu = model.predict_mean(draws)
    print("predictive mean against the counts: correlation %.3f" % np.corrcoef(mu, y)[0, 1])
    # the slow route, for comparison: materialise 64 rows and hand them to the any-likelihood entry
    ll = model.log_lik(draws, rows=(0, min(64, a.rows)))
    t = l2hmc_amd.loo_from_log_lik(ll, select="fused")
    print("first rows, materialised: max |elpd_loo_i difference| %.2g" % np.max(np.abs(t.elpd_loo_i - model.loo(draws).elpd_loo_i[:ll.shape[1]])))


if __name__ == "__main__":
    main()
