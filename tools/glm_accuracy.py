#!/usr/bin/env python3
"""The accuracy record of the Poisson regression's fused model criticism (csrc/glm.hip; tests/glm_case.py has the bounds):

    python tools/glm_accuracy.py            # CPU: the sensitivities K of the float64 route (tests/glm_case.py K_*)
    python tools/glm_accuracy.py --device   # plus, on the GPU: the device's share of every bound and gate

The output is kept in profiles/glm_accuracy.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import glm_case as gc  # noqa: E402
from tests import loglik_case as lk  # noqa: E402


def cpu():
    print("sensitivities of the float64 route under +-B_si (8 sign patterns): worst |change| / delta_i")
    worst = np.zeros(4)
    for shape in gc.SHAPES:
        k = gc.sensitivity(*shape)
        worst = np.maximum(worst, k)
        print("  %-18s khat %.3g  elpd_loo_i %.3g  n_eff (rel) %.3g  mcse (rel) %.3g" % ((shape,) + k))
    print("  worst              khat %.3g  elpd_loo_i %.3g  n_eff %.3g  mcse %.3g   (glm_case.K_* = 4 x these, rounded up)" % tuple(worst))
    print("  r_eff on the AR(1) history %s: %.3g" % (gc.AR1, gc.reff_sensitivity()))


def device():
    import torch
    import l2hmc_amd
    print("the device's share of the bounds (tests/glm_case.py)")
    for S, n, d in gc.SHAPES:
        W, X, y, o = gc.case(S, n, d)
        m = l2hmc_amd.PoissonRegression(X, y, offset=o)
        Wd = torch.as_tensor(W).cuda()
        ll64, _ = gc.log_lik(W, X, y, o)
        b = gc.bounds(W, X, y, o)
        ll_dev = m.log_lik(Wd).cpu().numpy()
        ll32 = ll_dev.astype(np.float64)
        # the three raw sums against `loglik_case.sum_bounds` of the written matrix; the predictive numbers against theirs
        t = m._glm.loo_tails(Wd)
        ex = lk.select_exact(ll_dev, np.full(n, t["tail"].shape[1], dtype=np.int64))
        ref_s, bound_s = lk.sum_bounds(ll_dev, ex)
        sums = np.stack([t[k].cpu().numpy() for k in ("body", "body_sq", "lik")])
        ps, f, pr = m._glm.pointwise_sums(Wd), m.waic(Wd), gc.restatement(W, X, y, o)
        pg = {"mean_mu": ps["sum_mu"] / S, "lppd_i": f.lppd_i, "mean_ll": ps["sum_ll"] / S, "p_waic_i": f.p_waic_i}
        print("  %-18s sums / sum_bounds %.3g   predictive / bound: %s" % ((S, n, d), np.max(np.abs(sums - ref_s) / bound_s),
              "  ".join("%s %.3g" % (k, np.max(np.abs(pg[k] - pr[k]) / b[k])) for k in pg)))
        r = lk.r_eff_for(n)
        got, ref = m.loo(Wd, r_eff=r), m.loo(W, r_eff=r)
        fin = np.isfinite(ref.khat)
        with np.errstate(all="ignore"):
            print("  %-18s ll / B %.3g   khat / gate %.3g  elpd_loo_i / gate %.3g  n_eff / gate %.3g  mcse / gate %.3g"
                  % ((S, n, d), np.max(np.abs(ll32 - ll64) / b["B"]),
                     np.max((np.abs(got.khat - ref.khat) / (gc.K_KHAT * b["delta"]))[fin]) if fin.any() else 0.0,
                     np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / (gc.K_ELPD * b["delta"])),
                     np.max((gc.rel(got.n_eff, ref.n_eff) / (gc.K_NEFF * b["delta"]))[fin]) if fin.any() else 0.0,
                     np.max((gc.rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / (gc.K_MCSE * b["delta"]))[fin]) if fin.any() else 0.0))


def device_reff():
    import torch
    import l2hmc_amd
    M, N, d, rho, max_lag, split, n = gc.AR1
    W, X, y, o = gc.ar1_case()
    m = l2hmc_amd.PoissonRegression(X, y, offset=o)
    delta = gc.bounds(W, X, y, o)["delta"]
    e = m.relative_eff(torch.as_tensor(W).cuda(), max_lag=max_lag, split=split)
    ref = m.relative_eff(W, max_lag=max_lag, split=split)
    print("  AR(1) history %s: r_eff %.3g .. %.3g, worst relative error / (K_REFF delta_i) %.3g"
          % (gc.AR1, e.r_eff.min(), e.r_eff.max(), np.max(gc.rel(e.r_eff, ref.r_eff) / (gc.K_REFF * delta))))


if __name__ == "__main__":
    cpu()
    if "--device" in sys.argv:
        device()
        device_reff()
