#!/usr/bin/env python3
"""The accuracy record of the binomial and negative-binomial regressions (L2HMC_ENERGY_BINOMIAL, csrc/glm_binomial.hip;
tests/binomial_case.py has the bounds):

    python tools/binomial_accuracy.py            # CPU: the float32 numpy restatement's share of every bound, and the
                                                 # sensitivities K of the finished numbers (tests/binomial_case.py K_*)
    python tools/binomial_accuracy.py --device   # plus, on the GPU: the kernels' share of every bound and gate

The output is kept in profiles/binomial_accuracy.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import binomial_case as bc  # noqa: E402
from tests import glm_case as gc  # noqa: E402
from tests import loglik_case as lk  # noqa: E402

ENERGY_SHAPES = [(17, 5), (1000, 25), (17, 128), (1000, 128)]
KINDS = [("binomial", None), ("negbinomial", 0.5), ("negbinomial", 10.0)]


def label(kind, phi):
    return kind if phi is None else "%s phi=%g" % (kind, phi)


def cpu():
    print("float32 numpy restatement: share of the bounds (U, grad U, ll) at 40 chains")
    for n, d in ENERGY_SHAPES:
        for kind, phi in KINDS:
            c = bc.case(40, n, d, kind, phi)
            U, G = bc.energy(c)
            sU, sg = bc.used(*bc.energy(c, dtype=np.float32), U, G, bc.bounds(c))
            sl = np.max(np.abs(bc.log_lik32(c).astype(np.float64) - bc.log_lik(c)[0]) / bc.ll_bounds(c)["B"])
            print("  n=%-5d d=%-4d %-22s U %.3f  grad U %.3f  ll %.3f" % (n, d, label(kind, phi), sU, sg, sl))
    print("sensitivities: worst |finished(float32 restatement)_i - finished(float64)_i| / max_s |ll32_si - ll64_si|")
    worst, where = np.zeros(4), [None] * 4
    for kind, phi, S, n, d in bc.STAT_CASES:
        k = bc.sensitivity(bc.case(S, n, d, kind, phi))
        for i in range(4):
            if k[i] > worst[i]:
                worst[i], where[i] = k[i], (label(kind, phi), S, n, d)
        print("  %-22s %-18s khat %.3g  elpd_loo_i %.3g  n_eff (rel) %.3g  mcse (rel) %.3g" % ((label(kind, phi), (S, n, d)) + k))
    for name, w, at in zip(("khat", "elpd_loo_i", "n_eff", "mcse"), worst, where):
        print("  worst %-11s %.4g at %s   (binomial_case.K_* = 4 x this, rounded up)" % (name, w, at))
    for kind, phi in KINDS:
        print("  r_eff on the AR(1) history %s, %s: %.4g" % (gc.AR1, label(kind, phi), bc.reff_sensitivity(bc.ar1_case(kind, phi))))


def device():
    import torch
    print("the kernels' share of the bounds (tests/binomial_case.py)")
    for n, d in ENERGY_SHAPES:
        for kind, phi in KINDS:
            c = bc.case(40, n, d, kind, phi)
            e = bc.model(c, prior_var=bc.PRIOR_VAR).get_energy_function(fused=True)
            U, G = e.evaluate(torch.as_tensor(c["W"]).cuda(), want_grad=True)
            Ur, Gr = bc.energy(c)
            sU, sg = bc.used(U.cpu().numpy(), G.cpu().numpy(), Ur, Gr, bc.bounds(c))
            print("  n=%-5d d=%-4d %-22s U %.3f  grad U %.3f" % (n, d, label(kind, phi), sU, sg))
    for kind, phi, S, n, d in bc.STAT_CASES:
        c = bc.case(S, n, d, kind, phi)
        m, Wd = bc.model(c), torch.as_tensor(c["W"]).cuda()
        b, ref = bc.ll_bounds(c), bc.restatement(c)
        ll32 = m.log_lik(Wd).cpu().numpy().astype(np.float64)
        ps, f = m._glm.pointwise_sums(Wd), m.waic(Wd)
        pg = {"mean_mu": ps["sum_mu"] / S, "lppd_i": f.lppd_i, "mean_ll": ps["sum_ll"] / S, "p_waic_i": f.p_waic_i}
        r = lk.r_eff_for(n)
        got, host = m.loo(Wd, r_eff=r), m.loo(c["W"], r_eff=r)
        fin = np.isfinite(host.khat)
        with np.errstate(all="ignore"):
            print("  %-22s %-18s ll / B %.3g  predictive / bound: %s   khat / gate %.3g  elpd_loo_i / gate %.3g  n_eff / gate %.3g  "
                  "mcse / gate %.3g" % (label(kind, phi), (S, n, d), np.max(np.abs(ll32 - bc.log_lik(c)[0]) / b["B"]),
                                        "  ".join("%s %.3g" % (k, np.max(np.abs(pg[k] - ref[k]) / b[k])) for k in pg),
                                        np.max((np.abs(got.khat - host.khat) / (bc.K_KHAT * b["delta"]))[fin]) if fin.any() else 0.0,
                                        np.max(np.abs(got.elpd_loo_i - host.elpd_loo_i) / (bc.K_ELPD * b["delta"])),
                                        np.max((gc.rel(got.n_eff, host.n_eff) / (bc.K_NEFF * b["delta"]))[fin]) if fin.any() else 0.0,
                                        np.max((gc.rel(got.mcse_elpd_loo_i, host.mcse_elpd_loo_i) / (bc.K_MCSE * b["delta"]))[fin])
                                        if fin.any() else 0.0))
    M, N, d, rho, max_lag, split, n = gc.AR1
    for kind, phi in KINDS:
        c = bc.ar1_case(kind, phi)
        m = bc.model(c)
        delta = bc.ll_bounds(c)["delta"]
        e = m.relative_eff(torch.as_tensor(c["W"]).cuda(), max_lag=max_lag, split=split)
        ref = m.relative_eff(c["W"], max_lag=max_lag, split=split)
        print("  AR(1) history, %s: r_eff %.3g .. %.3g, worst relative error / (K_REFF delta_i) %.3g"
              % (label(kind, phi), e.r_eff.min(), e.r_eff.max(), np.max(gc.rel(e.r_eff, ref.r_eff) / (bc.K_REFF * delta))))


if __name__ == "__main__":
    cpu()
    if "--device" in sys.argv:
        device()
