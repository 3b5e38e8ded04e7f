#!/usr/bin/env python3
"""The accuracy record of probit regression (L2HMC_ENERGY_PROBIT, csrc/glm_probit.hip; tests/probit_case.py has the bounds):

    python tools/probit_accuracy.py            # CPU: the float32 numpy restatement's share of every bound, and the
                                               # sensitivities K of the finished numbers (tests/probit_case.py K_*)
    python tools/probit_accuracy.py --device   # plus, on the GPU: the kernels' share of every bound and gate, U, grad U, ll,
                                               # mean, khat, elpd, n_eff, mcse and r_eff, and the largest of each

The output is kept in profiles/probit_accuracy.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import glm_case as gc  # noqa: E402
from tests import loglik_case as lk  # noqa: E402
from tests import probit_case as pc  # noqa: E402

ENERGY_SHAPES = [(1, 2), (17, 5), (1000, 25), (17, 128), (1000, 128), (1000, 65)]


def cpu():
    print("erfcx: ERFCX_ULPS = %g (tools/fit_erfcx.py on np.linspace%s)" % (pc.ERFCX_ULPS, (pc.ERFCX_GRID,)))
    print("float32 numpy restatement: share of the bounds (U, grad U, ll) at 40 chains")
    for n, d in ENERGY_SHAPES:
        c = pc.case(40, n, d)
        U, G = pc.energy(c)
        sU, sg = pc.used(*pc.energy(c, dtype=np.float32), U, G, pc.bounds(c))
        sl = np.max(np.abs(pc.log_lik32(c).astype(np.float64) - pc.log_lik(c)[0]) / pc.ll_bounds(c)["B"])
        print("  n=%-5d d=%-4d U %.3f  grad U %.3f  ll %.3f" % (n, d, sU, sg, sl))
    c = pc.EDGE
    U, G = pc.energy(c)
    sU, sg = pc.used(*pc.energy(c, dtype=np.float32), U, G, pc.bounds(c))
    sl = np.max(np.abs(pc.log_lik32(c).astype(np.float64) - pc.log_lik(c)[0]) / pc.ll_bounds(c)["B"])
    print("  EDGE (t to +-30)  U %.3f  grad U %.3f  ll %.3f" % (sU, sg, sl))
    print("sensitivities: worst |finished(float32 restatement)_i - finished(float64)_i| / max_s |ll32_si - ll64_si|")
    worst, where = np.zeros(4), [None] * 4
    for S, n, d in pc.SHAPES:
        k = pc.sensitivity(pc.case(S, n, d))
        for i in range(4):
            if k[i] > worst[i]:
                worst[i], where[i] = k[i], (S, n, d)
        print("  %-18s khat %.6g  elpd_loo_i %.4g  n_eff (rel) %.4g  mcse (rel) %.6g" % (((S, n, d),) + k))
    for name, w, at in zip(("khat", "elpd_loo_i", "n_eff", "mcse"), worst, where):
        print("  worst %-11s %.6g at %s   (probit_case.K_* = 4 x this, rounded up)" % (name, w, at))
    print("  r_eff on the AR(1) history %s: %.5g" % (gc.AR1, pc.reff_sensitivity(pc.ar1_case())))


def device():
    import torch
    top = {}

    def note(**kw):
        for k, v in kw.items():
            top[k] = max(top.get(k, 0.0), float(v))
    print("the kernels' share of the bounds (tests/probit_case.py)")
    for n, d in ENERGY_SHAPES:
        c = pc.case(40, n, d)
        e = pc.model(c, prior_var=pc.PRIOR_VAR).get_energy_function(fused=True)
        U, G = e.evaluate(torch.as_tensor(c["W"]).cuda(), want_grad=True)
        Ur, Gr = pc.energy(c)
        sU, sg = pc.used(U.cpu().numpy(), G.cpu().numpy(), Ur, Gr, pc.bounds(c))
        note(U=sU, grad_U=sg)
        print("  n=%-5d d=%-4d U %.3f  grad U %.3f" % (n, d, sU, sg))
    c = pc.EDGE
    m = pc.model(c, prior_var=pc.PRIOR_VAR)
    Wd = torch.as_tensor(c["W"]).cuda()
    U, G = m.get_energy_function(fused=True).evaluate(Wd, want_grad=True)
    Ur, Gr = pc.energy(c)
    sU, sg = pc.used(U.cpu().numpy(), G.cpu().numpy(), Ur, Gr, pc.bounds(c))
    b = pc.ll_bounds(c)
    sl = np.max(np.abs(m.log_lik(Wd).cpu().numpy().astype(np.float64) - pc.log_lik(c)[0]) / b["B"])
    sm = np.max(np.abs(m._glm.pointwise_sums(Wd)["sum_mu"] / c["W"].shape[0] - pc.restatement(c)["mean_mu"]) / b["mean_mu"])
    note(U=sU, grad_U=sg, ll=sl, mean=sm)
    print("  EDGE (t to +-30)  U %.3f  grad U %.3f  ll %.3f  mean %.3f" % (sU, sg, sl, sm))
    for S, n, d in pc.SHAPES + pc.GEOM_SHAPES:
        c = pc.case(S, n, d)
        m, Wd = pc.model(c), torch.as_tensor(c["W"]).cuda()
        b, ref = pc.ll_bounds(c), pc.restatement(c)
        ll32 = m.log_lik(Wd).cpu().numpy().astype(np.float64)
        ps, f = m._glm.pointwise_sums(Wd), m.waic(Wd)
        pg = {"mean_mu": ps["sum_mu"] / S, "lppd_i": f.lppd_i, "mean_ll": ps["sum_ll"] / S, "p_waic_i": f.p_waic_i}
        r = lk.r_eff_for(n)
        got, host = m.loo(Wd, r_eff=r), m.loo(c["W"], r_eff=r)
        fin = np.isfinite(host.khat)
        with np.errstate(all="ignore"):
            sh = {"ll": np.max(np.abs(ll32 - pc.log_lik(c)[0]) / b["B"])}
            sh.update({k: np.max(np.abs(pg[k] - ref[k]) / b[k]) for k in pg})
            sh["khat"] = np.max((np.abs(got.khat - host.khat) / (pc.K_KHAT * b["delta"]))[fin]) if fin.any() else 0.0
            sh["elpd"] = np.max(np.abs(got.elpd_loo_i - host.elpd_loo_i) / (pc.K_ELPD * b["delta"]))
            sh["n_eff"] = np.max((gc.rel(got.n_eff, host.n_eff) / (pc.K_NEFF * b["delta"]))[fin]) if fin.any() else 0.0
            sh["mcse"] = np.max((gc.rel(got.mcse_elpd_loo_i, host.mcse_elpd_loo_i) / (pc.K_MCSE * b["delta"]))[fin]) if fin.any() else 0.0
        note(ll=sh["ll"], mean=sh["mean_mu"], lppd=sh["lppd_i"], mean_ll=sh["mean_ll"], p_waic=sh["p_waic_i"], khat=sh["khat"],
             elpd=sh["elpd"], n_eff=sh["n_eff"], mcse=sh["mcse"])
        print("  %-18s " % ((S, n, d),) + "  ".join("%s %.3g" % kv for kv in sh.items()))
    M, N, d, rho, max_lag, split, n = gc.AR1
    c = pc.ar1_case()
    m = pc.model(c)
    delta = pc.ll_bounds(c)["delta"]
    e = m.relative_eff(torch.as_tensor(c["W"]).cuda(), max_lag=max_lag, split=split)
    ref = m.relative_eff(c["W"], max_lag=max_lag, split=split)
    sr = np.max(gc.rel(e.r_eff, ref.r_eff) / (pc.K_REFF * delta))
    note(r_eff=sr)
    print("  AR(1) history: r_eff %.3g .. %.3g, worst relative error / (K_REFF delta_i) %.3g" % (e.r_eff.min(), e.r_eff.max(), sr))
    print("largest share of each bound or gate on the device: " + "  ".join("%s %.3g" % kv for kv in top.items()))
    print("largest of all: %.3g (nothing may exceed 1.0)" % max(top.values()))


if __name__ == "__main__":
    cpu()
    if "--device" in sys.argv:
        device()
