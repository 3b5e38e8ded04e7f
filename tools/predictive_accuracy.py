#!/usr/bin/env python
"""Accuracy of the posterior-predictive / WAIC kernel (csrc/predictive.hip) on the MI355X against the float64 numpy path of
l2hmc_amd/predictive.py on the same float32 inputs: for every case of tests/test_gpu_predictive.py's main test (and the
saturated and constant-label ones) the worst error-to-bound ratio of p_mean, lppd_i, mean ll and p_waic_i, the bounds being those
of tests/predictive_case.py `device_bounds`.  A ratio above 1 fails the GPU test.

    python tools/predictive_accuracy.py > profiles/predictive_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import predictive
from tests import predictive_case as pc

SHAPES = [(21, 1, 1), (37, 17, 3), (16, 16, 16), (523, 33, 17), (300, 50, 128), (4099, 100, 25)]


def finished(sums):
    f = predictive.finish(sums)
    f["mean_ll"] = np.asarray(sums["sum_ll"]) / sums["n_draws"]
    return f


def main():
    print("# (S, n, d) case | worst |error| / bound: p_mean, lppd_i, mean ll, p_waic_i | worst |error|: the same four")
    cases = [(s, {}) for s in SHAPES] + [((523, 33, 17), {"labels": "ones"}), ((523, 33, 17), {"labels": "zeros"}),
                                         ((523, 33, 17), {"max_logit": 60.0, "x_scale": 8.0})]
    worst = dict.fromkeys(("p_mean", "lppd_i", "mean_ll", "p_waic_i"), 0.0)
    for (S, n, d), kw in cases:
        W, X, y = pc.case(S, n, d, seed=1000 + S + n + d, **kw)
        ref = finished(predictive.pointwise_sums(W, X, y))
        got = finished(predictive.pointwise_sums(torch.as_tensor(W).cuda(), X, y))
        r = pc.ratios(got, ref, pc.device_bounds(W, X, y))
        e = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in r}
        for k in r:
            worst[k] = max(worst[k], r[k])
        print("(%d, %d, %d) %s | %.3f %.3f %.3f %.3f | %.2e %.2e %.2e %.2e" % (
            S, n, d, " ".join("%s=%s" % kv for kv in sorted(kw.items())) or "-", r["p_mean"], r["lppd_i"], r["mean_ll"],
            r["p_waic_i"], e["p_mean"], e["lppd_i"], e["mean_ll"], e["p_waic_i"]))
    print("worst error / bound: p_mean %.3f  lppd_i %.3f  mean ll %.3f  p_waic_i %.3f" % (
        worst["p_mean"], worst["lppd_i"], worst["mean_ll"], worst["p_waic_i"]))


if __name__ == "__main__":
    main()
