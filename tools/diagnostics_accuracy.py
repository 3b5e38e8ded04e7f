#!/usr/bin/env python
"""Accuracy of the convergence-diagnostic kernels (csrc/chain_stats.hip) on the MI355X against the float64 restatement of
tests/diagnostics_case.py, on the six AR(1) fixtures, split and unsplit: the raw sums as fractions of G[k, 0], and rhat / ess
relative.  The worst ess deviation is what tests/test_gpu_diagnostics.py gates at ten times (`ESS_MEASURED`).  Then the same
figures for the histories of diagnostics_case.PLAN_FIXTURES (several column chunks per block, d > 256), which the tests gate by
the derived ceiling alone.

    python tools/diagnostics_accuracy.py > profiles/diagnostics_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import diagnostics
from tests import diagnostics_case as dc


def main():
    print("# fixture split max_lag | mean / (|mean| + sd) | M2, G / G[k,0] | rhat, sd, ess relative | ess ceiling (max_lag+1) 4e-5 / tau")
    worst = 0.0
    for name in sorted(dc.FIXTURES):
        X, lag = dc.fixture(name)
        Xd = torch.as_tensor(X).cuda()
        for split in (True, False):
            ref = dc.reference_summary(X, lag, split)
            mean, m2, G = ref["sums"]
            sums = diagnostics.chain_sums(Xd, lag, split)
            got = diagnostics.finish(sums)
            sd = np.sqrt(m2 / (ref["n_steps"] - 1))
            e_mean = np.max(np.abs(sums["mean"].cpu().numpy() - mean) / (np.abs(mean) + sd))
            e_m2 = np.max(np.abs(sums["m2"].cpu().numpy() - m2).sum(axis=0) / G[:, 0])
            e_G = np.max(np.abs(sums["G"].cpu().numpy() - G) / G[:, :1])
            e_rhat = np.max(np.abs(got.rhat - ref["rhat"]) / ref["rhat"])
            e_sd = np.max(np.abs(got.sd - ref["sd"]) / ref["sd"])
            e_ess = np.max(np.abs(got.ess - ref["ess"]) / np.abs(ref["ess"]))
            worst = max(worst, e_ess)
            print("%s %d %3d | %.2e | %.2e %.2e | %.2e %.2e %.2e | %.2e | truncated equal: %s" % (
                name, split, lag, e_mean, e_m2, e_G, e_rhat, e_sd, e_ess, ((lag + 1) * 4e-5 / ref["tau"]).min(),
                bool(np.array_equal(got.truncated, ref["truncated"]))))
    print("worst relative deviation of ess: %.2e" % worst)
    # the histories that reach the plan's other branches (several column chunks per block, d > 256), against the column
    # restatement; their ess is gated by the ceiling alone, the figure above stays that of the six fixtures
    print("# plan fixture (steps x chains x d) split max_lag | the same columns")
    worst = 0.0
    for name in sorted(dc.PLAN_FIXTURES):
        X, lag, split = dc.plan_fixture(name)
        ref = dc.reference_summary_columns(X, lag, split)
        mean, m2, G = ref["sums"]
        sums = diagnostics.chain_sums(torch.as_tensor(X).cuda(), lag, split)
        got = diagnostics.finish(sums)
        sd = np.sqrt(m2 / (ref["n_steps"] - 1))
        e_mean = np.max(np.abs(sums["mean"].cpu().numpy() - mean) / (np.abs(mean) + sd))
        e_m2 = np.max(np.abs(sums["m2"].cpu().numpy() - m2).sum(axis=0) / G[:, 0])
        e_G = np.max(np.abs(sums["G"].cpu().numpy() - G) / G[:, :1])
        e_rhat = np.max(np.abs(got.rhat - ref["rhat"]) / ref["rhat"])
        e_sd = np.max(np.abs(got.sd - ref["sd"]) / ref["sd"])
        e_ess = np.max(np.abs(got.ess - ref["ess"]) / np.abs(ref["ess"]))
        worst = max(worst, e_ess)
        print("%s (%s) %d %3d | %.2e | %.2e %.2e | %.2e %.2e %.2e | %.2e | truncated equal: %s" % (
            name, "x".join(str(v) for v in X.shape), split, lag, e_mean, e_m2, e_G, e_rhat, e_sd, e_ess,
            ((lag + 1) * 4e-5 / ref["tau"]).min(), bool(np.array_equal(got.truncated, ref["truncated"]))))
        sys.stdout.flush()
    print("worst relative deviation of ess over the plan fixtures: %.2e" % worst)


if __name__ == "__main__":
    main()
