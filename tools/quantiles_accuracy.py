#!/usr/bin/env python
"""Worst relative deviation of `quantiles.describe`'s `ess_quantile` on the device from the float64 restatement of
tests/quantiles_case.py (np.quantile, the indicator history, the estimator of tests/diagnostics_case.py chain by chain), over
the six AR(1) fixtures, split and unsplit, at p = 0.05, 0.5, 0.95 -- the figure tests/test_gpu_quantiles.py quotes as
ESS_QUANTILE_MEASURED.  Also: whether the quantiles equal np.quantile bit for bit and how many stopping indices differ; and,
for the histories of the two PLAN_FIXTURES tables, whether the order statistics equal np.sort and how far the indicator sums
are from the column restatement.

    python tools/quantiles_accuracy.py > profiles/quantiles_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import diagnostics as dg
from l2hmc_amd import quantiles
from tests import diagnostics_case as dc
from tests import quantiles_case as qc


def main():
    assert torch.cuda.is_available(), "quantiles_accuracy needs a GPU"
    worst = 0.0
    print("fixture split   worst ess_quantile rel   ceiling (max_lag+1) 4e-5 / tau   quantiles == np.quantile   truncated differ")
    for name in sorted(dc.FIXTURES):
        X, lag = dc.fixture(name)
        Xd = torch.as_tensor(X).cuda()
        for split in (True, False):
            ref = qc.reference_describe(X, lag, split)
            got = quantiles.describe(Xd, qc.PROBS, lag, split)
            e = np.abs(got.ess_quantile - ref["ess_quantile"]) / ref["ess_quantile"]
            ceiling = ((lag + 1) * 4e-5 / ref["tau_quantile"]).min()
            worst = max(worst, float(e.max()))
            print("%-7s %-5d   %-22.3g   %-30.3g   %-24s   %d" % (
                name, split, e.max(), ceiling, bool(np.array_equal(got.quantiles, ref["quantiles"])),
                int((got.truncated_quantile != ref["truncated_quantile"]).sum())))
            sys.stdout.flush()
    print("worst relative deviation of ess_quantile over all fixtures: %.3g" % worst)
    # the histories that reach the other branches of the two plans (tests/quantiles_case.py, tests/diagnostics_case.py)
    print("plan fixture      ranks   order statistics == np.sort   n_nan equal")
    for name, rows in (("long-walk-d70", 32), ("groups-d512", 3), ("copies-d3", 20)):
        X = qc.plan_history(name)
        Xd = torch.as_tensor(X).cuda()
        S, d = X.shape[0] * X.shape[1], X.shape[2]
        for ranks in (qc.standard_ranks(S), qc.rank_table(S, d, seed=1, R=rows)):
            want, want_nan = qc.reference_order_statistics(X, ranks)
            got, got_nan = quantiles.order_statistics(Xd, ranks)
            print("%-17s %-7d %-28s %s" % (name, ranks.shape[0], bool(np.array_equal(got, want, equal_nan=True)),
                                           bool(np.array_equal(got_nan, want_nan))))
    print("plan fixture      indicator sums at the coordinates' means: mean / (|mean| + sd) | M2, G / G[k,0]")
    for name in ("two-chunks-d3", "period65-d130", "period257-d257"):
        X, lag, split = dc.plan_fixture(name)
        thr = dc.spread(X.shape[2])[1]
        mean, m2, G = dc.reference_sums_columns(qc.indicator_history(X, thr), lag, split)
        sums = dg.chain_sums_below(torch.as_tensor(X).cuda(), thr, lag, split)
        scale = np.abs(mean) + np.sqrt(m2 / (sums["n_steps"] - 1))
        print("%-17s %.2e | %.2e %.2e" % (
            name, np.max(np.abs(sums["mean"].cpu().numpy() - mean) / np.where(scale > 0, scale, 1.0)),
            np.max(np.abs(sums["m2"].cpu().numpy() - m2).sum(axis=0) / G[:, 0]),
            np.max(np.abs(sums["G"].cpu().numpy() - G) / G[:, :1])))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
