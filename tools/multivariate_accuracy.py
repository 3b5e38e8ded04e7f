#!/usr/bin/env python
"""Worst deviation of the device's raw moments (`multivariate.moment_sums`, csrc/moment_sums.hip) and of `multi_ess` from the
two-pass float64 restatement of tests/multivariate_case.py, per fixture: the sums as a fraction of their gate
1e-10 sqrt(raw_ii raw_jj), multi_ess relative, next to the first-order bound 2 B tests/test_gpu_multivariate.py derives.  Then
the same for the histories of multivariate_case.PLAN_FIXTURES (more than 256 chunks of chains, every panel shape), with batches
and -- the sums alone -- without.

    python tools/multivariate_accuracy.py > profiles/multivariate_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import multivariate
from tests import multivariate_case as mc
from tests.test_gpu_multivariate import FIXTURES, PLAN_NAMES, mess_bound


def sums_fraction(got, ref):
    frac = 0.0
    for vec, mat, count in (("sum", "cross", ref["n_draws"]), ("batch_sum", "batch_cross", ref.get("n_batches"))):
        if got[mat] is None:
            continue
        gv, gm = mc.sum_gates(np.diag(ref[mat]), count)
        frac = max(frac, float(np.max(np.abs(got[vec].cpu().numpy() - ref[vec]) / gv)),
                   float(np.max(np.abs(got[mat].cpu().numpy() - ref[mat]) / gm)))
    return frac


def row(name, width):
    X = mc.history(name)
    Xd = torch.as_tensor(np.array(X)).cuda()
    b = mc.default_batch(X.shape[0])
    ref = mc.reference(X, b)
    got = multivariate.moment_sums(Xd, b)
    frac = sums_fraction(got, ref)
    s = multivariate.finish(got)
    e = abs(s.multi_ess - ref["multi_ess"]) / ref["multi_ess"]
    print("%-*s %-19s %-7d %-34.3g %-14.6g %-20.3g %-11.3g %.3g" % (
        width, name, "x".join(str(v) for v in X.shape), b, frac, s.multi_ess, e, 2 * mess_bound(ref),
        np.linalg.cond(ref["cov_asymptotic"])))
    sys.stdout.flush()
    return frac, e, Xd


def main():
    assert torch.cuda.is_available(), "multivariate_accuracy needs a GPU"
    print("fixture shape               batch   sums: worst fraction of the gate   multi_ess      relative deviation   "
          "bound 2 B   cond(Sigma)")
    worst_sum = worst_ess = 0.0
    for name in FIXTURES + ["R"]:
        frac, e, _ = row(name, 7)
        worst_sum, worst_ess = max(worst_sum, frac), max(worst_ess, e)
    print("worst over all fixtures: sums %.3g of their gate, multi_ess %.3g relative" % (worst_sum, worst_ess))
    print("plan fixture   shape               batch   sums: worst fraction of the gate   multi_ess      relative deviation   "
          "bound 2 B   cond(Sigma)   (and, on a line of its own, the sums without batches as a fraction of the gate)")
    worst_sum = worst_ess = 0.0
    for name in PLAN_NAMES:
        assert mc.default_batch(mc.PLAN_FIXTURES[name][0]) == mc.PLAN_FIXTURES[name][3]
        frac, e, Xd = row(name, 14)
        plain = sums_fraction(multivariate.moment_sums(Xd, 0), mc.reference(mc.history(name), 0))
        print("%-14s batch 0: %.3g" % (name, plain))
        worst_sum, worst_ess = max(worst_sum, frac, plain), max(worst_ess, e)
    print("worst over the plan fixtures: sums %.3g of their gate, multi_ess %.3g relative" % (worst_sum, worst_ess))


if __name__ == "__main__":
    main()
