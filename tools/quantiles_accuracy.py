#!/usr/bin/env python
"""Worst relative deviation of `quantiles.describe`'s `ess_quantile` on the device from the float64 restatement of
tests/quantiles_case.py (np.quantile, the indicator history, the estimator of tests/diagnostics_case.py chain by chain), over
the six AR(1) fixtures, split and unsplit, at p = 0.05, 0.5, 0.95 -- the figure tests/test_gpu_quantiles.py quotes as
ESS_QUANTILE_MEASURED.  Also: whether the quantiles equal np.quantile bit for bit and how many stopping indices differ.

    python tools/quantiles_accuracy.py > profiles/quantiles_accuracy.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

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


if __name__ == "__main__":
    main()
