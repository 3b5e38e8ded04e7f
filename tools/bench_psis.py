#!/usr/bin/env python
"""Time of the PSIS kernels (GPU box) at the three shapes of profiles/loo_bench.txt -- a device history of 1000 x 4096 draws of
d = 25 against n = 1000 rows, and histories of the same element count at d = 2 and d = 128 -- in one run:

 (i)   `predictive.loo(finish="torch")`: today's default, the float64 Pareto profile as chunked torch;
 (ii)  `predictive.loo(finish="kernel")`: the same tails finished on csrc/psis.hip;
 (iii) `predictive.loo_tails` alone: what both share;
 (iv)  `l2hmc_psis_smooth` alone on the prepared float64 tails of the same case (buffers allocated once), and its log1p per
       second: a row of tail length L evaluates (30 + floor(sqrt L) + 1) L of them for the profile and the mean at theta_hat,
       and 2 L more in the two smoothing passes.

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.

    python tools/bench_psis.py [--reps 3] [--quick] > profiles/psis_bench.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_loo import fmt, make_case, measure
from l2hmc_amd import _ffi, _pareto, predictive


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the draws")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_psis needs a GPU"
    elems, n = 1000 * 4096 * 25 // (10 if a.quick else 1), 1000
    L = _ffi.lib()
    slower = []
    for d in (25, 2, 128):
        S, W, X, y = make_case(d, elems, n)
        M = predictive.loo_tail_len(S)
        print("draws (%d, %d) = %.0f MB, n = %d rows, tail_len M = %d" % (S, d, W.numel() * 4 / 1e6, n, M))
        tails = predictive.loo_tails(W, X, y)
        xp = _pareto._Torch()
        _, _, lam_c, lam = predictive._loo_prepare(xp, tails["cutoff"], tails["n_tail"], tails["tail"])
        lam, lam_c, n_tail = lam.contiguous(), lam_c.contiguous(), tails["n_tail"].contiguous()
        ws = torch.empty(_ffi.check(L.l2hmc_psis_workspace_bytes(n, M)), dtype=torch.uint8, device="cuda")
        out = torch.empty((3, n), dtype=torch.float64, device="cuda")

        def kernel_only():
            _ffi.check(L.l2hmc_psis_smooth(lam.data_ptr(), n_tail.data_ptr(), lam_c.data_ptr(), n, M, out.data_ptr(), None,
                                           ws.data_ptr(), _ffi.current_stream(lam.device)))

        forms = (('(i)   predictive.loo(finish="torch")', lambda: predictive.loo(W, X, y)),
                 ('(ii)  predictive.loo(finish="kernel")', lambda: predictive.loo(W, X, y, finish="kernel")),
                 ("(iii) predictive.loo_tails", lambda: predictive.loo_tails(W, X, y)),
                 ("(iv)  l2hmc_psis_smooth alone", kernel_only))
        st, sk = predictive.loo(W, X, y), predictive.loo(W, X, y, finish="kernel")
        print("  finish=torch: elpd_loo %.6f, max khat %.6f, n_bad %d;  finish=kernel: elpd_loo %.6f, max khat %.6f, n_bad %d" % (
            st.elpd_loo, float(np.max(st.khat)), st.n_bad, sk.elpd_loo, float(np.max(sk.khat)), sk.n_bad))
        print("  kernel - torch: max |d khat| %.3g, max |d elpd_loo_i| %.3g" % (
            float(np.max(np.abs(sk.khat - st.khat))), float(np.max(np.abs(sk.elpd_loo_i - st.elpd_loo_i)))))
        for _, fn in forms:
            fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(measure(fn))
        for name, _ in forms:
            print("  %-42s %s" % (name, fmt(times[name])))
        t_torch, t_kernel, t_tails, t_smooth = (float(np.median(times[name])) for name, _ in forms)
        Lh = n_tail.cpu().numpy().astype(np.float64)
        fitted = Lh >= predictive.MIN_TAIL_FIT
        log1ps = float(np.sum(np.where(fitted, (30.0 + np.floor(np.sqrt(Lh)) + 1.0) * Lh, 0.0) + 2.0 * Lh))
        print("  the finish and the rest of loo: torch %.3f ms, kernel %.3f ms (of which l2hmc_psis_smooth %.3f ms)" % (
            1e3 * (t_torch - t_tails), 1e3 * (t_kernel - t_tails), 1e3 * t_smooth))
        print("  l2hmc_psis_smooth: %.3g log1p in %.3f ms = %.3g log1p per second" % (log1ps, 1e3 * t_smooth, log1ps / t_smooth))
        print("  loo(finish=\"kernel\") = x %.2f of loo(finish=\"torch\")%s" % (
            t_kernel / t_torch, "" if t_kernel < t_torch else "   ** the kernel route is NOT faster here **"))
        if t_kernel >= t_torch:
            slower.append(d)
        sys.stdout.flush()
        del W, ws, lam, tails
    print("the kernel route is faster at every shape" if not slower else "the kernel route is NOT faster at d = %s" % slower)


if __name__ == "__main__":
    main()
