#!/usr/bin/env python
"""Time of the convergence diagnostics (GPU box) on AR(1) histories of the logistic-regression example's shape (400, 4096, 25)
and of (2000, 65536, 2):

 (i)   `diagnostics.summarize` on the device history (split, default max_lag): two kernel passes, the fold, the host finish;
 (ii)  what it replaces: the device-to-host copy of the second half of the history and examples/logistic_regression.py's former
       `min_ess` (numpy loops over coordinates and lags; restated below);
 (iii) the per-product yardstick: `l2hmc_autocov` (every lag 0 .. steps - 2, all series in one number) against the new kernels
       with max_lag = steps - 2, unsplit, which form the same lags per coordinate -- both as products (series * sum over lags
       of the steps that lag pairs) per second.

Every figure: one warm-up call, then `--reps` calls, each ended by a device synchronise; median and the min .. max spread.

    python tools/bench_diagnostics.py [--reps 7] [--quick]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import diagnostics, func_utils


def host_min_ess(hist):
    """examples/logistic_regression.py `min_ess` before `diagnostics.summarize` replaced it."""
    h = hist - hist.mean(axis=(0, 1), keepdims=True)
    M = h.shape[0]
    out = []
    for k in range(h.shape[2]):
        z = h[:, :, k]
        var = (z * z).mean()
        rho = [1.0]
        for t in range(1, M // 2):
            r = (z[:-t] * z[t:]).mean() / var
            if r < 0.05:
                break
            rho.append(r)
        tau = 1.0 + 2.0 * sum(rho[1:])
        out.append(M * h.shape[1] / tau)
    return float(min(out))


def ar1_device(M, N, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    phi = torch.linspace(0.0, 0.95, d, device="cuda")
    mean, sd = torch.linspace(-2.0, 2.0, d, device="cuda"), torch.linspace(0.02, 1.0, d, device="cuda")
    X = torch.empty((M, N, d), device="cuda")
    x = torch.randn((N, d), device="cuda", generator=g)
    for t in range(M):
        if t:
            x = phi * x + torch.sqrt(1 - phi * phi) * torch.randn((N, d), device="cuda", generator=g)
        X[t] = mean + sd * x
    return X


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def fmt(t):
    return "%9.3f ms (%.3f .. %.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the example's shape only")
    a = ap.parse_args()
    shapes = [(400, 4096, 25)] + ([] if a.quick else [(2000, 65536, 2)])
    for M, N, d in shapes:
        X = ar1_device(M, N, d, seed=M + d)
        print("history (%d, %d, %d): %.1f MB" % (M, N, d, X.numel() * 4 / 1e6))
        s = diagnostics.summarize(X)
        print("  (i)   summarize, split, max_lag %d:            %s   [max rhat %.4f, min ess %.0f]" % (
            s.max_lag, fmt(timed(lambda: diagnostics.summarize(X), a.reps)), s.max_rhat, s.min_ess))
        half = X[M // 2:]
        sh = diagnostics.summarize(half)
        print("        the same on the second half (the example):  %s   [min ess %.0f]" % (
            fmt(timed(lambda: diagnostics.summarize(half), a.reps)), sh.min_ess))
        reps_host = max(2, a.reps // 3)
        t_copy = timed(lambda: half.cpu().numpy().astype(np.float64), reps_host)
        hh = half.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        e = host_min_ess(hh)
        t_host = time.perf_counter() - t0
        print("  (ii)  device-to-host copy of the second half:    %s" % fmt(t_copy))
        print("        host min_ess on it (one run):               %9.3f ms   [min ess %.0f]" % (1e3 * t_host, e))
        del hh
        series = N * d
        lags = M - 1                                                     # 0 .. M - 2
        products = series * sum(M - t for t in range(lags))
        t_old = timed(lambda: func_utils.device_autocov(X), a.reps)
        t_new = timed(lambda: diagnostics.chain_sums(X, max_lag=M - 2, split=False), a.reps)
        print("  (iii) l2hmc_autocov, %d lags:                  %s   %.3g products/s" % (lags, fmt(t_old), products / t_old[0]))
        print("        l2hmc_chain_stats, the same lags, unsplit:  %s   %.3g products/s   (x %.2f)" % (
            fmt(t_new), products / t_new[0], t_old[0] / t_new[0]))
        sys.stdout.flush()
        del X, half


if __name__ == "__main__":
    main()
