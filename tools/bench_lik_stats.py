#!/usr/bin/env python
"""Time of `predictive.relative_eff` (GPU box) on the three 410 MB device histories of profiles/loo_bench.txt -- 4096 chains x
{1000 steps of d = 25, 12500 of d = 2, 195 of d = 128} -- against n = 1000 rows, at max_lag 31 and 255:

 (i)   `predictive.relative_eff` as a user calls it: packing the rows, the kernels (csrc/lik_stats.hip), the (chains, n)
       moments reduced on the device, the (n, max_lag + 1) lag sums to the host, the host finish;
 (ii)  `l2hmc_logistic_lik_stats` alone (packed rows, workspace and outputs allocated once);
 (iii) the comparisons: one `l2hmc_logistic_predict` pass over the same history (one contraction pass, the unit the cost of
       (ii) is counted in) and `predictive.loo` of the same draws without and with `r_eff="auto"` (both finishes).

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.

    python tools/bench_lik_stats.py [--reps 3] [--quick] > profiles/lik_stats_bench.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import _ffi, predictive


def measure(fn):
    """Seconds per call of as many back-to-back calls as fill 0.25 s."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    inner = max(1, min(200, int(0.25 / max(first, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def fmt(ts):
    return "%10.3f ms (%.3f .. %.3f)" % (1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="the d = 25 history only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lik_stats needs a GPU"
    chains, n = 4096, 1000
    print("$ python tools/bench_lik_stats.py " + " ".join(sys.argv[1:]) + "        (" + torch.cuda.get_device_name() + ")")
    shapes = [(1000, 25)] if a.quick else [(1000, 25), (12500, 2), (195, 128)]
    L = _ffi.lib()
    for M, d in shapes:
        g = torch.Generator(device="cuda").manual_seed(M + d)
        X = torch.randn((n, d), device="cuda", generator=g)
        w_true = torch.randn(d, device="cuda", generator=g) * 0.5
        y = (torch.rand(n, device="cuda", generator=g) < torch.sigmoid(X @ w_true)).float()
        hist = torch.empty((M, chains, d), device="cuda")      # AR(1) chains, rho = 0.7, about a posterior-like cloud
        hist[0] = torch.randn((chains, d), device="cuda", generator=g)
        for t in range(1, M):
            hist[t] = 0.7 * hist[t - 1] + (1 - 0.49) ** 0.5 * torch.randn((chains, d), device="cuda", generator=g)
        hist = w_true + 0.1 * hist
        S = M * chains
        print("history (%d, %d, %d) = %.0f MB, n = %d rows: S n = %.3g pairs" % (M, chains, d, hist.numel() * 4 / 1e6, n, S * n))
        packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device="cuda")
        _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(X.device)))
        pws = torch.empty(_ffi.check(L.l2hmc_logistic_predict_workspace_doubles(S, n, d)), dtype=torch.float64, device="cuda")
        psums = torch.empty((4, n), dtype=torch.float64, device="cuda")

        def predict_pass():
            _ffi.check(L.l2hmc_logistic_predict(hist.data_ptr(), S, d, packed.data_ptr(), n, psums.data_ptr(), pws.data_ptr(),
                                                _ffi.current_stream(hist.device)))

        times = {}
        for max_lag in (31, 255):
            if max_lag > M - 1:
                print("  max_lag %3d: not run, the history has %d steps" % (max_lag, M))
                continue
            ws = torch.empty(_ffi.check(L.l2hmc_logistic_lik_stats_workspace_bytes(M, chains, d, n, max_lag, 0)), dtype=torch.uint8,
                             device="cuda")
            mean = torch.empty((chains, n), dtype=torch.float64, device="cuda")
            m2 = torch.empty((chains, n), dtype=torch.float64, device="cuda")
            G = torch.empty((n, max_lag + 1), dtype=torch.float64, device="cuda")

            def kernel_only(max_lag=max_lag, ws=ws, mean=mean, m2=m2, G=G):
                _ffi.check(L.l2hmc_logistic_lik_stats(hist.data_ptr(), M, chains, d, packed.data_ptr(), n, max_lag, 0, mean.data_ptr(),
                                                      m2.data_ptr(), G.data_ptr(), ws.data_ptr(), _ffi.current_stream(hist.device)))

            s = predictive.relative_eff(hist, X, y, max_lag=max_lag)
            print("  max_lag %3d: r_eff %.3f .. %.3f, %d truncated, %d NaN" % (max_lag, np.nanmin(s.r_eff), np.nanmax(s.r_eff),
                                                                            s.n_truncated, s.n_nan))
            times["(i)   predictive.relative_eff, max_lag %d" % max_lag] = (lambda max_lag=max_lag: predictive.relative_eff(hist, X, y, max_lag=max_lag), [])
            times["(ii)  l2hmc_logistic_lik_stats alone, max_lag %d" % max_lag] = (kernel_only, [])
        times["(iii) l2hmc_logistic_predict alone (one contraction pass)"] = (predict_pass, [])
        times["(iii) predictive.loo"] = (lambda: predictive.loo(hist, X, y), [])
        times["(iii) predictive.loo, finish=kernel"] = (lambda: predictive.loo(hist, X, y, finish="kernel"), [])
        times["(iii) predictive.loo, r_eff=auto"] = (lambda: predictive.loo(hist, X, y, r_eff="auto"), [])
        times["(iii) predictive.loo, r_eff=auto, finish=kernel"] = (lambda: predictive.loo(hist, X, y, r_eff="auto", finish="kernel"), [])
        o = predictive.loo(hist, X, y, r_eff="auto", finish="kernel")
        print("  loo(r_eff=auto): elpd_loo %.3f (se %.3f, mcse %.4f), min n_eff %.0f, tail lengths %d .. %d against %d" % (
            o.elpd_loo, o.se, o.mcse_elpd_loo, o.min_n_eff, o.tail_len_row.min(), o.tail_len_row.max(), predictive.loo_tail_len(S)))
        for fn, _ in times.values():
            fn()
        for _ in range(a.reps):
            for fn, ts in times.values():
                ts.append(measure(fn))
        for name, (_, ts) in times.items():
            print("  %-58s %s" % (name, fmt(ts)))
        tp = float(np.median(times["(iii) l2hmc_logistic_predict alone (one contraction pass)"][1]))
        for name, (_, ts) in times.items():
            if name.startswith("(ii) "):
                print("  %s = x %.1f of one predict pass" % (name[6:], float(np.median(ts)) / tp))
        sys.stdout.flush()
        del hist, pws, packed


if __name__ == "__main__":
    main()
