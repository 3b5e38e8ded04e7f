#!/usr/bin/env python
"""Time of `predictive.waic` (GPU box) on a device history of 4096 chains x {100, 1000} recorded proposals against n = 1000
and n = 4096 rows of d = 25 features:

 (i)   `predictive.waic` as a user calls it: packing the rows, the kernel (csrc/predictive.hip), the (4, n) sums to the host,
       the host finish;
 (ii)  `l2hmc_logistic_predict` alone (packed rows, workspace and output allocated once): the kernel and its small reduction,
       with the rates the shapes imply -- 2 S n d flops of the contraction and 3 S n transcendentals (exp, reciprocal, log);
 (iii) the comparison: the same four sums from a chunked torch expression on the same GPU -- `draws @ X.T`, sigmoid,
       logsigmoid, running float64 sums, 65 536 draws at a time so that the (draws, rows) temporaries stay near 1 GB.

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many back-to-back
calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.  The two forms'
numbers are compared before they are timed.

    python tools/bench_predictive.py [--reps 5] [--quick] > profiles/predictive_bench.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import _ffi, predictive

TORCH_CHUNK = 65536


def torch_sums(W, X, sign):
    """The comparison: (4, n) float64 sums from torch expressions, a chunk of draws at a time."""
    n = X.shape[0]
    out = torch.zeros((4, n), dtype=torch.float64, device=W.device)
    for a in range(0, W.shape[0], TORCH_CHUNK):
        L = W[a:a + TORCH_CHUNK] @ X.T
        ll = torch.nn.functional.logsigmoid(L * sign)
        out[0] += torch.sigmoid(L).sum(dim=0, dtype=torch.float64)
        out[1] += torch.exp(ll).sum(dim=0, dtype=torch.float64)
        lld = ll.double()
        out[2] += lld.sum(dim=0)
        out[3] += (lld * lld).sum(dim=0)
    return out


def torch_waic(W, X, sign):
    s = torch_sums(W, X, sign).cpu().numpy()
    return predictive.finish({"sum_p": s[0], "sum_lik": s[1], "sum_ll": s[2], "sum_ll2": s[3], "n_draws": W.shape[0]})


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
    return "%9.3f ms (%.3f .. %.3f)" % (1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100 proposals, n = 1000 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predictive needs a GPU"
    chains, d = 4096, 25
    shapes = [(100, 1000)] if a.quick else [(100, 1000), (1000, 1000), (100, 4096), (1000, 4096)]
    L = _ffi.lib()
    for M, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(M + n)
        X = torch.randn((n, d), device="cuda", generator=g)
        w_true = torch.randn(d, device="cuda", generator=g) * 0.5
        y = (torch.rand(n, device="cuda", generator=g) < torch.sigmoid(X @ w_true)).float()
        hist = w_true + 0.1 * torch.randn((M, chains, d), device="cuda", generator=g)      # a posterior-like cloud
        S = M * chains
        W, sign = hist.reshape(S, d), 2.0 * y - 1.0
        print("history (%d, %d, %d) = %.0f MB, n = %d rows: S n = %.3g pairs" % (M, chains, d, hist.numel() * 4 / 1e6, n, S * n))

        packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device="cuda")
        _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(X.device)))
        ws = torch.empty(_ffi.check(L.l2hmc_logistic_predict_workspace_doubles(S, n, d)), dtype=torch.float64, device="cuda")
        sums = torch.empty((4, n), dtype=torch.float64, device="cuda")

        def kernel_only():
            _ffi.check(L.l2hmc_logistic_predict(W.data_ptr(), S, d, packed.data_ptr(), n, sums.data_ptr(), ws.data_ptr(),
                                                _ffi.current_stream(W.device)))

        forms = (("(i)   predictive.waic", lambda: predictive.waic(hist, X, y)),
                 ("(ii)  l2hmc_logistic_predict alone", kernel_only),
                 ("(iii) chunked torch expression + finish", lambda: torch_waic(W, X, sign)))
        mine, theirs = predictive.waic(hist, X, y), torch_waic(W, X, sign)          # (also the warm-up of (i) and (iii))
        kernel_only()
        print("  elpd_waic %.4f (kernel) %.4f (torch); p_waic %.4f %.4f; worst |d elpd_i| %.2e" % (
            mine.elpd_waic, theirs.elpd_waic, mine.p_waic, theirs.p_waic, np.max(np.abs(mine.elpd_i - theirs.elpd_i))))
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(measure(fn))
        for name, _ in forms:
            print("  %-42s %s" % (name, fmt(times[name])))
        tk, tt, tw = (float(np.median(times[name])) for name in (forms[1][0], forms[2][0], forms[0][0]))
        print("  (ii) as rates: %.3g contraction flop/s, %.3g transcendentals/s, history read at %.3g B/s per pass" % (
            2.0 * S * n * d / tk, 3.0 * S * n / tk, 4.0 * S * d / tk))
        print("  torch / waic = x %.2f;  torch / kernel alone = x %.2f%s" % (
            tt / tw, tt / tk, "" if tw < tt else "   ** the kernel path does NOT beat the torch form here **"))
        sys.stdout.flush()
        del hist, W, ws, packed


if __name__ == "__main__":
    main()
