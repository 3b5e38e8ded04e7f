#!/usr/bin/env python
"""Time of `multivariate.multi_ess` (GPU box) on a device history of 1000 proposals x 4096 chains x 25 coordinates (410 MB)
and on d = 2 and d = 128 with the same element count -- the shapes of profiles/quantiles_bench.txt:

 (i)   `multivariate.multi_ess` as a user calls it (workspace and outputs allocated, the kernels, 2 (d + d^2) numbers to the
       host, the float64 finish);
 (ii)  `l2hmc_moment_sums` alone (workspace and outputs allocated once);
 (iii) the route a user has without it: a float64 copy of the history, centring, Z^T Z, and the same on the reshaped batch
       means, in torch;
 (iv)  one plain read of the history, `X.sum()`: the floor.

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.
The two routes' multi_ess are compared before they are timed; the kernels' register counts come from the compiler's listing.

    python tools/bench_multivariate.py [--reps 5] [--quick] > profiles/multivariate_bench.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from l2hmc_amd import _ffi, multivariate


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


def torch_route(hist, b):
    """Lambda, Sigma and multi_ess the way a user computes them today (everything on the device, float64)."""
    M, N, d = hist.shape
    X = hist.double()
    n = M * N
    mu = X.reshape(n, d).mean(dim=0)
    Z = X.reshape(n, d) - mu
    lam = Z.T @ Z / (n - 1)
    a = M // b
    Y = X[M - a * b:].reshape(a, b, N, d).mean(dim=1).reshape(a * N, d) - mu
    sig = b * (Y.T @ Y) / (a * N - 1)
    return float(n * torch.exp((torch.linalg.slogdet(lam)[1] - torch.linalg.slogdet(sig)[1]) / d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100 proposals only")
    ap.add_argument("--dims", default="25,2,128", help="the coordinate counts to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_multivariate needs a GPU"
    L = _ffi.lib()
    M, N = (100 if a.quick else 1000), 4096
    try:
        import kernel_resources as kr
        for k, vg, sc, acc in kr.resources().get("moment_sums.s", []):
            print("registers  %-36s %4d (accumulation registers from %d), scratch %d" % (k, vg, acc, sc))
    except Exception as exc:                                              # no listings here: the library was built elsewhere
        print("registers  (no compiler listing: %s)" % exc)
    for d in (int(v) for v in a.dims.split(",")):
        n = N * 25 // d                                                   # the same element count
        g = torch.Generator(device="cuda").manual_seed(d)
        hist = torch.randn((M, n, d), device="cuda", generator=g) * torch.linspace(0.1, 3.0, d, device="cuda") + 0.5
        b = multivariate.default_batch_size(M)
        ws = torch.empty(_ffi.check(L.l2hmc_moment_sums_workspace_doubles(M, n, d, b)), dtype=torch.float64, device="cuda")
        out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in (d, d * d, d, d * d)]
        print("history (%d, %d, %d) = %.0f MB, batch %d, workspace %.1f MB" % (M, n, d, hist.numel() * 4 / 1e6, b,
                                                                              ws.numel() * 8 / 1e6))

        def sums_only():
            _ffi.check(L.l2hmc_moment_sums(hist.data_ptr(), M, n, d, b, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(),
                                           _ffi.current_stream(hist.device)))

        forms = [("(i)   multivariate.multi_ess", lambda: multivariate.multi_ess(hist)),
                 ("(ii)  l2hmc_moment_sums alone", sums_only),
                 ("(iii) torch: float64 copy, Z^T Z", lambda: torch_route(hist, b)),
                 ("(iv)  X.sum(), one read", lambda: hist.sum())]
        ours, theirs = multivariate.multi_ess(hist).multi_ess, torch_route(hist, b)
        print("  multi_ess %.6g, torch route %.6g: relative difference %.3g" % (ours, theirs, abs(ours - theirs) / theirs))
        for _, fn in forms:
            fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(measure(fn))
        for name, _ in forms:
            print("  %-34s %s" % (name, fmt(times[name])))
        med = {name[:5].strip(): float(np.median(times[name])) for name, _ in forms}
        print("  (ii) = x %.2f of one read (iv), history read at %.3g B/s; (i) = x %.2f of (iv); torch route / (i) = x %.1f" % (
            med["(ii)"] / med["(iv)"], 4.0 * hist.numel() / med["(ii)"], med["(i)"] / med["(iv)"], med["(iii)"] / med["(i)"]))
        sys.stdout.flush()
        del hist, ws


if __name__ == "__main__":
    main()
