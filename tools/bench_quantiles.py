#!/usr/bin/env python
"""Time of the posterior-quantile path (GPU box) on a device history of 1000 proposals x 4096 chains x 25 coordinates
(410 MB) and on d = 2 and d = 128 with the same element count:

 (i)   `quantiles.describe` as a user calls it (summarize's sums, the quantile select, one indicator chain-sums call per
       quantile, the MCSE select, the host finish);
 (ii)  `l2hmc_order_stats` alone at the 6 ranks of three quantiles (ranks, workspace and outputs allocated once);
 (iii) the torch route: `torch.sort` of the (S, d) view along dim 0, then indexing (a second copy of the history, and the
       int64 index tensor torch.sort returns with it);
 (iv)  one plain read of the history, `X.sum()`: the bandwidth unit.

(ii) is reported as a multiple of (iv) next to its floor -- one read of the history per pass and coordinate / rank group.
Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.
The two routes' order statistics are compared before they are timed.  L2HMC_ORDER_STATS_RUNS=1 in the environment selects the
run-counting variant of the pass-0 count kernel.

    python tools/bench_quantiles.py [--reps 5] [--quick] > profiles/quantiles_bench.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import _ffi, quantiles

PROBS = (0.05, 0.5, 0.95)


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


def groups(d, R, p):
    """Reads of the history in count pass p: the plan of csrc/order_stats.hip restated (64 (coordinate, rank) pairs per group)."""
    best = None
    rg = 1
    while True:
        sg = min(d, 64 // rg)
        n = -(-d // sg) * (1 if p == 0 else -(-R // rg))
        best = n if best is None or n < best else best
        if p == 0 or rg >= R or rg >= 32:
            return best
        rg *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100 proposals only")
    ap.add_argument("--no-describe", action="store_true", help="skip (i)")
    ap.add_argument("--dims", default="25,2,128", help="the coordinate counts to run (a kernel trace of one shape)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quantiles needs a GPU"
    L = _ffi.lib()
    passes = L.l2hmc_order_stats_passes()
    M, N = (100 if a.quick else 1000), 4096
    print("count variant of pass 0: %s" % ("runs counted in a register (L2HMC_ORDER_STATS_RUNS=1)"
                                           if os.environ.get("L2HMC_ORDER_STATS_RUNS", "0") not in ("", "0") else "one LDS atomic per draw"))
    for d in (int(v) for v in a.dims.split(",")):
        n = N * 25 // d                                                   # the same element count
        g = torch.Generator(device="cuda").manual_seed(d)
        hist = torch.randn((M, n, d), device="cuda", generator=g) * torch.linspace(0.1, 3.0, d, device="cuda") + 0.5
        S = M * n
        X2 = hist.view(S, d)
        lo, hi, _ = quantiles._quantile_ranks(S, np.array(PROBS))
        ranks = np.repeat(np.concatenate([lo, hi])[:, None], d, axis=1)
        R = ranks.shape[0]
        reads = sum(groups(d, R, p) for p in range(passes))
        print("history (%d, %d, %d) = %.0f MB, %d ranks: %d passes of %d bins, %d reads of the history (groups per pass %s)" % (
            M, n, d, hist.numel() * 4 / 1e6, R, passes, L.l2hmc_order_stats_bins(), reads, [groups(d, R, p) for p in range(passes)]))
        rk = torch.as_tensor(ranks).cuda()
        ws = torch.empty(_ffi.check(L.l2hmc_order_stats_workspace_bytes(d, R)), dtype=torch.uint8, device="cuda")
        values = torch.empty((R, d), dtype=torch.float32, device="cuda")
        n_nan = torch.empty(d, dtype=torch.int64, device="cuda")

        def select_only():
            _ffi.check(L.l2hmc_order_stats(X2.data_ptr(), S, d, rk.data_ptr(), R, values.data_ptr(), n_nan.data_ptr(),
                                           ws.data_ptr(), _ffi.current_stream(X2.device)))

        def torch_route():
            return torch.sort(X2, dim=0)[0][rk[:, 0]]

        forms = [("(ii)  l2hmc_order_stats alone", select_only), ("(iii) torch.sort + indexing", torch_route),
                 ("(iv)  X.sum(), one read", lambda: hist.sum())]
        if not a.no_describe:
            forms.insert(0, ("(i)   quantiles.describe", lambda: quantiles.describe(hist, PROBS)))
        select_only()
        theirs = torch_route()
        print("  order statistics equal torch.sort's: %s" % bool(torch.equal(values, theirs)))
        del theirs
        for _, fn in forms:
            fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(measure(fn))
        for name, _ in forms:
            print("  %-34s %s" % (name, fmt(times[name])))
        med = {name[:5].strip(): float(np.median(times[name])) for name, _ in forms}
        print("  (ii) = x %.2f of one read (iv); floor = %d reads: x %.2f of its floor; history read at %.3g B/s per read; "
              "torch.sort / (ii) = x %.1f" % (med["(ii)"] / med["(iv)"], reads, med["(ii)"] / (reads * med["(iv)"]),
                                               reads * 4.0 * S * d / med["(ii)"], med["(iii)"] / med["(ii)"]))
        sys.stdout.flush()
        del hist, X2, ws


if __name__ == "__main__":
    main()
