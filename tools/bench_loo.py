#!/usr/bin/env python
"""Time of PSIS-LOO (GPU box) on a device history of 1000 x 4096 draws of d = 25 against n = 1000 rows, and on histories of the
same element count at d = 2 and d = 128:

 (i)   `predictive.loo` as a user calls it: packing, the five passes over the history (csrc/loo.hip), the device finish;
 (ii)  `predictive.loo_tails`: the kernels alone plus packing and allocation;
 (iii) `l2hmc_logistic_predict` on the same shape in the same run: one fused contraction pass of the same shape, the yardstick
       (ii) is reported as a multiple of.  It is not a lower bound of a count pass: it spends three transcendentals and four
       float64 additions per (draw, row) pair that a count pass does not, so at small d five passes can cost less than x 5;
 (iv)  the comparison: a chunked torch route on the same GPU -- logits of 65 536 draws at a time, `torch.topk` of the M
       smallest per row merged with the running M.  It is timed on the first `--torch-chunks` chunks and scaled to the whole
       history (its cost per chunk does not change once the running tail is full), and it only finds the tails: no body sums.

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.

    python tools/bench_loo.py [--reps 3] [--quick] > profiles/loo_bench.txt

The time of each single pass comes from a kernel trace of one call, summarised by this tool:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_loo.py --once 25
    python tools/bench_loo.py --from-trace DIR/.../*_kernel_trace.csv >> profiles/loo_bench.txt"""
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


def torch_tails(W, X, sign, M, chunks):
    """The M smallest signed logits per row over the first `chunks` chunks of draws: (M, n)."""
    low = None
    for a in range(0, min(W.shape[0], chunks * TORCH_CHUNK), TORCH_CHUNK):
        t = (W[a:a + TORCH_CHUNK] @ X.T) * sign
        low = t if low is None else torch.cat([low, t])
        if low.shape[0] > M + 1:
            low = torch.topk(low, M + 1, dim=0, largest=False).values
    return low


def make_case(d, elems, n=1000):
    S = elems // d
    g = torch.Generator(device="cuda").manual_seed(d)
    X = torch.randn((n, d), device="cuda", generator=g)
    w_true = torch.randn(d, device="cuda", generator=g) * 0.5
    y = (torch.rand(n, device="cuda", generator=g) < torch.sigmoid(X @ w_true)).float()
    W = w_true + 0.1 * torch.randn((S, d), device="cuda", generator=g)               # a posterior-like cloud
    return S, W, X, y


def once(d, elems):
    """Two `loo_tails` calls and a `waic` on the benchmark's own case (for a kernel trace: the second call is the warm one)."""
    S, W, X, y = make_case(d, elems)
    for _ in range(2):
        t = predictive.loo_tails(W, X, y)
    predictive.waic(W, X, y)
    torch.cuda.synchronize()
    print("traced: draws (%d, %d), n = %d, min n_tail %d" % (S, d, X.shape[0], int(t["n_tail"].min())))


def from_trace(path):
    """Per-dispatch times of the LAST `loo_tails` call in a rocprofv3 kernel trace (csv), in launch order."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "Kernel_Name" in r]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ours = [r for r in rows if any(k in r["Kernel_Name"] for k in ("loo_", "radix_advance", "chunk_reduce", "predict_kernel"))]
    starts = [i for i, r in enumerate(ours) if "loo_init_kernel" in r["Kernel_Name"]]
    call = ours[starts[-1]:] if starts else ours
    print("per-dispatch times of one loo_tails call (and the predict pass of the waic after it), from %s" % os.path.basename(path))
    # (the shared advance and reduce kernels carry no "loo_": the call's dispatches are those before the waic's predict_kernel)
    total, count_pass, in_loo = 0.0, 0, True
    for r in call:
        name = r["Kernel_Name"].split("(")[0].replace("l2hmc::", "").replace("void ", "")
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        label = ""
        if "loo_kernel" in name and name.rstrip(">").endswith(", 0"):
            label = "count pass %d" % count_pass
            count_pass += 1
        elif "loo_kernel" in name:
            label = "gather pass"
        in_loo = in_loo and "predict_kernel" not in name
        if in_loo:
            total += ms
        print("  %-34s %-14s %9.3f ms" % (name, label, ms))
    print("  sum of the loo_tails dispatches: %.3f ms" % total)


def measure(fn, fill=0.25):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    inner = max(1, min(200, int(fill / max(first, 1e-6))))
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
    ap.add_argument("--quick", action="store_true", help="a tenth of the draws")
    ap.add_argument("--torch-chunks", type=int, default=4)
    ap.add_argument("--once", type=int, metavar="D", help="one traced call at dimension D, no timing")
    ap.add_argument("--from-trace", metavar="CSV", help="summarise a rocprofv3 kernel trace of --once")
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace)
    assert torch.cuda.is_available(), "bench_loo needs a GPU"
    elems, n = 1000 * 4096 * 25 // (10 if a.quick else 1), 1000
    if a.once:
        return once(a.once, elems)
    L = _ffi.lib()
    for d in (25, 2, 128):
        S, W, X, y = make_case(d, elems, n)
        M = predictive.loo_tail_len(S)
        sign = 2.0 * y - 1.0
        print("draws (%d, %d) = %.0f MB, n = %d rows, tail_len M = %d: S n = %.3g pairs" % (S, d, W.numel() * 4 / 1e6, n, M, S * n))
        packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device="cuda")
        _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(X.device)))
        ws = torch.empty(_ffi.check(L.l2hmc_logistic_predict_workspace_doubles(S, n, d)), dtype=torch.float64, device="cuda")
        sums = torch.empty((4, n), dtype=torch.float64, device="cuda")

        def predict_only():
            _ffi.check(L.l2hmc_logistic_predict(W.data_ptr(), S, d, packed.data_ptr(), n, sums.data_ptr(), ws.data_ptr(),
                                                _ffi.current_stream(W.device)))

        chunks = min(a.torch_chunks, (S + TORCH_CHUNK - 1) // TORCH_CHUNK)
        forms = (("(i)   predictive.loo", lambda: predictive.loo(W, X, y)),
                 ("(ii)  predictive.loo_tails", lambda: predictive.loo_tails(W, X, y)),
                 ("(iii) l2hmc_logistic_predict alone", predict_only),
                 ("(iv)  torch topk route, %d chunks" % chunks, lambda: torch_tails(W, X, sign, M, chunks)))
        s = predictive.loo(W, X, y)
        w = predictive.waic(W, X, y)
        print("  elpd_loo %.3f (se %.3f), p_loo %.3f, max khat %.3f, n_bad %d, min n_tail %d;  elpd_waic %.3f, p_waic %.3f" % (
            s.elpd_loo, s.se, s.p_loo, float(np.max(s.khat)), s.n_bad, int(s.n_tail.min()), w.elpd_waic, w.p_waic))
        # the two routes agree on the tails of the draws both have seen
        sub = W[:chunks * TORCH_CHUNK]
        if sub.shape[0] >= 2:
            Ms = predictive.loo_tail_len(sub.shape[0])
            mine = predictive.loo_tails(sub, X, y)
            theirs = torch_tails(sub, X, sign, Ms, chunks)
            print("  sub-history of %d draws: cutoff equal to torch's rank-M element on %d of %d rows" % (
                sub.shape[0], int((mine["cutoff"] == torch.sort(theirs, dim=0).values[Ms]).sum()), n))
        for _, fn in forms[1:]:
            fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(measure(fn))
        for name, _ in forms:
            print("  %-42s %s" % (name, fmt(times[name])))
        t_loo, t_tails, t_pred, t_torch = (float(np.median(times[name])) for name, _ in forms)
        scale = ((S + TORCH_CHUNK - 1) // TORCH_CHUNK) / chunks
        print("  loo_tails (five passes) = x %.2f of one predict pass;  finish and the rest of loo: %.3f ms" % (
            t_tails / t_pred, 1e3 * (t_loo - t_tails)))
        print("  torch route scaled to the whole history: %.1f ms = x %.2f of loo_tails%s" % (
            1e3 * t_torch * scale, t_torch * scale / t_tails,
            "" if t_tails < t_torch * scale else "   ** the kernels do NOT beat the torch route here **"))
        sys.stdout.flush()
        del W, ws, packed


if __name__ == "__main__":
    main()
