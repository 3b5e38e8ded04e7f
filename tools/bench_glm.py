#!/usr/bin/env python
"""Time of the Poisson regression's model criticism (GPU box) on a device history of 1000 x 4096 draws of d = 25 against
n = 1000 rows, and on histories of the same element count at d = 2 and d = 128 (the shapes of profiles/loo_bench.txt):

 (i)   the fused routes as a user calls them: `model.loo(W)` (packing, the five passes of csrc/glm.hip, the finish on
       l2hmc_psis_smooth) and `model.waic(W)`; `model._glm.loo_tails(W)` is the kernels alone plus packing and allocation;
 (ii)  the slow route on the library's own kernels: `model.log_lik(W, rows=...)` in row groups of at most 512 rows and at most
       `--group-bytes` of float32 matrix, each handed to `loo_from_log_lik(select="fused")`;
 (iii) the torch route: the same row groups formed by torch expressions, each handed to `loo_from_log_lik(select="topk")`
       (a float64 copy of the group and a `torch.topk`): groups a quarter as wide;
 (iv)  the yardstick: `predictive.loo_tails` (l2hmc_logistic_loo_tails) on the same draws and rows with binary labels.
(ii) and (iii) are timed on their first `--groups` row groups and scaled to the n rows when those do not cover them (said
on the line).  Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as
many back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.

    python tools/bench_glm.py [--reps 3] [--quick] > profiles/glm_bench.txt

The time of each single pass comes from a kernel trace of one call, summarised by this tool:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_glm.py --once 25
    python tools/bench_glm.py --from-trace DIR/.../*_kernel_trace.csv >> profiles/glm_bench.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import l2hmc_amd
from l2hmc_amd import predictive, psis


def make_case(d, elems, n=1000):
    S = elems // d
    g = torch.Generator(device="cuda").manual_seed(d)
    X = torch.randn((n, d), device="cuda", generator=g) * (0.6 / d ** 0.5)
    w_true = torch.randn(d, device="cuda", generator=g)
    o = torch.rand(n, device="cuda", generator=g) * 2.0 - 0.5
    y = torch.poisson(torch.exp(X @ w_true + o), generator=g)
    W = w_true + 0.1 * torch.randn((S, d), device="cuda", generator=g)               # a posterior-like cloud
    model = l2hmc_amd.PoissonRegression(X.cpu().numpy(), y.cpu().numpy(), offset=o.cpu().numpy())
    return S, W, X, y, o, model


def groups_of(n, S, group_bytes, shrink=1):
    m = max(1, min(512, group_bytes // (4 * S)) // shrink)
    return [(a, min(a + m, n)) for a in range(0, n, m)]


def slow_route(model, W, groups):
    """(ii): elpd_loo_i of the rows of `groups`, each group materialised by l2hmc_glm_log_lik and finished by the fused select."""
    out = []
    for a, b in groups:
        ll = model.log_lik(W, rows=(a, b))
        out.append(psis.loo_from_log_lik(ll, select="fused").elpd_loo_i)
        del ll
    return np.concatenate(out)


def torch_route(W, X, y, o, g, groups):
    """(iii): the same by torch expressions and `torch.topk`."""
    out = []
    for a, b in groups:
        h = W @ X[a:b].T + o[a:b]
        ll = y[a:b] * h - torch.exp(h) - g[a:b]
        del h
        out.append(psis.loo_from_log_lik(ll, select="topk").elpd_loo_i)
        del ll
    return np.concatenate(out)


def once(d, elems):
    """Two `loo_tails` calls of the model and one of the logistic yardstick (for a kernel trace: the second call is the warm one)."""
    S, W, X, y, o, model = make_case(d, elems)
    for _ in range(2):
        t = model._glm.loo_tails(W)
    predictive.loo_tails(W, X, (y > 0).float())
    torch.cuda.synchronize()
    print("traced: draws (%d, %d), n = %d, min n_tail %d" % (S, d, X.shape[0], int(t["n_tail"].min())))


def from_trace(path):
    """Per-dispatch times of the LAST glm `loo_tails` call in a rocprofv3 kernel trace (csv) and of the logistic call after it."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "Kernel_Name" in r]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ours = [r for r in rows if any(k in r["Kernel_Name"] for k in ("loo_", "radix_advance", "chunk_reduce"))]
    starts = [i for i, r in enumerate(ours) if "glm_loo_init_kernel" in r["Kernel_Name"]]
    call = ours[starts[-1]:] if starts else ours
    print("per-dispatch times of one l2hmc_glm_loo_tails call and of l2hmc_logistic_loo_tails on the same draws and rows, from %s"
          % os.path.basename(path))
    totals, which, passes = {"glm": 0.0, "logistic": 0.0}, "glm", {"glm": 0, "logistic": 0}
    for r in call:
        name = r["Kernel_Name"].split("(")[0].replace("l2hmc::", "").replace("void ", "").replace("PoissonLog, ", "")
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "loo_init_kernel" in name and "glm" not in name:
            which = "logistic"
        label = ""
        if "loo_kernel" in name and name.rstrip(">").endswith(", 0"):
            label = "count pass %d" % passes[which]
            passes[which] += 1
        elif "loo_kernel" in name:
            label = "gather pass"
        totals[which] += ms
        print("  %-34s %-14s %9.3f ms" % (name, label, ms))
    print("  sum of the dispatches: glm %.3f ms, logistic %.3f ms" % (totals["glm"], totals["logistic"]))


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


def fmt(ts, scale=1.0):
    return "%10.3f ms (%.3f .. %.3f)" % (1e3 * scale * float(np.median(ts)), 1e3 * scale * min(ts), 1e3 * scale * max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the draws")
    ap.add_argument("--groups", type=int, default=2, help="row groups of (ii) and (iii) that are timed")
    ap.add_argument("--group-bytes", type=int, default=16 << 30)
    ap.add_argument("--dims", type=int, nargs="*", default=[25, 2, 128])
    ap.add_argument("--once", type=int, metavar="D", help="one traced call at dimension D, no timing")
    ap.add_argument("--from-trace", metavar="CSV", help="summarise a rocprofv3 kernel trace of --once")
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace)
    assert torch.cuda.is_available(), "bench_glm needs a GPU"
    elems, n = 1000 * 4096 * 25 // (10 if a.quick else 1), 1000
    if a.once:
        return once(a.once, elems)
    print("library: %s" % os.path.basename(l2hmc_amd._ffi.LIB_PATH))
    for d in a.dims:
        S, W, X, y, o, model = make_case(d, elems, n)
        g = torch.lgamma(y.double() + 1.0).float()
        yb = (y > 0).float()
        print("draws (%d, %d) = %.0f MB, n = %d rows, counts up to %d, tail_len M = %d: S n = %.3g pairs, the matrix %.1f GB"
              % (S, d, W.numel() * 4 / 1e6, n, int(y.max()), predictive.loo_tail_len(S), S * n, S * n * 4 / 1e9))
        gs, gt = groups_of(n, S, a.group_bytes)[:a.groups], groups_of(n, S, a.group_bytes, 4)[:a.groups]
        rows_s, rows_t = gs[-1][1], gt[-1][1]
        s, w = model.loo(W), model.waic(W)
        print("  elpd_loo %.3f (se %.3f), p_loo %.3f, max khat %.3f, n_bad %d;  elpd_waic %.3f, p_waic %.3f"
              % (s.elpd_loo, s.se, s.p_loo, float(np.max(s.khat)), s.n_bad, w.elpd_waic, w.p_waic))
        # results must not change with the route: the slow route gives the fused route's bits, the torch route its numbers
        e_s, e_t = slow_route(model, W, gs), torch_route(W, X, y, o, g, gt)
        print("  max |elpd_loo_i difference| to the fused route: materialised %.3g over %d rows, torch %.3g over %d rows"
              % (np.max(np.abs(e_s - s.elpd_loo_i[:rows_s])), rows_s, np.max(np.abs(e_t - s.elpd_loo_i[:rows_t])), rows_t))
        forms = (("(i)   model.loo", lambda: model.loo(W), 1.0),
                 ("(i)   model.waic", lambda: model.waic(W), 1.0),
                 ("(i)   l2hmc_glm_loo_tails + packing", lambda: model._glm.loo_tails(W), 1.0),
                 ("(ii)  log_lik groups + select=fused, %d of %d rows" % (rows_s, n), lambda: slow_route(model, W, gs), n / rows_s),
                 ("(iii) torch groups + select=topk, %d of %d rows" % (rows_t, n), lambda: torch_route(W, X, y, o, g, gt), n / rows_t),
                 ("(iv)  l2hmc_logistic_loo_tails + packing", lambda: predictive.loo_tails(W, X, yb), 1.0))
        times = {name: [] for name, _, _ in forms}
        for _ in range(a.reps):
            for name, fn, _ in forms:
                times[name].append(measure(fn))
        for name, _, scale in forms:
            print("  %-52s %s%s" % (name, fmt(times[name]), "" if scale == 1.0 else "   scaled to %d rows: %s" % (n, fmt(times[name], scale))))
        med = {name: scale * float(np.median(times[name])) for name, _, scale in forms}
        t_loo, _, t_tails, t_slow, t_torch, t_log = (med[name] for name, _, _ in forms)
        print("  model.loo = x %.2f of the materialised route, x %.2f of the torch route%s;  glm tails = x %.2f of the logistic tails"
              % (t_loo / t_slow, t_loo / t_torch,
                 "" if t_loo < t_slow else "   ** the fused route does NOT beat materialising here **", t_tails / t_log))
        sys.stdout.flush()
        del W


if __name__ == "__main__":
    main()
