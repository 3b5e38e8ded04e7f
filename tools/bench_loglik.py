#!/usr/bin/env python
"""Time of PSIS-LOO of a generic log-likelihood matrix on the device (GPU box), fused selection against `torch.topk`, at three
float32 shapes -- 409 600 x 256, 4 096 000 x 32 and 40 960 x 2048 (four column groups) -- in one run:

 (i)    `psis.loo_from_log_lik(select="topk")`: the default route, unchanged by the fused one: the baseline;
 (ii)   `psis.loo_from_log_lik(select="fused")`;
 (iii)  `psis.loo_from_log_lik(select="fused", r_eff=...)`: per-column tails, n_eff and the Monte Carlo SE;
 (iv)   `l2hmc_loglik_tails` alone on the first column group (buffers allocated once): select, gather, reduce;
 (v)    `l2hmc_order_stats` alone with the same two ranks per column: (iv) - (v) is the gather pass with its init and reduce;
 (vi)   `ll.sum()` of the same group: a plain read of the matrix, the memory bound of one pass;
 (vii)  `psis.relative_eff_from_log_lik` at max_lag = 31, (viii) at the default max_lag, on the history form (steps, 1024, n).

Every figure: one warm-up call of each form, then `--reps` rounds that alternate the forms; a measurement is as many
back-to-back calls as fill a quarter of a second, ended by a device synchronise; median per call and the min .. max spread.
The fused and the topk results are compared on the same matrix before anything is timed.

    python tools/bench_loglik.py [--reps 3] [--quick] > profiles/loglik_bench.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_loo import fmt, measure
from l2hmc_amd import _ffi, psis
from l2hmc_amd._pareto import loo_tail_len

CHAINS = 1024


def make(steps, n, seed):
    """(steps, CHAINS, n) float32 on the device: -softplus of Gaussian logits whose scale grows with the column."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = (0.5 + 1.5 * torch.arange(n, device="cuda") / max(n - 1, 1)).float()
    t = torch.randn((steps, CHAINS, n), generator=g, device="cuda") * scale + 1.0
    return -torch.nn.functional.softplus(-t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the draws")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loglik needs a GPU"
    L = _ffi.lib()
    q = 10 if a.quick else 1
    for steps, n in ((400 // q, 256), (4000 // q, 32), (40, 2048 // q)):
        hist = make(steps, n, 11 + n)
        S = steps * CHAINS
        ll = hist.reshape(S, n)
        M = loo_tail_len(S)
        print("log_lik (%d, %d) float32 = %.0f MB, history form (%d, %d, %d), tail_len M = %d" % (S, n, ll.numel() * 4 / 1e6, steps,
                                                                                             CHAINS, n, M))
        m = min(n, psis.MAX_DEVICE_COLS)
        block = ll[:, :m].contiguous() if m < n else ll
        dev = ll.device
        ws = torch.empty(_ffi.check(L.l2hmc_loglik_tails_workspace_bytes(S, m)), dtype=torch.uint8, device=dev)
        cutoff, top = (torch.empty(m, dtype=torch.float32, device=dev) for _ in range(2))
        n_tail = torch.empty(m, dtype=torch.int64, device=dev)
        tail = torch.empty((m, M), dtype=torch.float32, device=dev)
        sums = torch.empty((3, m), dtype=torch.float64, device=dev)
        ranks = torch.tensor([[M] * m, [S - 1] * m], dtype=torch.int64, device=dev)
        vals = torch.empty((2, m), dtype=torch.float32, device=dev)
        nn = torch.empty(m, dtype=torch.int64, device=dev)
        ws2 = torch.empty(_ffi.check(L.l2hmc_order_stats_workspace_bytes(m, 2)), dtype=torch.uint8, device=dev)
        stream = _ffi.current_stream(dev)

        def entry():
            _ffi.check(L.l2hmc_loglik_tails(block.data_ptr(), S, m, None, M, cutoff.data_ptr(), top.data_ptr(), n_tail.data_ptr(),
                                            tail.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), stream))

        def select():
            _ffi.check(L.l2hmc_order_stats(block.data_ptr(), S, m, ranks.data_ptr(), 2, vals.data_ptr(), nn.data_ptr(),
                                           ws2.data_ptr(), stream))

        r = np.linspace(0.15, 1.1, n)
        lag31 = min(31, steps - 1)
        forms = (('(i)    loo_from_log_lik(select="topk")', lambda: psis.loo_from_log_lik(ll)),
                 ('(ii)   loo_from_log_lik(select="fused")', lambda: psis.loo_from_log_lik(ll, select="fused")),
                 ('(iii)  loo_from_log_lik(select="fused", r_eff)', lambda: psis.loo_from_log_lik(ll, select="fused", r_eff=r)),
                 ("(iv)   l2hmc_loglik_tails, %d columns" % m, entry),
                 ("(v)    l2hmc_order_stats, 2 ranks, %d columns" % m, select),
                 ("(vi)   ll.sum(), %d columns" % m, lambda: block.sum()),
                 ("(vii)  relative_eff_from_log_lik(max_lag=%d)" % lag31, lambda: psis.relative_eff_from_log_lik(hist, max_lag=lag31)),
                 ("(viii) relative_eff_from_log_lik(default max_lag)", lambda: psis.relative_eff_from_log_lik(hist)))
        st, sf = psis.loo_from_log_lik(ll), psis.loo_from_log_lik(ll, select="fused")
        print("  topk: elpd_loo %.6f, max khat %.6f, n_bad %d;  fused: elpd_loo %.6f, max khat %.6f, n_bad %d;  n_tail equal: %s, "
              "max |d elpd_loo_i| %.3g, max |d khat| %.3g" % (st.elpd_loo, float(np.max(st.khat)), st.n_bad, sf.elpd_loo,
                                                           float(np.max(sf.khat)), sf.n_bad, np.array_equal(st.n_tail, sf.n_tail),
                                                           float(np.max(np.abs(st.elpd_loo_i - sf.elpd_loo_i))),
                                                           float(np.max(np.abs(st.khat - sf.khat)))))
        for _, fn in forms:
            fn()
        times = [[] for _ in forms]
        for _ in range(a.reps):
            for k, (_, fn) in enumerate(forms):
                times[k].append(measure(fn))
        for (name, _), ts in zip(forms, times):
            print("  %-52s %s" % (name, fmt(ts)))
        med = [float(np.median(ts)) for ts in times]
        gb = block.numel() * 4 / 1e9
        print("  fused / topk %.3f x;  gather pass (iv) - (v) %.3f ms = %.2f x the plain read (vi), which runs at %.0f GB/s"
              % (med[0] / med[1], 1e3 * (med[3] - med[4]), (med[3] - med[4]) / med[5], gb / med[5]))
        del hist, ll, block
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
