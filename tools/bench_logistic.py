#!/usr/bin/env python
"""Bayesian logistic regression throughput (GPU box): microseconds per HMC proposal (T leapfrog steps, T + 1 gradients) of the
fused target (L2HMC_ENERGY_LOGISTIC, the general trajectory kernel's persistent loop) against the same likelihood written as a
torch callable (the slow path: U and grad U from torch between launches of the GEMM engine), on seeded synthetic data.

    python tools/bench_logistic.py [--T 10] [--proposals 10] [--reps 3] [--quick]

Columns: kernel (`_ffi.last_kernel()`), us per proposal of both paths, and the algorithmic flop count 4 n d (T + 1) per chain and
proposal (the two data contractions per gradient) as a fraction of the 157.3 TFLOP/s f32-MFMA peak of the MI355X."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, _ffi, sample_chain

F32_MFMA_PEAK = 157.3e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def data(n, d, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    X = (X - X.mean(0)) / X.std(0)                                  # standardised features
    w = rng.randn(d) / np.sqrt(d)
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w))).astype(np.float32)
    return X.astype(np.float32), y


def torch_energy(X, y, prior_var):
    Xt, yt = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()

    def U(w):
        L = w @ Xt.T
        return (torch.nn.functional.softplus(L) - L * yt).sum(1) + 0.5 * (w * w).sum(1) / prior_var

    def gU(w):
        return (torch.sigmoid(w @ Xt.T) - yt) @ Xt + w / prior_var
    return U, gU


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--proposals", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="German-credit shape only")
    a = ap.parse_args()
    grid = [(n, d, N) for n in (256, 1000, 4096) for d in (8, 25, 64) for N in (4096, 16384)]
    grid.insert(0, (1000, 25, 8192))                               # German-credit shape at 8192 chains
    if a.quick:
        grid = grid[:1]
    print("%6s %4s %6s  %-28s %11s %11s %8s %9s" % ("n", "d", "chains", "kernel", "fused us", "slow us", "speedup", "f32 roof"))
    for n, d, N in grid:
        X, y = data(n, d, seed=n + d)
        s2 = 1.0
        eps = 0.5 / np.sqrt(n)
        x0 = torch.as_tensor((0.1 * np.random.RandomState(1).randn(N, d)).astype(np.float32)).cuda()
        dyn = Dynamics(d, LogisticRegression(X, y, prior_var=s2).get_energy_function(), T=a.T, eps=eps, hmc=True)
        dyn.eps_override = eps
        P = a.proposals
        t_f = timed(lambda: sample_chain(x0, dyn, P, seed=1), a.reps) / P
        kern = _ffi.last_kernel()
        U, gU = torch_energy(X, y, s2)
        slow = Dynamics(d, U, T=a.T, eps=eps, hmc=True, grad_energy=gU)
        slow.eps_override = eps
        Ps = max(1, P // 5)
        t_s = timed(lambda: sample_chain(x0, slow, Ps, seed=1), max(1, a.reps - 1)) / Ps
        flop = 4.0 * n * d * (a.T + 1) * N
        roof = flop / t_f / F32_MFMA_PEAK
        print("%6d %4d %6d  %-28s %11.1f %11.1f %8.1f %8.1f%%" % (n, d, N, kern, 1e6 * t_f, 1e6 * t_s, t_s / t_f, 100 * roof))
        print(json.dumps({"n": n, "d": d, "chains": N, "T": a.T, "kernel": kern, "fused_us_per_proposal": 1e6 * t_f,
                          "slow_us_per_proposal": 1e6 * t_s, "flop_per_proposal": flop, "f32_roof_fraction": roof}))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
