#!/usr/bin/env python
"""Poisson regression as a sampling target (GPU box): microseconds per HMC proposal (T leapfrog steps, T + 1 gradients) of
  fused     the fused Poisson target (L2HMC_ENERGY_POISSON: the general trajectory kernel's persistent loop),
  slow      the same model on the slow path (`get_energy_function()`: U and grad U from torch between launches of the GEMM engine),
  logistic  the fused logistic-regression target of the same shape (same contractions, three transcendentals per row against one),
at n = 1000, d = 25, T = 10 and 4096 / 8192 chains, on seeded synthetic data.

    python tools/bench_poisson.py [--rounds 7] [--proposals 10] [--out profiles/poisson_target_bench.txt]

The three are timed in alternating rounds (fused, logistic, slow, fused, ...) after a warm-up of each, and the medians over the
rounds are reported with the spread (min .. max), so that a drift of the machine shows in all three columns and not in one."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, PoissonRegression, _ffi, sample_chain


def data(n, d, seed=0):
    """Standardised features, counts from a log-linear model with exposures in [0.5, 3], labels from the logistic model of the same w."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    X = (X - X.mean(0)) / X.std(0)
    w = rng.randn(d) / np.sqrt(d)
    o = np.log(rng.uniform(0.5, 3.0, size=n))
    y = rng.poisson(np.exp(X @ w + o))
    lab = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ w))).astype(np.float32)
    return X.astype(np.float32), y.astype(np.float32), o.astype(np.float32), lab


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--d", type=int, default=25)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--proposals", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_target_bench.txt"))
    a = ap.parse_args()
    n, d, T, P = a.n, a.d, a.T, a.proposals
    X, y, o, lab = data(n, d, seed=n + d)
    eps = 0.25 / np.sqrt(n * float(np.exp(o).mean()))
    lines = ["Poisson regression as a sampling target: us per HMC proposal (T = %d leapfrog steps), n = %d, d = %d" % (T, n, d),
             "device: %s; medians of %d alternating rounds of %d proposals (min .. max)" % (torch.cuda.get_device_name(0), a.rounds, P),
             "%6s  %-24s %22s %22s %24s %9s %9s" % ("chains", "kernel", "fused Poisson us", "fused logistic us", "slow-path Poisson us",
                                                  "slow/fused", "pois/logi")]
    for N in (4096, 8192):
        x0 = torch.as_tensor((0.05 * np.random.RandomState(1).randn(N, d)).astype(np.float32)).cuda()
        model = PoissonRegression(X, y, offset=o, prior_var=1.0)
        dyns = {"fused": Dynamics(d, model.get_energy_function(fused=True), T=T, eps=eps, hmc=True),
                "logistic": Dynamics(d, LogisticRegression(X, lab, prior_var=1.0).get_energy_function(), T=T, eps=eps, hmc=True),
                "slow": Dynamics(d, model.get_energy_function(), T=T, eps=eps, hmc=True)}
        for dyn in dyns.values():
            dyn.eps_override = eps
        runs = {k: (lambda dyn=dyn: sample_chain(x0, dyn, P, seed=1)) for k, dyn in dyns.items()}
        kern = {}
        for k, fn in runs.items():                                  # warm-up: code objects, the packed data set, workspaces
            fn()
            torch.cuda.synchronize()
            kern[k] = _ffi.last_kernel()
        _, p, _ = runs["fused"]()
        ts = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k in ("fused", "logistic", "slow"):
                ts[k].append(1e6 * once(runs[k]) / P)
        med = {k: float(np.median(v)) for k, v in ts.items()}

        def cell(k):
            return "%8.1f (%.1f .. %.1f)" % (med[k], min(ts[k]), max(ts[k]))
        lines.append("%6d  %-24s %22s %22s %24s %9.1f %9.2f" % (N, kern["fused"], cell("fused"), cell("logistic"), cell("slow"),
                                                               med["slow"] / med["fused"], med["fused"] / med["logistic"]))
        print(json.dumps({"n": n, "d": d, "chains": N, "T": T, "kernels": kern, "us_per_proposal": med,
                          "spread": {k: [min(v), max(v)] for k, v in ts.items()}, "accept": float(p.mean())}))
        sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
