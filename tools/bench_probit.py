#!/usr/bin/env python
"""Probit regression (GPU box), two tables in ONE run:

 (a) as a sampling target: microseconds per HMC proposal (T leapfrog steps, T + 1 gradients) of
       probit     the fused probit target (L2HMC_ENERGY_PROBIT: the general trajectory kernel's persistent loop), trials 1 .. 50,
       binomial   the fused binomial target of the same shape and data layout (L2HMC_ENERGY_BINOMIAL), the yardstick,
       logistic   the fused logistic-regression target of the same shape (L2HMC_ENERGY_LOGISTIC),
       slow       the probit model on the slow path (`get_energy_function()`: torch between launches of the GEMM engine),
     at n = 1000, d = 25, T = 10 and 4096 / 8192 chains, on seeded synthetic data, timed in alternating rounds after a warm-up
     of each; medians over the rounds with the spread (min .. max);
 (b) the model criticism from a device history of 1000 x 4096 draws of d = 25 against 1000 rows: `model.loo(W)` and
     `model.waic(W)` of `ProbitRegression` next to `BinomialRegression`'s in the same run (one warm-up call of each, then
     `--reps` alternating rounds; median per call and the spread).

    python tools/bench_probit.py [--rounds 7] [--proposals 100] [--reps 3] [--out profiles/probit_bench.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import BinomialRegression, Dynamics, LogisticRegression, ProbitRegression, _ffi, sample_chain


def ndtr(t):
    return torch.special.ndtr(torch.as_tensor(np.asarray(t, dtype=np.float64))).numpy()


def data(n, d, seed=0):
    """Standardised features; successes out of 1 .. 50 trials from the probit and from the logistic model of the same w, and
    binary labels from the logistic model."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    X = (X - X.mean(0)) / X.std(0)
    w = rng.randn(d) / np.sqrt(d)
    trials = rng.randint(1, 51, size=n)
    p = 1.0 / (1.0 + np.exp(-X @ w))
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    return {"X": f32(X), "trials": f32(trials), "succ_probit": f32(rng.binomial(trials, ndtr(X @ w))),
            "succ_logit": f32(rng.binomial(trials, p)), "lab": f32(rng.uniform(size=n) < p)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cell(ts):
    return "%8.1f (%.1f .. %.1f)" % (float(np.median(ts)), min(ts), max(ts))


def target_table(a, lines):
    n, d, T, P = a.n, a.d, a.T, a.proposals
    D = data(n, d, seed=n + d)
    # the probit posterior is the stiffest: its curvature is bounded by sum_i m_i x_i x_i^T (the logit's by a quarter of it)
    eps = 0.25 / np.sqrt(n * float(D["trials"].mean()))
    zero = np.zeros(n, dtype=np.float32)
    probit = ProbitRegression(D["X"], D["succ_probit"], D["trials"], offset=zero, prior_var=1.0)
    binom = BinomialRegression(D["X"], D["succ_logit"], D["trials"], offset=zero, prior_var=1.0)
    order = ("probit", "binomial", "logistic", "slow")
    lines += ["(a) sampling target: us per HMC proposal (T = %d leapfrog steps), n = %d, d = %d, step size %.4g for all" % (T, n, d, eps),
              "medians of %d alternating rounds of %d proposals (min .. max)" % (a.rounds, P),
              "%6s  %-24s " % ("chains", "kernel (probit)") + " ".join("%26s" % ("%s us" % k) for k in order) + "  slow/probit  probit/binom  probit/logi"]
    for N in (4096, 8192):
        x0 = torch.as_tensor((0.05 * np.random.RandomState(1).randn(N, d)).astype(np.float32)).cuda()
        fns = {"probit": probit.get_energy_function(fused=True), "binomial": binom.get_energy_function(fused=True),
               "logistic": LogisticRegression(D["X"], D["lab"], prior_var=1.0).get_energy_function(),
               "slow": probit.get_energy_function()}
        dyns = {k: Dynamics(d, f, T=T, eps=eps, hmc=True) for k, f in fns.items()}
        for dyn in dyns.values():
            dyn.eps_override = eps
        runs = {k: (lambda dyn=dyn: sample_chain(x0, dyn, P, seed=1)) for k, dyn in dyns.items()}
        kern, acc = {}, {}
        for k, fn in runs.items():                                  # warm-up: code objects, the packed data set, workspaces
            _, p, _ = fn()
            torch.cuda.synchronize()
            kern[k], acc[k] = _ffi.last_kernel(), float(p.mean())
        ts = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k in order:
                ts[k].append(1e6 * once(runs[k]) / P)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        lines.append("%6d  %-24s " % (N, kern["probit"]) + " ".join("%26s" % cell(ts[k]) for k in order)
                     + "  %11.1f  %12.2f  %11.2f" % (med["slow"] / med["probit"], med["probit"] / med["binomial"],
                                                     med["probit"] / med["logistic"]))
        print(json.dumps({"n": n, "d": d, "chains": N, "T": T, "kernels": kern, "us_per_proposal": med,
                          "spread": {k: [min(v), max(v)] for k, v in ts.items()}, "accept": acc}))
        sys.stdout.flush()


def stats_table(a, lines):
    n, d, S = a.n, a.d, a.draws
    g = torch.Generator(device="cuda").manual_seed(d)
    X = torch.randn((n, d), device="cuda", generator=g) * (0.6 / d ** 0.5)
    w_true = torch.randn(d, device="cuda", generator=g)
    o = torch.rand(n, device="cuda", generator=g) * 2.0 - 0.5
    W = w_true + 0.1 * torch.randn((S, d), device="cuda", generator=g)               # a posterior-like cloud
    Xh, oh = X.cpu().numpy(), o.cpu().numpy()
    rng = np.random.RandomState(d)
    eta = Xh.astype(np.float64) @ w_true.cpu().numpy().astype(np.float64) + oh
    trials = rng.randint(1, 51, size=n)
    models = {"probit": ProbitRegression(Xh, rng.binomial(trials, ndtr(eta)), trials, offset=oh),
              "binomial": BinomialRegression(Xh, rng.binomial(trials, 1.0 / (1.0 + np.exp(-eta))), trials, offset=oh)}
    calls = {(k, what): (lambda m=m, what=what: getattr(m, what)(W)) for k, m in models.items() for what in ("loo", "waic")}
    for fn in calls.values():
        fn()
    ts = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            ts[k].append(1e3 * once(fn))
    lines += ["", "(b) model criticism from a device history: %d draws of d = %d (%.0f MB) against n = %d rows; ms per call, medians of %d "
              "alternating rounds (min .. max)" % (S, d, 4e-6 * S * d, n, a.reps),
              "%-10s %26s %26s" % ("model", "loo ms", "waic ms")]
    for k in models:
        lines.append("%-10s %26s %26s" % (k, cell(ts[k, "loo"]), cell(ts[k, "waic"])))
    print(json.dumps({"draws": S, "d": d, "n": n, "ms": {"%s.%s" % k: float(np.median(v)) for k, v in ts.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--d", type=int, default=25)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--proposals", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=1000 * 4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probit_bench.txt"))
    a = ap.parse_args()
    lines = ["Probit regression: tools/bench_probit.py on %s" % torch.cuda.get_device_name(0)]
    target_table(a, lines)
    stats_table(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
