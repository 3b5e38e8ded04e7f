#!/usr/bin/env python3
"""The accuracy evidence of PSIS-LOO, written with its command line to profiles/loo_accuracy.txt:

    python tools/loo_accuracy.py [--no-gpu]

CPU part (always): on the fixtures of tests/loo_case.py the numpy route against the direct restatement, the reference khat
range and its distance from the gates, and the sensitivities behind K_KHAT / K_ELPD -- the worst |change| / delta_i of khat and
elpd_loo_i of the float64 estimator when every logit moves by +-delta_si (8 seeded sign patterns per fixture).
GPU part (when a ROCm device is there): the kernels' raw outputs and finished numbers against the numpy route in units of
their gates, and the device `loo_finish` against the numpy one on the same tails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loo_case as lc  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "loo_accuracy.txt")


def cpu_part(say):
    from l2hmc_amd import predictive
    worst_k = worst_e = 0.0
    say("fixture           M   max khat  min khat  nearest gate / (K_KHAT delta)   numpy route - restatement (khat, elpd)   sens khat  sens elpd")
    for S, n, d in lc.FIXTURES:
        W, X, y = lc.case(S, n, d)
        t = lc.signed_logits(W, X, y)
        ref = lc.restatement(W, X, y, t)
        got = predictive.loo(W, X, y)
        di, dsi = lc.delta(W, X)
        fin = np.isfinite(ref["khat"])
        assert np.array_equal(fin, np.isfinite(got.khat)) and np.array_equal(ref["n_tail"], got.n_tail)
        dk = float(np.max(np.abs(got.khat[fin] - ref["khat"][fin]))) if fin.any() else 0.0
        de = float(np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])))
        sk = se = 0.0
        for pattern in range(8):
            sign = np.where(np.random.RandomState(100 * pattern + S).rand(*t.shape) < 0.5, -1.0, 1.0)
            per = lc.restatement(W, X, y, t + sign * dsi)
            both = fin & np.isfinite(per["khat"])
            if both.any():
                sk = max(sk, float(np.max(np.abs(per["khat"] - ref["khat"])[both] / di[both])))
            se = max(se, float(np.max(np.abs(per["elpd_loo_i"] - ref["elpd_loo_i"]) / di)))
        room = np.inf
        if fin.any():
            gap = np.minimum(np.abs(ref["khat"] - lc.KHAT_BAD), np.abs(ref["khat"] - lc.khat_threshold(S)))
            room = float(np.min((gap / (lc.K_KHAT * di))[fin]))
        say("%-16s %4d  %8.3f  %8.3f  %12.3g   %26.2g %9.2g   %14.3g  %9.3g" % (
            (S, n, d), lc.tail_len(S), ref["khat"][fin].max() if fin.any() else np.nan,
            ref["khat"][fin].min() if fin.any() else np.nan, room, dk, de, sk, se))
        worst_k, worst_e = max(worst_k, sk), max(worst_e, se)
    say("worst sensitivity: khat %.4g, elpd_loo_i %.4g per unit of delta_i  ->  K_KHAT = 4 x %.4g, K_ELPD = 4 x %.4g in tests/loo_case.py"
        % (worst_k, worst_e, lc.K_KHAT / 4, lc.K_ELPD / 4))
    say("(a fixture whose 'nearest gate' column is below 1 has a reference khat within its gate of 0.7 or of khat_threshold: move its seed)")


def gpu_part(say):
    import torch
    from l2hmc_amd import predictive
    say("")
    say(torch.cuda.get_device_name() + ": kernels against the numpy route, in units of the gates of tests/test_gpu_loo.py; device loo_finish - numpy loo_finish")
    say("fixture           cutoff/delta  tail/delta  logsum/(delta + 16 eps)  khat/(K delta)  elpd/(K delta)   finish: khat      elpd")
    wk = we = 0.0
    for S, n, d in lc.FIXTURES:
        W, X, y = lc.case(S, n, d)
        ref_t = predictive.loo_tails(W, X, y)
        ref = predictive.loo_finish(ref_t)
        dev_t = predictive.loo_tails(torch.as_tensor(W).cuda(), X, y)
        got = predictive.loo_finish(dev_t)
        host_t = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dev_t.items()}
        same = predictive.loo_finish(host_t)
        di, _ = lc.delta(W, X)
        M = lc.tail_len(S)
        tail = np.sort(host_t["tail"].astype(np.float64), axis=1)
        both = np.isfinite(tail) & np.isfinite(ref_t["tail"])
        rt = float(np.max(np.where(both, np.abs(tail - ref_t["tail"]), 0.0) / di[:, None])) if M else 0.0
        rc = float(np.max(np.abs(host_t["cutoff"] - ref_t["cutoff"]) / di))

        def logsum(tt):
            m = np.minimum(np.asarray(tt["cutoff"], dtype=np.float64), 0.0)
            lam = np.where(np.isfinite(tt["tail"]), np.logaddexp(0.0, -np.asarray(tt["tail"], dtype=np.float64)), -np.inf)
            return np.logaddexp(np.log(tt["body"]) - m, np.logaddexp.reduce(lam, axis=1) if M else -np.inf)
        with np.errstate(all="ignore"):
            rl = float(np.max(np.abs(logsum(host_t) - logsum(ref_t)) / (di + 16 * lc.EPS)))
            fin = np.isfinite(ref.khat) & np.isfinite(got.khat)
            rk = float(np.max(np.abs(got.khat - ref.khat)[fin] / (lc.K_KHAT * di[fin]))) if fin.any() else 0.0
            re_ = float(np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / (lc.K_ELPD * di)))
            fk = float(np.max(np.abs(got.khat - same.khat)[fin])) if fin.any() else 0.0
            fe = float(np.max(np.abs(got.elpd_loo_i - same.elpd_loo_i)))
        wk, we = max(wk, fk), max(we, fe)
        say("%-16s %12.3g %11.3g %24.3g %15.3g %15.3g %14.3g %9.3g" % ((S, n, d), rc, rt, rl, rk, re_, fk, fe))
    say("device loo_finish against numpy loo_finish, worst: khat %.3g, elpd_loo_i %.3g  (tests gate at 100 x, never looser than 1e-6)" % (wk, we))


def main():
    lines = ["$ python tools/loo_accuracy.py " + " ".join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cpu_part(say)
    gpu = "--no-gpu" not in sys.argv
    if gpu:
        import torch
        gpu = torch.cuda.is_available()
    if gpu:
        gpu_part(say)
    else:
        say("")
        say("(no ROCm device: the kernels' ratios were not measured in this run)")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
