#!/usr/bin/env python3
"""The accuracy evidence of the PSIS kernels, written with its command line to profiles/psis_accuracy.txt:

    python tools/psis_accuracy.py [--no-gpu]

CPU part (always): two float64 host references against each other -- the module's numpy path (`predictive.loo_finish`,
`psis.loo_from_log_lik`: `_pareto._psis_rows`) and the row-at-a-time restatement of tests/psis_case.py; they differ in
summation order and in how x is formed.  Per tested tail length M, over the five k_true x three seeds and tails shorter than
M, the worst disagreement of khat and of elpd_loo_i; the matrices and histories the GPU tests use are measured the same way and
count towards their M.  `MEASURED` in tests/psis_case.py holds these figures; the gate at M is 100 x the worst at any length up to M, capped at 1e-9.
GPU part (when a ROCm device is there): the kernel route (`finish="kernel"`, device `loo_from_log_lik`) against the numpy path
on the same tails, as a share of each gate."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loo_case as lc  # noqa: E402
from tests import psis_case as pc  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "psis_accuracy.txt")
TAIL_LENGTHS = (5, 6, 63, 64, 65, 255, 256, 257, 769, 6072, 21467)
MATRICES = ((25, 3), (4099, 7), (65609, 4))
HISTORIES = lc.FIXTURES + [(70, 35, 5), (4, 3, 2)]


def rows_of(M):
    """The rows measured at tail length M: full tails for every k_true x 3 seeds' worth of rows, and shorter ones."""
    rows = [(M, k) for k in pc.K_TRUE for _ in range(3 if M <= 6072 else 1)]
    for L in sorted({0, 1, 4, 5, 6, M // 2, M - 1}):
        if 0 <= L < M:
            rows.append((L, pc.K_TRUE[L % 5]))
    return rows


def diff(a, b):
    with np.errstate(all="ignore"):
        both = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        return float(np.max(np.abs(a - b)[both])) if both.any() else 0.0


def cpu_part(say):
    from l2hmc_amd import predictive, psis
    worst = {}

    def note(M, dk, de):
        k, e = worst.get(M, (0.0, 0.0))
        worst[M] = (max(k, dk), max(e, de))

    say("numpy path - restatement, float64 both (tails of tests/psis_case.py)")
    say("   M   rows   khat range          |d khat|   |d elpd_loo_i|")
    for M in TAIL_LENGTHS:
        raw = pc.tails(M, rows_of(M), seed=M)
        got, ref = predictive.loo_finish(raw), pc.restate_finish(raw)
        dk, de = diff(got.khat, ref["khat"]), diff(got.elpd_loo_i, ref["elpd_loo_i"])
        fin = np.isfinite(ref["khat"])
        say("%6d %5d   %7.3f .. %6.3f   %9.3g   %9.3g" % (M, len(raw["n_tail"]), ref["khat"][fin].min(), ref["khat"][fin].max(), dk, de))
        note(M, dk, de)
    say("")
    say("loo_from_log_lik (numpy) - restatement on the matrices of tests/test_gpu_psis.py")
    for S, n in MATRICES:
        ll = pc.log_lik_case(S, n, seed=S, ties=True)
        got, ref = psis.loo_from_log_lik(ll), pc.restate_loo(ll)
        assert np.array_equal(got.n_tail, ref["n_tail"])
        dk, de = diff(got.khat, ref["khat"]), diff(got.elpd_loo_i, ref["elpd_loo_i"])
        say("(%6d, %d)  M = %4d   %9.3g   %9.3g" % (S, n, lc.tail_len(S), dk, de))
        note(lc.tail_len(S), dk, de)
    say("")
    say("predictive.loo (numpy) - loo_case.restatement on the histories of the finish=\"kernel\" tests")
    for S, n, d in HISTORIES:
        W, X, y = lc.case(S, n, d)
        got, ref = predictive.loo(W, X, y), lc.restatement(W, X, y)
        dk, de = diff(got.khat, ref["khat"]), diff(got.elpd_loo_i, ref["elpd_loo_i"])
        say("%-16s M = %4d   %9.3g   %9.3g" % ((S, n, d), lc.tail_len(S), dk, de))
        note(lc.tail_len(S), dk, de)
    say("")
    say("MEASURED = {   # tests/psis_case.py")
    for M in sorted(worst):
        say("    %d: (%.3g, %.3g)," % (M, worst[M][0], worst[M][1]))
    say("}")
    stale = {M: v for M, v in worst.items() if pc.MEASURED.get(M) != (float("%.3g" % v[0]), float("%.3g" % v[1]))}
    say("tests/psis_case.py MEASURED %s" % ("agrees with this run" if not stale else "DIFFERS from this run at M = %s" % sorted(stale)))


def gpu_part(say):
    import torch
    from l2hmc_amd import predictive, psis
    say("")
    say(torch.cuda.get_device_name() + ": the kernel route against the numpy path on the same tails, as a share of each gate")
    say("   M     gate khat  gate elpd   |d khat|  share    |d elpd|  share")

    def line(M, dk, de):
        gk, ge = pc.gate(M)
        say("%6d   %9.3g  %9.3g  %9.3g  %6.3g  %9.3g  %6.3g" % (M, gk, ge, dk, dk / gk if gk else (np.inf if dk > 0 else 0.0),
                                                              de, de / ge if ge else (np.inf if de > 0 else 0.0)))
    for M in TAIL_LENGTHS:
        raw = pc.tails(M, rows_of(M), seed=M)
        dev = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
        got, ref = predictive.loo_finish(dev, finish="kernel"), predictive.loo_finish(raw)
        line(M, diff(got.khat, ref.khat), diff(got.elpd_loo_i, ref.elpd_loo_i))
    say("loo_from_log_lik on the device against numpy:")
    for S, n in MATRICES:
        ll = pc.log_lik_case(S, n, seed=S, ties=True)
        got, ref = psis.loo_from_log_lik(torch.as_tensor(ll).cuda()), psis.loo_from_log_lik(ll)
        line(lc.tail_len(S), diff(got.khat, ref.khat), diff(got.elpd_loo_i, ref.elpd_loo_i))
    say("loo(finish=\"kernel\") against the numpy finish of the same device tails:")
    for S, n, d in HISTORIES:
        W, X, y = lc.case(S, n, d)
        t = predictive.loo_tails(torch.as_tensor(W).cuda(), X, y)
        host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in t.items()}
        got, ref = predictive.loo_finish(t, finish="kernel"), predictive.loo_finish(host)
        line(lc.tail_len(S), diff(got.khat, ref.khat), diff(got.elpd_loo_i, ref.elpd_loo_i))


def main():
    lines = ["$ python tools/psis_accuracy.py " + " ".join(sys.argv[1:])]

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
        say("(no ROCm device: the kernel's shares were not measured in this run)")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
