#!/usr/bin/env python3
"""The accuracy evidence of the per-row relative efficiency, written with its command line to
profiles/lik_stats_accuracy.txt:

    python tools/lik_stats_accuracy.py [--no-gpu]

CPU part (always): on the fixtures of tests/lik_stats_case.py the numpy route of `predictive.relative_eff` against the direct
restatement, the reference r_eff range and tail lengths, and the sensitivity behind K_REFF -- the worst |relative change| /
delta_i of r_eff of the float64 estimator when every logit moves by +-delta_si (8 seeded sign patterns per fixture), over the
rows whose Geyer truncation index does not move; the rows where it moves are counted.  Then the same for `loo(r_eff="auto")`:
the numpy route against the direct restatement and the sensitivities behind K_NEFF and K_MCSE.
GPU part (when a ROCm device is there): the kernel's raw sums against float64 in units of their derived bounds, the
device's r_eff against the numpy route in units of K_REFF delta_i, `loo(r_eff="auto")` on the device with both finishes in
units of its gates, and the device finishes against the numpy finish on the same tails (FINISH_NEFF, FINISH_MCSE)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lik_stats_case as ls  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "lik_stats_accuracy.txt")


def cpu_part(say):
    from l2hmc_amd import predictive
    worst = 0.0
    say("fixture (M, N, d, rho, max_lag, split)   r_eff min .. max   truncated  near boundary   M_i min .. max (M at r_eff = 1)   numpy - restatement   sens r_eff")
    for f in ls.FIXTURES:
        M, N, d, rho, max_lag, split = f
        W, X, y = ls.ar1_case(M, N, d, rho)
        ref, near, sens = ls.sensitivity(f)
        got = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
        assert np.array_equal(got.truncated, ref["truncated"])
        Mi, M1 = ls.tail_lengths(ref["r_eff"], M * N), int(ls.tail_lengths(np.ones(1), M * N)[0])
        say("%-40s %7.3f .. %.3f %10d %14d %12d .. %-4d (%4d) %24.2g %12.3g" % (
            f, ref["r_eff"].min(), ref["r_eff"].max(), ref["truncated"].sum(), near.sum(), Mi.min(), Mi.max(), M1,
            np.max(np.abs(got.r_eff - ref["r_eff"])), sens))
        worst = max(worst, sens)
    say("worst sensitivity: r_eff %.4g (relative) per unit of delta_i  ->  K_REFF = 4 x %.4g in tests/lik_stats_case.py"
        % (worst, ls.K_REFF / 4))
    say("(at most %.0f %% of a fixture's rows may be near a truncation boundary: tests/test_lik_stats_cpu.py)" % (100 * ls.EXCLUDED_AT_MOST))
    say("")
    say("loo(r_eff=\"auto\"): numpy route - restatement (khat, elpd_loo_i absolute; n_eff, mcse relative), near boundary, sensitivities")
    say("fixture                                      khat     elpd    n_eff     mcse   near   sens n_eff   sens mcse")
    wn = wm = 0.0
    for f in ls.FIXTURES:
        M, N, d, rho, max_lag, split = f
        W, X, y = ls.ar1_case(M, N, d, rho)
        ref, near, sn, sm = ls.loo_sensitivity(f)
        got = predictive.loo(W, X, y, r_eff="auto")
        fin = np.isfinite(ref["khat"])
        assert np.array_equal(got.n_tail, ref["n_tail"]) and np.array_equal(got.tail_len_row, ref["tail_len_row"])
        say("%-40s %8.2g %8.2g %8.2g %8.2g %6d %12.4g %11.4g" % (
            f, np.max(np.abs(got.khat - ref["khat"])[fin]), np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])),
            np.max(np.abs(got.n_eff / ref["n_eff"] - 1.0)), np.max(np.abs(got.mcse_elpd_loo_i / ref["mcse"] - 1.0)), near.sum(), sn, sm))
        wn, wm = max(wn, sn), max(wm, sm)
    say("worst sensitivity: n_eff %.4g, mcse_elpd_loo_i %.4g (relative) per unit of delta_i  ->  K_NEFF = 4 x %.4g, K_MCSE = 4 x %.4g"
        % (wn, wm, ls.K_NEFF / 4, ls.K_MCSE / 4))


def gpu_part(say):
    import torch
    from l2hmc_amd import predictive
    say("")
    say(torch.cuda.get_device_name() + ": the kernel's raw sums / their derived bounds; device r_eff - numpy route in units of K_REFF delta_i")
    say("fixture                                       mean       M2        G      r_eff")
    for f in ls.FIXTURES:
        M, N, d, rho, max_lag, split = f
        W, X, y = ls.ar1_case(M, N, d, rho)
        ref, bound = ls.raw_bounds(W, X, y, max_lag, split)
        got = dict(zip(("mean", "m2", "G"), ls.device_raw(W, X, y, max_lag, split)))
        r = [float(np.max(np.abs(got[k] - ref[k]) / bound[k])) for k in ("mean", "m2", "G")]
        host = predictive.relative_eff(W, X, y, max_lag=max_lag, split=split)
        dev = predictive.relative_eff(torch.as_tensor(W).cuda(), X, y, max_lag=max_lag, split=split)
        _, near, _ = ls.sensitivity(f)
        di, _ = ls.delta(W, X)
        rr = float(np.max((np.abs(dev.r_eff / host.r_eff - 1.0) / (ls.K_REFF * di))[~near]))
        say("%-40s %9.3g %9.3g %9.3g %9.3g" % (f, r[0], r[1], r[2], rr))
    from tests import loo_case as lc
    say("")
    say("loo(r_eff=\"auto\") on the device / its gates (K_KHAT, K_ELPD of tests/loo_case.py; K_NEFF, K_MCSE); device finish - numpy finish on the same tails (relative)")
    say("fixture                                  finish     khat      elpd     n_eff      mcse   finish: n_eff      mcse")
    fn_w = fm_w = 0.0
    for f in ls.FIXTURES:
        M, N, d, rho, max_lag, split = f
        W, X, y = ls.ar1_case(M, N, d, rho)
        Wd = torch.as_tensor(W).cuda()
        ref = predictive.loo(W, X, y, r_eff="auto")
        _, near, _, _ = ls.loo_sensitivity(f)
        keep = ~near
        di, _ = ls.delta(W, X)
        for finish in ("torch", "kernel"):
            got = predictive.loo(Wd, X, y, finish=finish, r_eff="auto")
            fin = np.isfinite(ref.khat) & keep
            rk = float(np.max(np.abs(got.khat - ref.khat)[fin] / (lc.K_KHAT * di[fin])))
            re_ = float(np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i)[keep] / (lc.K_ELPD * di[keep])))
            rn = float(np.max(np.abs(got.n_eff / ref.n_eff - 1.0)[keep] / (ls.K_NEFF * di[keep])))
            rm = float(np.max(np.abs(got.mcse_elpd_loo_i / ref.mcse_elpd_loo_i - 1.0)[keep] / (ls.K_MCSE * di[keep])))
            dev_t = predictive.loo_tails(Wd, X, y, tail_len_row=got.tail_len_row)
            host_t = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dev_t.items()}
            same = predictive.loo_finish(host_t, r_eff=got.r_eff)
            mine = predictive.loo_finish(dev_t, finish=finish, r_eff=got.r_eff)
            fn = float(np.max(np.abs(mine.n_eff / same.n_eff - 1.0)))
            fm = float(np.max(np.abs(mine.mcse_elpd_loo_i / same.mcse_elpd_loo_i - 1.0)))
            fn_w, fm_w = max(fn_w, fn), max(fm_w, fm)
            say("%-40s %-6s %8.3g %9.3g %9.3g %9.3g %15.3g %9.3g" % (f, finish, rk, re_, rn, rm, fn, fm))
    say("device finishes against the numpy finish, worst: n_eff %.3g, mcse_elpd_loo_i %.3g  (tests gate at 100 x, never looser than 1e-6: "
        "FINISH_NEFF = %.3g, FINISH_MCSE = %.3g)" % (fn_w, fm_w, ls.FINISH_NEFF, ls.FINISH_MCSE))


def main():
    lines = ["$ python tools/lik_stats_accuracy.py " + " ".join(sys.argv[1:])]

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
        say("(no ROCm device: the kernel's ratios were not measured in this run)")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
