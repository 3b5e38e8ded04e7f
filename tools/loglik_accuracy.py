#!/usr/bin/env python3
"""The figures behind the gates of tests/loglik_case.py, measured on the CPU (no GPU, no kernel):

    python tools/loglik_accuracy.py [profiles/loglik_accuracy.txt]

Per tested matrix and AR(1) history: the disagreement of the module's float64 numpy route (`psis.loo_from_log_lik`, with and
without `r_eff`) and the column-at-a-time restatement of tests/loglik_case.py -- khat and elpd_loo_i absolute, n_eff and
mcse_elpd_loo_i relative -- and, last, the `MEASURED` table by number of draws that the case file holds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from l2hmc_amd import psis  # noqa: E402
from l2hmc_amd._pareto import loo_tail_len  # noqa: E402
from tests import loglik_case as lk  # noqa: E402


def disagreement(ll, r_eff):
    """(khat, elpd, n_eff rel, mcse rel) of one float64 matrix; the last two 0 without r_eff."""
    S, n = ll.shape
    got = psis.loo_from_log_lik(ll, r_eff=r_eff)
    lens = np.full(n, loo_tail_len(S)) if r_eff is None else lk.tail_lengths(r_eff, S)
    ref = lk.restate(ll, lens, r_eff)
    assert np.array_equal(got.n_tail, ref["n_tail"]), (got.n_tail, ref["n_tail"])
    both = np.isfinite(got.khat) & np.isfinite(ref["khat"])
    assert np.array_equal(np.isfinite(got.khat), np.isfinite(ref["khat"]))
    with np.errstate(invalid="ignore"):                      # (khat = +inf on both sides where nothing was fitted)
        dk = np.abs(got.khat - ref["khat"])[both]
    out = [float(np.max(dk, initial=0.0)), float(np.max(np.abs(got.elpd_loo_i - ref["elpd_loo_i"])))]
    if r_eff is None:
        return out + [0.0, 0.0]
    return out + [float(np.max(np.abs(got.n_eff / ref["n_eff"] - 1.0))), float(np.max(np.abs(got.mcse_elpd_loo_i / ref["mcse"] - 1.0)))]


def main():
    lines, table = [], {}

    def note(what, S, fig):
        lines.append("%-46s S = %6d   khat %.3g   elpd %.3g   n_eff %.3g   mcse %.3g" % ((what, S) + tuple(fig)))
        table[S] = tuple(max(a, b) for a, b in zip(table.get(S, (0.0,) * 4), fig))

    for S, n in lk.FINISH_SHAPES:
        ll = lk.matrix(S, n).astype(np.float64)
        note("matrix (%d, %d), one tail length" % (S, n), S, disagreement(ll, None))
        note("matrix (%d, %d), r_eff 0.15 .. 1.1" % (S, n), S, disagreement(ll, lk.r_eff_for(n)))
    for f in lk.AR1_FIXTURES:
        ll = lk.ar1_log_lik(f)[0]
        r = psis.relative_eff_from_log_lik(ll, max_lag=f[4], split=f[5]).r_eff
        flat = ll.reshape(-1, ll.shape[-1])
        note("AR(1) %s, r_eff auto" % (f,), flat.shape[0], disagreement(flat, r))
        note("AR(1) %s, one tail length" % (f,), flat.shape[0], disagreement(flat, None))
    lines.append("")
    lines.append("MEASURED = {")
    for S in sorted(table):
        lines.append("    %d: (%s)," % (S, ", ".join("%.3g" % v for v in table[S])))
    lines.append("}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("tools/loglik_accuracy.py: the numpy route of psis.loo_from_log_lik against the restatement of "
                     "tests/loglik_case.py (CPU, float64)\n" + text)


if __name__ == "__main__":
    main()
