#!/usr/bin/env python
"""The accuracy record of the fused Poisson-regression target (GPU box): the worst used share of every bound of
tests/poisson_target_case.py over the shapes of tests/test_gpu_poisson_target.py -- U and grad U on the planned and the streamed
data path, with and without offsets, under a temperature and under the AIS bridge -- and, for every trajectory case, the
distance of the kernels from the float32 oracle next to that oracle's own distance from float64 and the gate the test computes
from it.

    python tools/poisson_target_accuracy.py [--out profiles/poisson_target_accuracy.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, PoissonRegression
from tests import poisson_target_case as pc
from tests.helpers import to_dev, to_np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_target_accuracy.txt"))
    a = ap.parse_args()
    from tests.test_gpu_poisson_target import fused, twin
    out = ["Fused Poisson-regression target: share of the bounds of tests/poisson_target_case.py used on %s" % torch.cuda.get_device_name(0),
           "", "U and grad U, 40 chains, worst over {planned, streamed} x {offsets, zero offsets}",
           "%6s %4s %10s %10s" % ("n", "d", "U", "grad U")]
    worst = {"U": 0.0, "g": 0.0}
    for n in (1, 16, 17, 1000, 8192):
        for d in (2, 5, 25, 50, 128):
            W, X, y, o = pc.case(40, n, d)
            sU = sg = 0.0
            for env in (None, "0"):
                if env is None:
                    os.environ.pop("L2HMC_LOGISTIC_LDS", None)
                else:
                    os.environ["L2HMC_LOGISTIC_LDS"] = env
                for oo in (o, np.zeros_like(o)):
                    U, G = fused(X, y, oo).evaluate(to_dev(W), want_grad=True)
                    u1, g1 = pc.used(to_np(U), to_np(G), *pc.energy(W, X, y, oo), pc.bounds(W, X, y, oo))
                    sU, sg = max(sU, u1), max(sg, g1)
            os.environ.pop("L2HMC_LOGISTIC_LDS", None)
            worst["U"], worst["g"] = max(worst["U"], sU), max(worst["g"], sg)
            out.append("%6d %4d %10.4f %10.4f" % (n, d, sU, sg))
    out.append("worst used share: U %.4f, grad U %.4f" % (worst["U"], worst["g"]))
    W, X, y, o = pc.case(33, 300, 8)
    dyn = Dynamics(8, fused(X, y, o), T=5, eps=0.01, hmc=True)
    out += ["", "scaled bounds, n = 300, d = 8, 33 chains"]
    for label, T, beta in (("temperature 2.5", 2.5, 1.0), ("AIS bridge beta 0.3", 1.0, 0.3)):
        dyn.use_temperature, dyn.temperature, dyn.anneal_beta = T != 1.0, T, (beta if beta != 1.0 else 0.0)
        Ur, Gr, b = pc.scaled(W, X, y, o, temperature=T, beta=beta)
        sU, sg = pc.used(to_np(dyn.energy(to_dev(W))), to_np(dyn.grad_energy(to_dev(W))), Ur, Gr, b)
        out.append("%-22s U %.4f  grad U %.4f" % (label, sU, sg))
    out += ["", "trajectories, N = %d, T = %d: kernel against the float32 oracle | float32 oracle against float64 | gate = max(project gate, 4 x that)"
            % (pc.TRAJ_N, pc.TRAJ_T), "(x, v: relative to max(1, |.|); log-Jacobian: relative; accept probability: absolute)"]
    for n, d, H in pc.TRAJ_CASES:
        c = pc.traj_case(n, d, H)
        dyn = twin(c["g"], fused(c["X"], c["y"], c["o"]), c["hmc"], max(H, 1), c["eps"])
        xd, vd = to_dev(c["x"]), to_dev(c["v"])
        X1, V1, lj = dyn.forward(xd, init_v=vd, log_jac=True)
        p = dyn.forward(xd, init_v=vd)[2]
        rX, rV, rlj, rp = c["ref"]["forward"]
        errs = (pc.rel_err(to_np(X1), rX), pc.rel_err(to_np(V1), rV), pc.rel_err(to_np(lj), rlj), pc.abs_err(to_np(p), rp))
        gates = tuple(pc.gate(b, dd) for b, dd in zip((pc.STATE_GATE, pc.STATE_GATE, pc.SCALAR_GATE, pc.SCALAR_GATE), c["dist"]["forward"]))
        out.append("n=%4d d=%3d H=%2d eps=%-9.3g accept %.3f" % (n, d, H, c["eps"], float(rp.mean())))
        for name, e, dd, gt in zip(("x", "v", "logjac", "p"), errs, c["dist"]["forward"], gates):
            out.append("    %-7s %.3g | %.3g | %.3g   (share of the gate %.3f)" % (name, e, dd, gt, e / gt))
        for s in (0, 3):
            for key, got in (("fwd%d" % s, dyn._forward_step(xd, vd, s)), ("bwd%d" % s, dyn._backward_step(xd, vd, s))):
                es = tuple(pc.rel_err(to_np(got[i]), c["ref"][key][i]) for i in range(3))
                out.append("    %-7s x %.3g | %.3g   v %.3g | %.3g   logjac %.3g | %.3g" % (
                    key, es[0], c["dist"][key][0], es[1], c["dist"][key][1], es[2], c["dist"][key][2]))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
