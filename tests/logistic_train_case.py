"""Shared by tests/test_logistic_train_cpu.py and tests/test_gpu_logistic_train.py: the oracle's logistic-regression target
(an object with energy / grad / hessvec for oracle/l2hmc_train_oracle.py `training_loss_and_grad(..., target=)`), the cases
of the issue and the quantities of one case with their gates.

Gates: the project's own -- `check_grads_per_tensor` defaults per tensor, loss 1e-4 relative, Lx 1e-4 relative, px 1e-4
absolute.  Where a quantity needs more (U is a float32 sum of up to n terms of order 0.7: at n = 1000 one rounding of U is
already 6e-5 in log p), its gate is 3 x the distance of the FLOAT32 NUMPY ORACLE from the float64 one on the same case, never
below the plain gate (`helpers.train_bracket`'s rule: the yardstick is the reference's arithmetic, not the kernel under test).

Run as a program (`python -m tests.logistic_train_case OUT.npz n d eps H N`) it writes the flat gradient of one
`LogisticTrainer.loss_and_grad` call, from whatever library L2HMC_DBG_LIB names: the two-schedule comparison."""
import sys

import numpy as np

from tests import helpers

PRIOR_VAR = 2.0
# (n, d, eps, H): n = 17 has one live row in its second block, n = 1 a block of 15 padded rows; d = 25 / 50 end inside a tile
CASES = [(1, 2, 0.1, 10), (17, 5, 0.1, 10), (200, 25, 0.05, 10), (1000, 25, 0.02, 10), (300, 50, 0.03, 10), (200, 25, 0.05, 15)]
T_CASE, N_CASE = 6, 48


class LogisticTarget(object):
    """U(w) = sum_i [softplus(x_i . w) - y_i x_i . w] + |w|^2 / (2 s2), rows of w = chains, at `dtype`."""

    def __init__(self, X, y, s2, dtype=np.float64):
        self.X, self.y, self.s2, self.dtype = np.asarray(X, dtype), np.asarray(y, dtype), dtype(s2), dtype

    def _s(self, w):
        L = np.asarray(w, self.dtype) @ self.X.T
        return L, self.dtype(0.5) * (self.dtype(1) + np.tanh(self.dtype(0.5) * L))

    def energy(self, w):
        w = np.asarray(w, self.dtype)
        L = w @ self.X.T
        return (np.logaddexp(self.dtype(0), L) - self.y * L).sum(1) + self.dtype(0.5) * (w * w).sum(1) / self.s2

    def grad(self, w):
        w = np.asarray(w, self.dtype)
        _, s = self._s(w)
        return (s - self.y) @ self.X + w / self.s2

    def hessvec(self, w, u):
        u = np.asarray(u, self.dtype)
        _, s = self._s(w)
        return (s * (self.dtype(1) - s) * (u @ self.X.T)) @ self.X + u / self.s2


def blr_data(n, d, seed=7, w_scale=1.5):
    """tests/test_gpu_logistic.py::blr_data (kept here so that the CPU tests need not import a GPU test module)"""
    rng = np.random.RandomState(seed)
    X = (rng.randn(n, d) * (1.0 / np.sqrt(d))).astype(np.float32)
    w = rng.randn(d) * w_scale
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X.astype(np.float64) @ w))).astype(np.float32)
    return X, y


def make_case(n, d, eps, H, N=N_CASE, T=T_CASE):
    """(g, X, y): nets / masks of `synthetic_case("gauss_diag", d, H, T, N, seed=d, eps)`, start states 0.5 randn, and the
    seeded z, momenta and directions of a training call"""
    g = helpers.synthetic_case("gauss_diag", d, H=H, T=T, N=N, seed=d, eps=eps)
    X, y = blr_data(n, d, seed=7)
    g["x"] = (0.5 * np.random.RandomState(2).randn(N, d)).astype(np.float32)
    rng = np.random.RandomState(3)
    g["z"] = rng.randn(N, d).astype(np.float32)
    for pre in ("x.", "z."):
        g[pre + "dir"] = rng.randint(0, 2, N).astype(np.uint8)
        g[pre + "v_fwd"] = rng.randn(N, d).astype(np.float32)
        g[pre + "v_bwd"] = rng.randn(N, d).astype(np.float32)
    return g, X, y


def draws_of(g):
    return {"z": g["z"], "x_dir": g["x.dir"], "z_dir": g["z.dir"],
            "x_v": np.where(g["x.dir"][:, None] != 0, g["x.v_fwd"], g["x.v_bwd"]),
            "z_v": np.where(g["z.dir"][:, None] != 0, g["z.v_fwd"], g["z.v_bwd"])}


def grads_of(ref):
    return {k: ref[k] for k in ref if k.startswith(("xnet.", "vnet.")) or k == "alpha"}


def oracle_pair(g, X, y, tau=None):
    """(loss64, ref64, yard): the float64 oracle of the case (on U / tau when tau is given) and, per quantity, the float32
    numpy oracle's distance from it -- per gradient tensor (max norm), 'loss' (absolute), 'Lx' (rel_err), 'px' (abs_err)"""
    from oracle import l2hmc_train_oracle as TO
    from tests.test_tempered_training_cpu import _Tempered

    def run(dtype):
        t = LogisticTarget(X, y, PRIOR_VAR, dtype)
        with np.errstate(all="ignore"):
            return TO.training_loss_and_grad(g, dtype, target=t if tau is None else _Tempered(t, tau))
    l64, r64 = run(np.float64)
    l32, r32 = run(np.float32)
    yard = {k: float(np.abs(np.asarray(r32[k], np.float64).reshape(np.shape(r64[k])) - np.asarray(r64[k], np.float64)).max())
            for k in grads_of(r64)}
    yard["loss"] = abs(float(l32) - float(l64))
    yard["Lx"] = helpers.rel_err(r32["Lx"], r64["Lx"])
    yard["px"] = helpers.abs_err(r32["px"], r64["px"])
    return float(l64), r64, yard


def check_case(label, loss, Lx, px, got, l64, r64, yard):
    """every quantity of one call against the float64 oracle at its gate (module docstring); prints each figure first.
    Returns the worst ratio err / gate over everything."""
    e_loss, g_loss = abs(float(loss) - l64), max(1e-4 * max(1.0, abs(l64)), 3.0 * yard["loss"])
    e_x, g_x = helpers.rel_err(Lx, r64["Lx"]), max(1e-4, 3.0 * yard["Lx"])
    e_p, g_p = helpers.abs_err(px, r64["px"]), max(1e-4, 3.0 * yard["px"])
    print("%s: loss %.6e (ref %.6e) err %.2e / gate %.2e;  Lx %.2e / %.2e;  px %.2e / %.2e (float32 oracle: %.2e)"
          % (label, float(loss), l64, e_loss, g_loss, e_x, g_x, e_p, g_p, yard["px"]))
    assert e_loss < g_loss, (label, "loss", e_loss, g_loss)
    assert e_x < g_x, (label, "Lx", e_x, g_x)
    assert e_p < g_p, (label, "px", e_p, g_p)
    worst = helpers.check_grads_per_tensor(label, got, grads_of(r64), yard=yard, yard_factor=3.0)
    print("%s: worst tensor %s at %.2f of its gate" % (label, worst[1], worst[0]))
    return max(worst[0], e_loss / g_loss, e_x / g_x, e_p / g_p)


def hip_trainer(g, X, y, tau=None):
    """(dyn, LogisticTrainer) on the fused target with the case's nets, mask and step size (alpha trained, as the notebook does)"""
    import torch
    from l2hmc_amd import Dynamics, LogisticRegression, LogisticTrainer, layers
    from oracle import l2hmc_oracle as O
    d, T, H = int(g["x_dim"]), int(g["T"]), int(g["H"])
    e = LogisticRegression(X, y, prior_var=PRIOR_VAR).get_energy_function()
    dyn = Dynamics(d, e, T=T, eps=float(g["eps"]), net_factory=layers.stq_network(H), use_temperature=tau is not None)
    if tau is not None:
        dyn.temperature = tau
    dyn.mask = g["mask"]
    with torch.no_grad():
        dyn.alpha.fill_(float(np.log(g["eps"])))
        for w, pre in ((dyn._xw, "xnet."), (dyn._vw, "vnet.")):
            for k in O.NET_KEYS:
                w[k].copy_(torch.as_tensor(g[pre + k]).reshape(w[k].shape))
    return dyn, LogisticTrainer(dyn)


if __name__ == "__main__":
    out, n, d, eps, H, N = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
    import os
    from l2hmc_amd import _ffi
    if os.environ.get("L2HMC_DBG_LIB"):                              # (as tools/train_slots_dump.py: before the library loads)
        _ffi.LIB_PATH = os.path.abspath(os.environ["L2HMC_DBG_LIB"])
    g, X, y = make_case(n, d, eps, H, N=N)
    dyn, tr = hip_trainer(g, X, y)
    loss, Lx, px = tr.loss_and_grad(helpers.to_dev(g["x"]), draws=draws_of(g))
    np.savez(out, flat=helpers.to_np(tr.flat), Lx=helpers.to_np(Lx), px=helpers.to_np(px), loss=float(loss),
             kernel=_ffi.last_kernel())
