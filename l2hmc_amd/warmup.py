"""Warm-up: choose the step size eps = exp(alpha) of a `Dynamics` on the device, by dual averaging.

    x, info = warmup(x0, dyn, 100, seed=1)          # dyn.alpha now holds the adapted step size
    info.eps, info.accept, info.n_search, info.n_averaged

Every trajectory kernel reads eps = expf(*alpha) from device memory when it starts.  An update is therefore one launch of the
sampler loop (`sample_chain`: M = `proposals_per_update` proposals on all chains) and one `l2hmc_adapt_update`
(csrc/adapt.hip), which reduces the window's accept probabilities and rewrites `alpha` IN PLACE: the doubling search of
Hoffman & Gelman (2014) Alg. 4 on the mean accept probability over the chains until it crosses 0.5, then the dual averaging of
their Alg. 5 towards `target_accept`; `l2hmc_adapt_finish` sets the averaged step size.  include/l2hmc.h states the rules in
the order the kernel applies them (tests/warmup_case.py restates them in float64 numpy).  The loop copies nothing to the host
and never synchronises: state, trace and alpha stay on the device, and `info`'s properties read them back when asked.

Known limit.  With a fixed trajectory length T the accept rate of a low-dimensional Gaussian is not monotone in eps (resonances
where eps T is near a multiple of pi), so the averaged step size need not reach the target there: a numpy restatement gave
0.66 - 0.98 for target 0.65 on a standard normal in d = 2 and d = 8 at T = 10.  Jittering the step size would address it and is
not part of this module.
"""
import math

import torch

from . import _ffi
from ._history import launch
from .distributions import as_device_f32
from .sampler import sample_chain

STATE_DOUBLES = 16                    # L2HMC_ADAPT_STATE_DOUBLES
SINGLE_BLOCK_MAX = 65536              # L2HMC_ADAPT_SINGLE_BLOCK_MAX: windows up to this are one launch of one workgroup
REDUCE, APPLY = 1, 2                  # L2HMC_ADAPT_REDUCE, L2HMC_ADAPT_APPLY
STATE_FIELDS = ("phase", "dir", "t", "log_eps", "log_eps_bar", "H_bar", "mu", "accept", "updates", "target", "gamma", "t0",
                "kappa", "log_eps_min", "log_eps_max")


class WarmupInfo(object):
    """What `warmup` returns next to the state: the device tensors `state` (16 doubles, include/l2hmc.h) and `trace`
    ((n_updates, 4): mean accept, log eps the window ran at, log eps then set, phase after), `next_proposal0` (where a
    seeded run's Philox stream continues), and properties that copy to the host WHEN READ."""

    def __init__(self, state, trace, next_proposal0):
        self.state, self.trace, self.next_proposal0 = state, trace, next_proposal0

    def _host(self):
        return self.state.cpu().numpy()

    @property
    def log_eps(self):
        return float(self._host()[3])

    @property
    def eps(self):
        return math.exp(self.log_eps)

    @property
    def accept(self):
        """mean accept probability of the last window"""
        return float(self._host()[7])

    @property
    def n_search(self):
        """updates that ran in the search phase"""
        return int(self.trace.shape[0]) - self.n_averaged

    @property
    def n_averaged(self):
        """dual-averaging updates (the state's t)"""
        return int(self._host()[2])


def check_dynamics(dynamics):
    if dynamics.eps_override is not None:
        raise ValueError("warmup adapts the device-side alpha; this Dynamics has eps_override set, which bypasses it "
                         "(set eps_override = None)")
    a = dynamics.alpha
    if not (a.is_cuda and a.dtype == torch.float32 and a.numel() == 1):
        raise ValueError("Dynamics.alpha must be one float32 on the ROCm device")


def adapt_init(dynamics, search=True, target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, eps_bounds=(1e-8, 1e3)):
    """A fresh (16,) float64 device state for `dynamics.alpha` (`l2hmc_adapt_init`: alpha is read on the device)."""
    lo, hi = (float(b) for b in eps_bounds)
    if not (lo > 0.0 and hi > 0.0):
        raise ValueError("eps_bounds must be positive (got %r)" % (eps_bounds,))
    dev = dynamics.device
    state = torch.empty(STATE_DOUBLES, dtype=torch.float64, device=dev)
    launch(dev, _ffi.lib().l2hmc_adapt_init, state.data_ptr(), dynamics.alpha.data_ptr(), int(bool(search)),
           float(target_accept), float(gamma), float(t0), float(kappa), math.log(lo), math.log(hi))
    return state


def adapt_update(p, state, alpha, trace_row=None, *, mode=REDUCE | APPLY, sums2=None, workspace=None):
    """One `l2hmc_adapt_update` on the current stream: `p` the accept probabilities of the window just run (any shape, float32
    on the device; ignored with mode = APPLY), `state` / `alpha` rewritten in place."""
    n = 0
    if mode & REDUCE:
        p = as_device_f32(p, state.device if state is not None else None)
        n = p.numel()
        need = _ffi.check(_ffi.lib().l2hmc_adapt_workspace_doubles(n))
        if need and (workspace is None or workspace.numel() < need):
            workspace = torch.empty(need, dtype=torch.float64, device=p.device)
    launch(p.device if mode & REDUCE else state.device, _ffi.lib().l2hmc_adapt_update, _ffi.ptr(p) if mode & REDUCE else None,
           n, int(mode), _ffi.ptr(sums2), _ffi.ptr(state), _ffi.ptr(alpha), _ffi.ptr(trace_row), _ffi.ptr(workspace))
    return workspace


def adapt_finish(state, alpha):
    launch(state.device, _ffi.lib().l2hmc_adapt_finish, state.data_ptr(), alpha.data_ptr())


def warmup(x, dynamics, n_updates=100, *, proposals_per_update=1, target_accept=0.8, search=True, gamma=0.05, t0=10.0,
           kappa=0.75, eps_bounds=(1e-8, 1e3), seed=None, proposal0=0, chain_offset=0, aux=None, _allreduce=None):
    """Adapt `dynamics`' step size on chains started at `x` (N, d); returns (x after the warm-up, `WarmupInfo`).

    n_updates windows of `proposals_per_update` proposals each; `search=False` skips the doubling search (start near a
    sensible step size then); gamma, t0, kappa are the dual-averaging constants of Hoffman & Gelman (2014) and `eps_bounds`
    clamps the step size.  Randomness as in `sample_chain`: with `seed=` the Philox stream, advancing by
    `proposals_per_update` per update from `proposal0` (continue a run at `info.next_proposal0`), else torch's generator.
    Works wherever alpha is read from the device -- HMC mode and S/T/Q nets, every built-in target, the GEMM engine and
    caller-supplied energies / nets -- and refuses a Dynamics with `eps_override` set."""
    check_dynamics(dynamics)
    n_updates, M = int(n_updates), int(proposals_per_update)
    if n_updates < 1 or M < 1:
        raise ValueError("n_updates and proposals_per_update must be >= 1")
    dynamics._check_aux(aux)
    x = as_device_f32(x, dynamics.device)
    dev = dynamics.device
    # alpha is written through its existing storage: a Parameter keeps its identity, a Trainer's flat theta (a view of the same
    # storage) sees the new value.  No `invalidate_caches()`: no prepared copy holds eps -- the packed weight fragments and the
    # GEMM engine's workspace are keyed on the NET parameters, and every kernel reads *alpha itself when it starts.
    alpha = dynamics.alpha.detach()
    state = adapt_init(dynamics, search, target_accept, gamma, t0, kappa, eps_bounds)
    trace = torch.zeros((n_updates, 4), dtype=torch.float64, device=dev)
    need = _ffi.check(_ffi.lib().l2hmc_adapt_workspace_doubles(M * x.shape[0]))
    ws = torch.empty(need, dtype=torch.float64, device=dev) if need else None
    sums2 = torch.zeros(2, dtype=torch.float64, device=dev) if _allreduce is not None else None
    for k in range(n_updates):
        x, p, _ = sample_chain(x, dynamics, M, seed=seed, proposal0=int(proposal0) + k * M, chain_offset=chain_offset, aux=aux)
        if _allreduce is None:
            adapt_update(p, state, alpha, trace[k], workspace=ws)
        else:                       # ranks: every rank applies the same two doubles, so every rank holds bit-identical state
            adapt_update(p, None, None, mode=REDUCE, sums2=sums2, workspace=ws)
            _allreduce(sums2)
            adapt_update(None, state, alpha, trace[k], mode=APPLY, sums2=sums2)
    adapt_finish(state, alpha)
    return x, WarmupInfo(state, trace, int(proposal0) + n_updates * M)
