"""Parallel tempering (replica exchange) over a temperature ladder, inside the persistent sampler loop.

K copies of every chain run at temperatures T_0 <= ... <= T_{K-1}; after every `proposals_per_round` proposals the
neighbouring rungs of each ladder swap states by the Metropolis rule

    accept (k, k + 1)  iff  log u < (1 / T_k - 1 / T_{k+1}) (U_a - U_b)

(U the untempered energy of the rows a, b holding rungs k, k + 1), in a deterministic even-odd sweep: round g proposes the
pairs k = g mod 2, g mod 2 + 2, ...  Rows never move -- a swap exchanges the rows' rung labels -- and a ladder of K <= 16 rungs
lies inside one 16-chain tile of the trajectory kernel, so the sweep is LDS work between two proposals of the same launch
(`l2hmc_trajectory_ladder`, include/l2hmc.h).  The cold rung (T_0) is the sample.

Layout: N = n_ladders * K rows, row r in ladder r // K, its temperature temperatures[rung_of_row[r]].  Proposal draws are keyed
by (seed, global chain, proposal index), swap uniforms by (seed, global ladder, round) -- splitting the ladders over launches or
ranks (`chain_offset`, a multiple of K) gives the same bits.
"""
import math

import numpy as np
import torch

from .distributions import as_device_f32

RUNGS = (2, 4, 8, 16)


def geometric_ladder(t_min, t_max, K):
    """K temperatures from t_min to t_max in geometric progression (both ends exact)."""
    K = int(K)
    if K < 2:
        raise ValueError("a ladder has at least 2 rungs")
    t_min, t_max = float(t_min), float(t_max)
    if not (0.0 < t_min <= t_max < math.inf):
        raise ValueError("need 0 < t_min <= t_max < inf")
    r = (t_max / t_min) ** (1.0 / (K - 1))
    return [t_min] + [t_min * r ** k for k in range(1, K - 1)] + [t_max]


def _check_temperatures(temperatures):
    t = [float(v) for v in temperatures]
    if len(t) not in RUNGS:
        raise ValueError("a ladder has 2, 4, 8 or 16 rungs (got %d)" % len(t))
    t32 = np.asarray(t, dtype=np.float32)
    if not (np.all(np.isfinite(t32)) and np.all(t32 > 0) and np.all(np.diff(t32) >= 0)):
        raise ValueError("ladder temperatures must be positive, finite and non-decreasing: %r" % (t,))
    return [float(v) for v in t32]


class ParallelTempering(object):
    """Replica exchange for `dynamics` over `temperatures` (K in {2, 4, 8, 16}), `n_ladders` ladders.

    `dynamics.temperature` and `use_temperature` are ignored under a ladder: every row runs at its rung's temperature.  The
    fused trajectory kernel carries it (HMC or S/T/Q nets with H <= 15, the built-in targets); a Dynamics on the GEMM engine
    (VAE posterior, caller-supplied energies or nets, wider nets) and the AIS bridge (`anneal_beta`) are refused.

    State that persists across `run` calls (and `state_dict` / `load_state_dict`): the rung labels, the round-trip states, the
    round counter and the proposal counter of the Philox stream."""

    def __init__(self, dynamics, temperatures, n_ladders, *, seed=0, chain_offset=0):
        self.dynamics = dynamics
        self.temperatures = _check_temperatures(temperatures)
        self.K = len(self.temperatures)
        self.n_ladders = int(n_ladders)
        if self.n_ladders < 1:
            raise ValueError("n_ladders must be >= 1")
        self.chain_offset = int(chain_offset)
        if self.chain_offset < 0 or self.chain_offset % self.K:
            raise ValueError("chain_offset must be a non-negative multiple of the number of rungs (%d)" % self.K)
        dynamics._check_ladder()
        self.seed = int(seed)
        self.N = self.n_ladders * self.K
        dev = dynamics.device
        self.rung_of_row = (torch.arange(self.N, device=dev) % self.K).to(torch.int8)
        self.trip_state = torch.zeros(self.N, dtype=torch.int8, device=dev)
        self.round = 0          # global index of the next round
        self.proposal = 0       # Philox proposal index of the next proposal

    # ---- state -----------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {'temperatures': list(self.temperatures), 'n_ladders': self.n_ladders, 'seed': self.seed,
                'chain_offset': self.chain_offset, 'round': self.round, 'proposal': self.proposal,
                'rung_of_row': self.rung_of_row.cpu().clone(), 'trip_state': self.trip_state.cpu().clone()}

    def load_state_dict(self, sd):
        if list(map(float, sd['temperatures'])) != self.temperatures or int(sd['n_ladders']) != self.n_ladders:
            raise ValueError("state of a different ladder")
        rr, ts = torch.as_tensor(sd['rung_of_row']), torch.as_tensor(sd['trip_state'])
        if tuple(rr.shape) != (self.N,) or tuple(ts.shape) != (self.N,):
            raise ValueError("rung_of_row / trip_state must be (%d,)" % self.N)
        self.seed, self.chain_offset = int(sd['seed']), int(sd['chain_offset'])
        self.round, self.proposal = int(sd['round']), int(sd['proposal'])
        self.rung_of_row = rr.to(device=self.dynamics.device, dtype=torch.int8).clone()
        self.trip_state = ts.to(device=self.dynamics.device, dtype=torch.int8).clone()

    # ---- sampling ----------------------------------------------------------------------------------------------------
    def x_by_rung(self, x):
        """(K, n_ladders, d): the state of every rung of every ladder, from the row-ordered (N, d) states."""
        x = as_device_f32(x, self.dynamics.device)
        d = x.shape[1]
        inv = torch.argsort(self.rung_of_row.view(self.n_ladders, self.K).long(), dim=1)       # row of rung k
        xl = x.view(self.n_ladders, self.K, d)
        return torch.gather(xl, 1, inv.unsqueeze(2).expand(-1, -1, d)).transpose(0, 1).contiguous()

    def run(self, x, n_rounds, proposals_per_round=1, record_cold=False, record_rungs=False, u=None, *,
            draws=None, record_states=False):
        """`n_rounds` rounds of `proposals_per_round` proposals + one swap sweep each, in ONE kernel launch.

        x: (N, d) row-ordered states (N = n_ladders K).  u: optional (R, n_ladders, K / 2) swap uniforms (pair (k, k + 1) at
        index k // 2); else the Philox stream.  draws: optional {'v': (R M, N, d), 'direction': (R M, N), 'u': (R M, N)}
        proposal draws; what is not given comes from the Philox stream.  Returns a dict: x (N, d) by row, x_by_rung
        (K, n_ladders, d), p (R M, N), cold_hist (R M, n_ladders, d) if record_cold, rung_hist (R, N) int8 if record_rungs,
        x_hist (R M, N, d) if record_states, swap_rate (K - 1) and the counts behind it (swaps_accepted / swaps_attempted),
        round_trips (n_ladders): this run's completed round trips."""
        dyn = self.dynamics
        dyn._check_ladder()
        R, M = int(n_rounds), int(proposals_per_round)
        if R < 1 or M < 1:
            raise ValueError("n_rounds and proposals_per_round must be >= 1")
        if tuple(np.shape(x) if not isinstance(x, torch.Tensor) else x.shape) != (self.N, dyn.x_dim):
            raise ValueError("x must be (n_ladders * K, d) = (%d, %d)" % (self.N, dyn.x_dim))
        x = as_device_f32(x, dyn.device)
        RM, nl, K, dev = R * M, self.n_ladders, self.K, dyn.device
        f32 = dict(dtype=torch.float32, device=dev)
        spec = {'temperatures': self.temperatures, 'rounds': R, 'proposals_per_round': M, 'round0': self.round,
                'rung_of_row': self.rung_of_row, 'trip_state': self.trip_state,
                'accepted': torch.zeros(K - 1, dtype=torch.int64, device=dev),
                'attempted': torch.zeros(K - 1, dtype=torch.int64, device=dev),
                'round_trips': torch.zeros(nl, dtype=torch.int64, device=dev)}
        if u is not None:
            spec['swap_u'] = as_device_f32(u, dev).reshape(R, nl, K // 2).contiguous()
        if record_cold:
            spec['cold_hist'] = torch.empty((RM, nl, dyn.x_dim), **f32)
        if record_rungs:
            spec['rung_hist'] = torch.empty((R, self.N), dtype=torch.int8, device=dev)
        draws = draws or {}
        lead = (RM,) if RM > 1 else ()
        v = draws.get('v')
        if v is not None:
            v = as_device_f32(v, dev).reshape(lead + (self.N, dyn.x_dim))
        pu = draws.get('u')
        if pu is not None:
            pu = as_device_f32(pu, dev).reshape(lead + (self.N,))
        direction = None if dyn.hmc else draws.get('direction')
        if direction is not None:
            direction = torch.as_tensor(direction, device=dev).to(torch.uint8).reshape(lead + (self.N,))
        rng = {'seed': self.seed, 'proposal0': self.proposal, 'chain_offset': self.chain_offset}
        want = ('p', 'x_next') + (('x_hist',) if record_states else ())
        o = dyn.run(x, v, 0, dyn.T, direction=direction, direction_all=1, u=pu, want=want, n_proposals=RM, rng=rng,
                    ladder=spec)
        self.round += R
        self.proposal += RM
        acc, att = spec['accepted'], spec['attempted']
        out = {'x': o['x_next'], 'x_by_rung': self.x_by_rung(o['x_next']), 'p': o['p'].reshape(RM, self.N),
               'swap_rate': acc.double() / att.clamp(min=1).double(), 'swaps_accepted': acc, 'swaps_attempted': att,
               'round_trips': spec['round_trips'], 'cold_hist': spec.get('cold_hist'), 'rung_hist': spec.get('rung_hist')}
        if record_states:
            out['x_hist'] = o['x_hist']
        return out
