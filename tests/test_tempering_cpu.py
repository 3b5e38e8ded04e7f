"""Parallel tempering without a GPU: the C ABI declares and exports the ladder entry point and its struct, the Python side
refuses what the ladder kernel does not run, and the numpy restatement of the swap sweep (tests/pt_reference.py) -- the yardstick
of tests/test_gpu_tempering.py -- is itself pinned: it keeps every rung's marginal and counts round trips as documented."""
import ctypes
import os
import re

import numpy as np
import pytest

from l2hmc_amd import _ffi
from l2hmc_amd import distributions as D
from tests import ladder_cases as LC
from tests import pt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ladder_symbol_and_struct_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    assert re.search(r"\bint l2hmc_trajectory_ladder\s*\(", hdr)
    assert "L2HMC_STRUCT_LADDER_ARGS = 8" in hdr
    assert "l2hmc_trajectory_ladder" in _ffi.SYMBOLS
    assert _ffi.STRUCTS[8] is _ffi.L2hmcLadderArgs
    L = _ffi.lib()
    assert hasattr(L, "l2hmc_trajectory_ladder")
    assert L.l2hmc_struct_bytes(8) == ctypes.sizeof(_ffi.L2hmcLadderArgs) == 16 + 64 + 8 + 8 * 8
    assert L.l2hmc_struct_bytes(99) == -1
    assert L.l2hmc_abi_version() == 6


def _traj_args(N=16, d=2):
    a = _ffi.L2hmcTrajectoryArgs()
    a.n_chains, a.d, a.T, a.n_steps = N, d, 4, 4
    a.x = a.masks = a.trig = a.u = 64          # (never dereferenced: every case below fails on the host)
    a.rng_flags = _ffi.RNG_V
    a.eps_host = 0.1
    a.energy.kind, a.energy.temperature = _ffi.ENERGY_GAUSS_DIAG, 1.0
    a.energy.mu = a.energy.prec = 64
    return a


def _ladder(K=4, temps=None):
    lg = _ffi.L2hmcLadderArgs()
    lg.n_rungs, lg.n_rounds, lg.proposals_per_round = K, 1, 1
    for i, t in enumerate(temps if temps is not None else [1.0 + i for i in range(min(K, 16))]):
        lg.temperatures[i] = t
    lg.rung_of_row = 64
    return lg


@pytest.mark.parametrize("case, code, msg", [
    (dict(K=3), -1, b"n_rungs"),
    (dict(K=32), -1, b"n_rungs"),
    (dict(temps=[1.0, 2.0, 1.5, 3.0]), -1, b"non-decreasing"),
    (dict(temps=[0.0, 1.0, 2.0, 3.0]), -1, b"positive"),
    (dict(temps=[1.0, 2.0, 3.0, float("inf")]), -1, b"finite"),
    (dict(N=18), -1, b"multiples"),
    (dict(offset=2), -1, b"multiples"),
    (dict(temperature=2.0), -1, b"temperature must be 1"),
    (dict(beta=0.5), -2, b"anneal_beta"),
    (dict(ais=True), -2, b"AIS"),
    (dict(variant=4), -2, b"variant"),
    (dict(variant=201), -2, b"variant"),
])
def test_ladder_argument_errors_are_raised_on_the_host(case, code, msg):
    L = _ffi.lib()
    a = _traj_args(N=case.get("N", 16))
    a.chain_offset = case.get("offset", 0)
    a.energy.temperature = case.get("temperature", 1.0)
    a.energy.anneal_beta = case.get("beta", 0.0)
    a.variant = case.get("variant", 0)
    if case.get("ais"):
        a.ais_beta = 64
    lg = _ladder(case.get("K", 4), case.get("temps"))
    assert L.l2hmc_trajectory_ladder(a, lg, None) == code
    assert msg in L.l2hmc_last_error()


def _dyn(d=2, hmc=True, H=10, energy=None):
    from l2hmc_amd import Dynamics, layers
    e = energy if energy is not None else D.Gaussian(np.zeros(d), np.eye(d)).get_energy_function()
    return Dynamics(d, e, T=5, eps=0.1, hmc=hmc, net_factory=None if hmc else layers.stq_network(H), device="cpu")


def test_python_side_validation():
    from l2hmc_amd import ParallelTempering, geometric_ladder
    t = geometric_ladder(1.0, 8.0, 4)
    assert t[0] == 1.0 and t[-1] == 8.0 and np.allclose(np.diff(np.log(t)), np.log(2.0))
    pt = ParallelTempering(_dyn(), t, 3)
    assert pt.N == 12 and pt.rung_of_row.tolist() == [0, 1, 2, 3] * 3 and pt.trip_state.abs().sum() == 0
    with pytest.raises(ValueError, match="2, 4, 8 or 16"):
        ParallelTempering(_dyn(), geometric_ladder(1.0, 8.0, 3), 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        ParallelTempering(_dyn(), [1.0, 3.0, 2.0, 4.0], 3)
    with pytest.raises(ValueError, match="positive"):
        ParallelTempering(_dyn(), [-1.0, 1.0], 3)
    with pytest.raises(ValueError, match="multiple"):
        ParallelTempering(_dyn(), t, 3, chain_offset=6)
    with pytest.raises(ValueError, match="n_ladders"):
        ParallelTempering(_dyn(), t, 0)
    with pytest.raises(ValueError, match=r"\(12, 2\)"):
        pt.run(np.zeros((10, 2), np.float32), 1)
    # the GEMM engine: a caller-supplied energy, nets wider than 15
    with pytest.raises(NotImplementedError, match="caller-supplied energy"):
        ParallelTempering(_dyn(energy=lambda x: (x * x).sum(1)), t, 3)
    with pytest.raises(NotImplementedError, match="wider than H = 15"):
        ParallelTempering(_dyn(hmc=False, H=20), t, 3)
    # the AIS bridge
    dyn = _dyn()
    dyn.anneal_beta = 0.5
    with pytest.raises(NotImplementedError, match="anneal_beta"):
        ParallelTempering(dyn, t, 3)
    with pytest.raises(NotImplementedError, match="anneal_beta"):
        dyn.run(np.zeros((12, 2), np.float32), None, 0, 5, n_proposals=1, ladder={})
    # nets within the fused range are accepted; state round-trips
    pt = ParallelTempering(_dyn(hmc=False, H=10), t, 3, seed=5)
    sd = pt.state_dict()
    sd["round"], sd["proposal"] = 7, 21
    sd["rung_of_row"] = sd["rung_of_row"].flip(0)
    pt.load_state_dict(sd)
    assert pt.round == 7 and pt.proposal == 21 and pt.rung_of_row.tolist() == [3, 2, 1, 0] * 3
    with pytest.raises(ValueError, match="different ladder"):
        ParallelTempering(_dyn(), [1.0, 2.0], 6).load_state_dict(sd)


def test_deo_sweep_keeps_every_rungs_marginal():
    """Exact per-rung sampling (x ~ N(0, T_k) on every rung, U = x^2 / 2), then one sweep: the states the rungs hold afterwards
    are still N(0, T_k) -- the swap rule is a Metropolis step on the product of the tempered targets.  A swap rule with the
    sign flipped hands the colder rungs the larger energies and fails by hundreds of standard errors."""
    rng = np.random.RandomState(0)
    temps = np.array([1.0, 1.7, 3.0, 5.0])
    nl, K = 100000, 4
    for rnd in (0, 1):
        labels = np.tile(rng.permutation(K), (nl, 1))
        x = rng.randn(nl, K) * np.sqrt(temps[labels])
        U = 0.5 * x * x
        u = rng.uniform(size=(nl, K // 2))
        for sign in (1.0, -1.0):
            new, acc, att, _ = ref.sweep(labels, sign * U, temps, rnd, u)
            assert np.all(np.sort(new, axis=1) == np.arange(K))
            assert att.sum() == nl * len(range(rnd & 1, K - 1, 2)) and 0 < acc.sum() < att.sum()
            z = [(np.mean(x[new == k] ** 2) - temps[k]) / (temps[k] * np.sqrt(2.0 / nl)) for k in range(K)]
            if sign > 0:
                assert max(abs(v) for v in z) < 5.0, (rnd, z)
            else:
                assert max(abs(v) for v in z) > 20.0, (rnd, z)
        # the even sweep touches pairs (0, 1), (2, 3); the odd one (1, 2) only
        _, _, att, _ = ref.sweep(labels, U, temps, rnd, u)
        assert att.tolist() == ([nl, 0, nl] if rnd == 0 else [0, nl, 0])


def test_deo_sweep_rule_and_nan():
    temps = [1.0, 2.0]
    labels = np.array([[0, 1], [1, 0], [0, 1]])
    U = np.array([[3.0, 1.0], [1.0, 3.0], [np.nan, 1.0]])
    # the row on rung 0 vs the row on rung 1: accept iff log u < (1 - 1/2) (U_a - U_b) = 1 in the first two ladders
    u = np.array([[np.exp(0.99)], [np.exp(1.01)], [0.5]])
    new, acc, att, _ = ref.sweep(labels, U, temps, 0, u)
    assert new.tolist() == [[1, 0], [1, 0], [0, 1]] and acc.tolist() == [1] and att.tolist() == [3]


def test_sweep_takes_the_near_tie_margin_as_a_scalar_or_per_ladder_and_pair():
    rng = np.random.RandomState(1)
    nl, K, temps = 500, 4, [1.0, 1.5, 2.5, 4.0]
    labels = np.stack([rng.permutation(K) for _ in range(nl)])
    U = rng.randn(nl, K) * 3.0
    u = rng.uniform(size=(nl, K // 2))
    for rnd in (0, 1):
        s = ref.sweep(labels, U, temps, rnd, u, tol=0.2)
        assert 0 < s[3].sum() < s[3].size
        for tol in (np.full((nl, K - 1), 0.2), np.full((1, K - 1), 0.2), np.full((nl, 1), 0.2), np.float32(0.2)):
            a = ref.sweep(labels, U, temps, rnd, u, tol=tol)
            assert all(np.array_equal(p, q) for p, q in zip(a, s))
        # a margin of its own per ladder and pair: near exactly where the scalar form of that entry's margin says so
        tol = rng.uniform(0.0, 0.5, size=(nl, K - 1))
        a = ref.sweep(labels, U, temps, rnd, u, tol=tol)
        assert all(np.array_equal(p, q) for p, q in zip(a[:3], s[:3]))                      # (decisions do not depend on it)
        for l, k in [(0, rnd), (7, rnd), (nl - 1, K - 2 if rnd == 0 else 1)]:
            assert a[3][l, k] == ref.sweep(labels, U, temps, rnd, u, tol=tol[l, k])[3][l, k]
        wide = np.where(np.arange(nl)[:, None] < nl // 2, np.inf, 0.0) * np.ones((1, K - 1))
        near = ref.sweep(labels, U, temps, rnd, u, tol=wide)[3]
        assert near[:nl // 2, rnd::2].all() and not near[nl // 2:].any() and not near[:, 1 - rnd::2].any()


def test_replay_follows_the_labels_it_is_given_and_skips_near_ties():
    """`replay` on a rung history made by `sweep` itself: everything is compared and the counters are the sweeps'; with the
    margin of one ladder set to infinity that ladder is left out; a wrong label in the history is reported."""
    import torch

    class Ladder(object):
        K, n_ladders = 4, 6
    rng = np.random.RandomState(2)
    K, nl, R, M, temps = 4, 6, 5, 2, [1.0, 1.5, 2.5, 4.0]
    x_hist = rng.randn(R * M, nl * K, 1) * 3.0
    u = rng.uniform(size=(R, nl, K // 2))
    labels0 = np.tile(np.arange(K), (nl, 1))
    lab, rh, acc, att = labels0, [], 0, 0
    trip, trips = np.zeros((nl, K), np.int64), np.zeros(nl, np.int64)
    for j in range(R):
        lab, a, t, _ = ref.sweep(lab, x_hist[j * M + M - 1, :, 0].reshape(nl, K), temps, j, u[j])
        rh.append(lab.reshape(-1))
        acc, att = acc + a, att + t
        trip, done = ref.update_trips(lab, trip, K)
        trips += done
    o = {"rung_hist": torch.as_tensor(np.asarray(rh, np.int8))}

    def U_of(xs):
        return xs[:, 0]
    got = ref.replay(Ladder, o, x_hist, U_of, temps, R, M, u, 0, labels0, tol=0.0)
    assert got[0] == R * nl and np.array_equal(got[1], acc) and np.array_equal(got[2], att) and np.array_equal(got[3], trips)
    got = ref.replay(Ladder, o, x_hist, U_of, temps, R, M, u, 0, labels0,
                     tol=lambda labels, U: np.where(np.arange(nl)[:, None] == 2, np.inf, 0.0) * np.ones((1, K - 1)))
    assert got[0] == R * nl - R
    bad = np.asarray(rh, np.int8)
    bad[1, [4, 5]] = bad[1, [5, 4]]
    with pytest.raises(AssertionError):
        ref.replay(Ladder, {"rung_hist": torch.as_tensor(bad)}, x_hist, U_of, temps, R, M, u, 0, labels0, tol=0.0)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_ladder_case_inputs_accept_and_reject_swaps_away_from_the_near_tie_margin(name):
    """The conditions tests/test_gpu_ladder_geometries.py puts on its inputs, from the float64 oracle energy of x0 alone."""
    c = LC.case(name)
    acc0, att0, near = c.check_inputs()
    assert 0 < acc0 < att0 and near < 0.01
    assert c.N % c.K == 0 and c.N <= 48 and (c.N % 16 != 0 or c.K == 16)        # a half-live last tile wherever K allows one
    assert LC.R * LC.M == 8 and LC.T == 5


def test_round_trip_counting_matches_a_hand_worked_sequence():
    K = 4
    # one ladder's labels after each sweep (rung of rows 0..3); the trips completed: row 0 at sweep 4 (top at 2) and 9 (top at 7),
    # row 2 at sweep 7 (top at 3), row 1 at sweep 12 (top at 10)
    seq = [[0, 1, 2, 3], [1, 0, 2, 3], [3, 0, 2, 1], [2, 0, 3, 1], [0, 1, 3, 2], [1, 0, 3, 2], [0, 1, 3, 2],
           [3, 1, 0, 2], [3, 1, 0, 2], [0, 1, 3, 2], [0, 3, 1, 2], [0, 2, 1, 3], [1, 0, 2, 3]]
    trip, total = np.zeros((1, K), np.int64), 0
    counts = []
    for lab in seq[1:]:
        trip, done = ref.update_trips(np.array([lab]), trip, K)
        counts.append(int(done[0]))
        total += int(done[0])
    assert counts == [0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1]
    assert total == 4
    assert ref.update_trips(np.array([[3, 2, 1, 0]]), np.array([[0, 0, 1, 1]]), K)[1].tolist() == [1]


def test_swap_uniforms_are_their_own_stream():
    a = ref.swap_uniforms(7, 5, 8, 3)
    assert a.shape == (5, 4) and np.all((a >= 0) & (a < 1)) and len(np.unique(a)) == 20
    assert np.array_equal(ref.swap_uniforms(7, 3, 8, 3, ladder0=2), a[2:])
    assert not np.array_equal(ref.swap_uniforms(7, 5, 8, 4), a)
    assert not np.array_equal(ref.swap_uniforms(8, 5, 8, 3), a)
