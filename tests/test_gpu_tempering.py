"""GPU: parallel tempering on the ladder form of the general trajectory kernel (l2hmc_trajectory_ladder).

Equal rungs are the scalar-temperature path bit for bit; distinct rungs match the float32 oracle's propose at each rung's
temperature; swap decisions, counters and round trips match the numpy restatement (tests/pt_reference.py) replayed on the
kernel's own states; a ladder started in its stationary distribution stays there; PT recovers the weights of a two-mode mixture
that HMC at T = 1 cannot cross; and the bits do not depend on how the ladders are split over launches or calls."""
import numpy as np
import pytest
import torch

from l2hmc_amd import Dynamics, ParallelTempering, geometric_ladder, sample_chain
from l2hmc_amd import distributions as D
from oracle import l2hmc_oracle as O
from tests import helpers
from tests import pt_reference as ref

pytestmark = pytest.mark.gpu


def _hmc_twin(g, variant=100):
    """HMC-mode Dynamics on a golden's energy, step size and schedule length."""
    d = int(g["x_dim"])
    dyn = Dynamics(d, helpers.hip_energy(g), T=int(g["T"]), eps=float(g["eps"]), hmc=True)
    dyn.eps_override = float(g["eps"])
    dyn.variant = variant
    return dyn


def _rows(g, N, seed=0):
    rng = np.random.RandomState(seed)
    x = np.asarray(g["x"], np.float32)
    return (x[rng.randint(0, x.shape[0], size=N)] + 0.1 * rng.randn(N, x.shape[1])).astype(np.float32)


@pytest.mark.parametrize("case", ["tilted8", "mog2d", "rough8"])
@pytest.mark.parametrize("hmc", [False, True])
def test_equal_rungs_are_the_scalar_path_bit_for_bit(case, hmc):
    g = helpers.load(case)
    dyn = _hmc_twin(g) if hmc else helpers.hip_dynamics(g, variant=100)
    K, nl, R, M = 4, 64, 3, 2
    x0 = helpers.to_dev(_rows(g, K * nl))
    dyn.use_temperature, dyn.temperature = True, 2.5
    xs, ps, _ = sample_chain(x0, dyn, R * M, seed=11)
    dyn.use_temperature, dyn.temperature = False, 1.0              # (ignored under a ladder either way)
    pt = ParallelTempering(dyn, [2.5] * K, nl, seed=11)
    o = pt.run(x0, R, M, record_rungs=True)
    torch.cuda.synchronize()
    assert torch.equal(o["x"], xs) and torch.equal(o["p"], ps)
    # equal rungs: every proposed swap is accepted (log u < 0), and the labels move
    assert torch.equal(o["swaps_accepted"], o["swaps_attempted"]) and int(o["swaps_attempted"].sum()) > 0


@pytest.mark.parametrize("case", ["tilted8", "mog2d"])
def test_each_rung_matches_the_oracle_at_its_temperature(case):
    g = helpers.load(case)
    dyn = helpers.hip_dynamics(g, variant=100)
    temps, nl = [1.0, 1.5, 2.5, 4.0], 16
    K, N, d = 4, 64, int(g["x_dim"])
    rng = np.random.RandomState(3)
    x = _rows(g, N, 1)
    v = rng.randn(N, d).astype(np.float32)
    dr = rng.randint(0, 2, size=N).astype(np.uint8)
    u = rng.uniform(size=N).astype(np.float32)
    pt = ParallelTempering(dyn, temps, nl, seed=0)
    o = pt.run(helpers.to_dev(x), 1, 1, draws={"v": v, "direction": dr, "u": u})
    xn, p = helpers.to_np(o["x"]), helpers.to_np(o["p"])[0]
    od = helpers.oracle_dynamics(g)
    for k, T in enumerate(temps):
        rows = np.arange(k, N, K)                                   # initial labels r % K
        od.temperature = np.float32(T)
        rLx, _, rpx, _ = O.propose(x[rows], od, v[rows], v[rows], dr[rows], u[rows], both_directions=False)
        assert helpers.abs_err(p[rows], rpx) < 1e-4, (k, helpers.abs_err(p[rows], rpx))
        helpers.check_x_next(xn[rows], x[rows], rLx, rpx, u[rows], 1e-4)


@pytest.mark.parametrize("injected", [True, False])
def test_swap_decisions_counters_and_round_trips_match_the_reference(injected):
    g = helpers.load("mog2d")
    dyn = helpers.hip_dynamics(g, variant=100)
    temps, nl, K, R, M = geometric_ladder(1.0, 6.0, 8), 32, 8, 24, 2
    pt = ParallelTempering(dyn, temps, nl, seed=21)
    rng = np.random.RandomState(5)
    u_inj = rng.uniform(size=(R, nl, K // 2)).astype(np.float32) if injected else None
    x0 = helpers.to_dev(_rows(g, K * nl, 2))
    o = pt.run(x0, R, M, record_rungs=True, record_states=True, u=u_inj)
    x_hist = o["x_hist"]

    def U_of(xs):
        return helpers.to_np(dyn.energy(xs)).astype(np.float64)        # T = 1 (use_temperature off)
    t32 = np.asarray(temps, np.float32).astype(np.float64)
    compared, acc, att, trips = ref.replay(pt, o, x_hist, U_of, t32, R, M, u_inj, 21, np.tile(np.arange(K), (nl, 1)), tol=1e-5)
    assert compared >= 0.95 * R * nl
    assert np.array_equal(att, helpers.to_np(o["swaps_attempted"]))
    assert np.abs(acc - helpers.to_np(o["swaps_accepted"])).sum() <= R * nl - compared
    assert np.array_equal(trips, helpers.to_np(o["round_trips"]))
    assert np.array_equal(helpers.to_np(pt.rung_of_row).astype(np.int64), helpers.to_np(o["rung_hist"][-1]).astype(np.int64))
    assert int(trips.sum()) > 0 and 0 < int(acc.sum()) < int(att.sum())


def test_a_ladder_started_in_its_stationary_distribution_stays_there():
    """Diagonal Gaussian, every rung started exactly from N(0, T_k Sigma): after 200 rounds each rung's mean and variance are
    within 5 standard errors of 0 and T_k Sigma (a sign error in the swap rule hands the cold rungs the hot states)."""
    d, nl, K = 4, 4096, 4
    var = np.array([1.0, 0.5, 2.0, 1.0])
    e = D.Gaussian(np.zeros(d), np.diag(var)).get_energy_function()
    dyn = Dynamics(d, e, T=5, eps=0.3, hmc=True)
    dyn.eps_override = 0.3
    temps = [1.0, 2.0, 4.0, 8.0]
    pt = ParallelTempering(dyn, temps, nl, seed=4)
    rng = np.random.RandomState(9)
    lab = np.arange(nl * K) % K
    x0 = (rng.randn(nl * K, d) * np.sqrt(np.asarray(temps)[lab][:, None] * var[None, :])).astype(np.float32)
    o = pt.run(helpers.to_dev(x0), 200, 1)
    xr = helpers.to_np(o["x_by_rung"]).astype(np.float64)
    assert float(o["swap_rate"].min()) > 0.05
    for k, T in enumerate(temps):
        s2 = T * var
        zm = xr[k].mean(axis=0) / np.sqrt(s2 / nl)
        zv = (xr[k].var(axis=0) - s2) / (s2 * np.sqrt(2.0 / nl))
        assert np.all(np.abs(zm) < 5) and np.all(np.abs(zv) < 5), (k, zm, zv)


# The mixing yardstick: two unit-variance modes at x0 = -5 (weight 0.7) and +5 (0.3).  The barrier between them is 12.5 nats at
# T = 1, which HMC with eps = 0.5, 10 leapfrog steps does not cross; the ladder T = 1 ... 40 (8 rungs, geometric) flattens it to
# 0.3 nats at the top.  1024 ladders, 1500 rounds of one proposal, the second half of the cold rung's history is the sample.
MIX_LADDER, MIX_EPS, MIX_STEPS, MIX_ROUNDS, MIX_LADDERS = geometric_ladder(1.0, 40.0, 8), 0.5, 10, 1500, 1024


def _two_modes():
    e = D.GMM([np.array([-5.0, 0.0]), np.array([5.0, 0.0])], [np.eye(2), np.eye(2)], [0.7, 0.3]).get_energy_function()
    dyn = Dynamics(2, e, T=MIX_STEPS, eps=MIX_EPS, hmc=True)
    dyn.eps_override = MIX_EPS
    dyn.variant = 100
    return dyn


def test_pt_recovers_the_mode_weights_that_hmc_at_t1_cannot():
    dyn = _two_modes()
    K, nl = len(MIX_LADDER), MIX_LADDERS
    rng = np.random.RandomState(0)
    x0 = (np.array([-5.0, 0.0]) + rng.randn(nl * K, 2)).astype(np.float32)          # every chain in the heavy mode
    pt = ParallelTempering(dyn, MIX_LADDER, nl, seed=1)
    o = pt.run(helpers.to_dev(x0), MIX_ROUNDS, 1, record_cold=True)
    cold = helpers.to_np(o["cold_hist"])[MIX_ROUNDS // 2:]
    frac = float((cold[..., 0] > 0).mean())
    assert abs(frac - 0.3) < 0.03, frac
    assert int(o["round_trips"].sum()) > nl
    xs, _, _ = sample_chain(helpers.to_dev(x0), dyn, MIX_ROUNDS, seed=1)
    plain = float((helpers.to_np(xs)[:, 0] > 0).mean())
    assert plain < 0.01, plain


def test_reproducible_across_calls_seeds_and_launch_splits():
    g = helpers.load("mog2d")
    dyn = helpers.hip_dynamics(g, variant=100)
    temps, nl, R = [1.0, 1.6, 2.6, 4.0], 64, 8
    K, N = 4, 4 * 64
    x0 = helpers.to_dev(_rows(g, N, 4))

    def full(R1=None):
        pt = ParallelTempering(dyn, temps, nl, seed=77)
        if R1 is None:
            o = pt.run(x0, R, 2, record_cold=True)
            return o, pt
        a = pt.run(x0, R1, 2)
        b = pt.run(a["x"], R - R1, 2)
        return b, pt

    o1, p1 = full()
    o2, p2 = full()
    assert torch.equal(o1["x"], o2["x"]) and torch.equal(o1["p"], o2["p"]) and torch.equal(p1.rung_of_row, p2.rung_of_row)
    assert torch.equal(o1["cold_hist"], o2["cold_hist"])
    o3, p3 = full(R // 2)
    assert torch.equal(o3["x"], o1["x"]) and torch.equal(p3.rung_of_row, p1.rung_of_row)
    assert torch.equal(o3["p"], o1["p"][R:]) and torch.equal(p3.trip_state, p1.trip_state)
    # two half-size launches, the second at chain_offset = N / 2
    ha = ParallelTempering(dyn, temps, nl // 2, seed=77)
    hb = ParallelTempering(dyn, temps, nl // 2, seed=77, chain_offset=N // 2)
    oa, ob = ha.run(x0[:N // 2], R, 2), hb.run(x0[N // 2:], R, 2)
    assert torch.equal(torch.cat([oa["x"], ob["x"]]), o1["x"]) and torch.equal(torch.cat([oa["p"], ob["p"]], 1), o1["p"])
    assert torch.equal(torch.cat([ha.rung_of_row, hb.rung_of_row]), p1.rung_of_row)
    assert torch.equal(oa["swaps_attempted"] + ob["swaps_attempted"], o1["swaps_attempted"])
    assert torch.equal(oa["swaps_accepted"] + ob["swaps_accepted"], o1["swaps_accepted"])
    # another seed, other bits
    o4 = ParallelTempering(dyn, temps, nl, seed=78).run(x0, R, 2)
    assert not torch.equal(o4["x"], o1["x"])
