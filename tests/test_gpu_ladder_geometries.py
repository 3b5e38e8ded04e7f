"""GPU: the ladder form of the general trajectory kernel (`traj_ladder_kernel<EK, DT, NW, KH>`, l2hmc_amd/csrc/traj_body.inc
under `if constexpr (LAD)`) with DISTINCT rung temperatures on every compiled geometry, energy kind, hidden k-step count and rung
count -- tests/ladder_cases.py is the table.  Per case, one ladder launch (R = 4 rounds of M = 2 proposals, injected draws and
swap uniforms, a half-live last tile) is held to

  a. chained launches of the scalar-temperature path, bit for bit: after an accepted swap that holds only if the re-evaluated
     grad U / T, U / T and VNet layer-1 partial are exactly what a fresh prologue computes at the new temperature;
  b. the numpy restatement of the sweep (tests/pt_reference.py) replayed on the kernel's own states: decisions, counters, round
     trips, final labels;
  c. cold_hist = the label-0 row of x_hist, bit for bit (the label after the sweep on a round's last proposal);
  d. (four cases) the first proposal after a sweep against the float32 oracle at each row's new temperature.

Outside the table: a chain_offset that is a multiple of K but not of 16, resuming through state_dict() on a fresh
ParallelTempering, nothing written past row N, and a non-finite row that rejects its swaps and stays in its lane.
"""
import numpy as np
import pytest
import torch

from l2hmc_amd import ParallelTempering, _ffi
from oracle import l2hmc_oracle as O
from tests import helpers
from tests import ladder_cases as LC
from tests import pt_reference as ref
from tests.helpers import to_dev, to_np

pytestmark = pytest.mark.gpu

R, M, T = LC.R, LC.M, LC.T
_runs = {}


def _get(name):
    """The case's one ladder launch, shared by the tests over the table: (case, dynamics, ladder, device outputs, host copies)."""
    if name not in _runs:
        c = LC.case(name)
        c.check_inputs()                                            # (CPU: float64 oracle energies of x0)
        dyn = c.hip_dynamics()
        pt = ParallelTempering(dyn, c.temps, c.nl, seed=0)
        draws = {"v": c.v, "direction": c.dr, "u": c.u}
        o = pt.run(to_dev(c.x0), R, M, record_cold=True, record_rungs=True, u=c.swap_u, draws=draws, record_states=True)
        torch.cuda.synchronize()
        kernel = _ffi.last_kernel()
        h = {k: to_np(o[k]) for k in ("x", "p", "x_hist", "cold_hist", "swaps_accepted", "swaps_attempted", "round_trips")}
        h["rung_hist"] = to_np(o["rung_hist"]).astype(np.int64)
        h["kernel"] = kernel
        _runs[name] = (c, dyn, pt, o, h)
    c, dyn, pt, o, h = _runs[name]
    assert h["kernel"] == c.kernel, (name, h["kernel"])
    # an accepted swap between distinct temperatures is what enters the re-evaluation; a rejected one must leave the row alone
    assert 0 < int(h["swaps_accepted"].sum()) < int(h["swaps_attempted"].sum()), (name, h["swaps_accepted"], h["swaps_attempted"])
    return _runs[name]


def _labels_before(c, h, j):
    """row labels in front of round j"""
    return c.labels0.reshape(-1) if j == 0 else h["rung_hist"][j - 1]


@pytest.mark.parametrize("name", list(LC.CASES))
def test_a_ladder_launch_is_chained_scalar_temperature_launches_bit_for_bit(name):
    c, dyn, pt, o, h = _get(name)
    x0, v, u = to_dev(c.x0), to_dev(c.v), to_dev(c.u)
    dr = None if c.hmc else to_dev(c.dr)
    scalar_kernel = c.kernel.replace("traj_ladder_kernel", "traj_kernel")
    assert np.array_equal(h["x"], h["x_hist"][-1])
    try:
        dyn.use_temperature = True
        for m in range(R * M):
            lab = _labels_before(c, h, m // M)
            x_in = x0 if m == 0 else o["x_hist"][m - 1]
            for k, Tk in enumerate(c.temps):
                dyn.temperature = float(np.float32(Tk))
                s = dyn.run(x_in, v[m], 0, T, direction=None if dr is None else dr[m], u=u[m], want=("p", "x_next"))
                assert _ffi.last_kernel() == scalar_kernel, (name, _ffi.last_kernel())
                rows = np.nonzero(lab == k)[0]
                assert len(rows) == c.nl
                sp, sx = to_np(s["p"]), to_np(s["x_next"])
                assert np.array_equal(h["p"][m][rows], sp[rows]), \
                    (name, "p", m, k, rows[np.nonzero(h["p"][m][rows] != sp[rows])[0]])
                assert np.array_equal(h["x_hist"][m][rows], sx[rows]), \
                    (name, "x", m, k, rows[np.nonzero(np.any(h["x_hist"][m][rows] != sx[rows], axis=1))[0]])
    finally:
        dyn.use_temperature, dyn.temperature = False, 1.0


@pytest.mark.parametrize("name", list(LC.CASES))
def test_swap_decisions_counters_and_round_trips_match_the_reference(name):
    c, dyn, pt, o, h = _get(name)

    def U_of(xs):
        return to_np(dyn.energy(xs)).astype(np.float64)            # T = 1 (use_temperature off)
    compared, acc, att, trips = ref.replay(pt, o, o["x_hist"], U_of, c.temps, R, M, c.swap_u, 0, c.labels0, tol=c.tol)
    print("%s: %s, %d of %d ladder-rounds left out by the near-tie rule (%.1f %%), accepted %s of %s"
          % (name, h["kernel"], R * c.nl - compared, R * c.nl, 100.0 * (R * c.nl - compared) / (R * c.nl), acc, att))
    assert compared >= 0.95 * R * c.nl
    assert np.array_equal(att, h["swaps_attempted"])
    want_att = [c.nl * sum(1 for j in range(R) if j % 2 == k % 2) for k in range(c.K - 1)]
    assert h["swaps_attempted"].tolist() == want_att
    assert np.abs(acc - h["swaps_accepted"]).sum() <= R * c.nl - compared
    assert np.array_equal(trips, h["round_trips"])
    assert np.array_equal(to_np(pt.rung_of_row).astype(np.int64), h["rung_hist"][-1])
    assert 0 < int(acc.sum()) < int(att.sum())
    for j in range(R):                                              # every round leaves a permutation of the rungs in every ladder
        assert np.array_equal(np.sort(h["rung_hist"][j].reshape(c.nl, c.K), axis=1), c.labels0)
    if c.K == 2:                                                    # the odd rounds of K = 2 propose nothing
        for j in range(1, R, 2):
            assert np.array_equal(h["rung_hist"][j], h["rung_hist"][j - 1]), j
        assert int(h["swaps_attempted"][0]) == c.nl * ((R + 1) // 2)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_cold_hist_is_the_label_0_row_of_x_hist_bit_for_bit(name):
    c, dyn, pt, o, h = _get(name)
    assert h["cold_hist"].shape == (R * M, c.nl, c.d)
    for m in range(R * M):
        j = m // M
        lab = h["rung_hist"][j] if (m + 1) % M == 0 else _labels_before(c, h, j)
        cold = lab.reshape(c.nl, c.K) == 0
        assert np.all(cold.sum(axis=1) == 1)
        rows = np.arange(c.nl) * c.K + np.argmax(cold, axis=1)
        assert np.array_equal(h["cold_hist"][m], h["x_hist"][m][rows]), (name, m)


# Measured float32-to-float64 oracle distance of that proposal, max(|p32 - p64|, rel |Lx32 - Lx64|) over the rungs (printed by the
# test): g20_w4 3.5e-6, g20_h14 1.8e-6, gmm20 3.6e-6, lr12_w4 3.5e-6 -- 3 x each lies under the project's 1e-4, which is
# therefore the gate.
@pytest.mark.parametrize("name", LC.ORACLE_CASES)
def test_the_first_proposal_after_a_sweep_matches_the_oracle_at_the_new_temperatures(name):
    """Tolerance: the larger of the project's 1e-4 and 3 x (`helpers.assert_bracket`'s factor) the distance between the float32
    and the float64 oracle on the same inputs -- measured between the two oracles, never against the kernel."""
    c, dyn, pt, o, h = _get(name)
    m, lab = M, h["rung_hist"][0]
    assert np.any(lab != c.labels0.reshape(-1))                     # some row starts this proposal at a new temperature
    x_in = h["x_hist"][M - 1]
    worst = 0.0
    for k, Tk in enumerate(c.temps):
        rows = np.nonzero(lab == k)[0]
        a32 = (x_in[rows], c.v[m][rows], c.dr[m][rows], c.u[m][rows])
        od32, od64 = c.oracle_dynamics(np.float32, Tk), c.oracle_dynamics(np.float64, Tk)
        L32, _, p32, _ = O.propose(a32[0], od32, a32[1], a32[1], a32[2], a32[3], both_directions=False)
        L64, _, p64, _ = O.propose(a32[0].astype(np.float64), od64, a32[1].astype(np.float64), a32[1].astype(np.float64),
                                   a32[2], a32[3].astype(np.float64), both_directions=False)
        dist = max(helpers.abs_err(p32, p64), helpers.rel_err(L32, L64))
        worst = max(worst, dist)
        tol = max(1e-4, 3.0 * dist)
        ep = helpers.abs_err(h["p"][m][rows], p32)
        print("%s rung %d: float32-to-float64 oracle distance %.2e, gate %.2e, kernel |p - p32| %.2e" % (name, k, dist, tol, ep))
        assert ep < tol, (name, k, ep, tol)
        helpers.check_x_next(h["x_hist"][m][rows], x_in[rows], L32, p32, a32[3], tol)
    print("%s: float32-to-float64 oracle distance of the post-swap proposal %.2e" % (name, worst))


# ---- outside the table: g20_w4's target and nets, K = 8 unless said ---------------------------------------------------------
def _base():
    c = LC.case("g20_w4")
    return c, c.hip_dynamics(), LC.case("k8").temps


def test_chain_offset_a_multiple_of_k_but_not_of_16():
    """40 rows in one launch = 24 rows at offset 0 + 16 rows at chain_offset = 24: row 24 sits in lane 8 of tile 1 in one launch
    and in lane 0 of tile 0 in the other, and its ladder's swap stream is keyed by (chain_offset + chain) / K."""
    c, dyn, temps = _base()
    K, Rr, Mm = 8, 6, 2
    x0 = to_dev(c.x0)
    full = ParallelTempering(dyn, temps, 5, seed=9)
    of = full.run(x0, Rr, Mm)
    pa = ParallelTempering(dyn, temps, 3, seed=9)
    pb = ParallelTempering(dyn, temps, 2, seed=9, chain_offset=3 * K)
    oa, ob = pa.run(x0[:3 * K], Rr, Mm), pb.run(x0[3 * K:], Rr, Mm)
    torch.cuda.synchronize()
    assert _ffi.last_kernel() == c.kernel
    assert torch.equal(torch.cat([oa["x"], ob["x"]]), of["x"]) and torch.equal(torch.cat([oa["p"], ob["p"]], 1), of["p"])
    assert torch.equal(torch.cat([pa.rung_of_row, pb.rung_of_row]), full.rung_of_row)
    assert torch.equal(torch.cat([pa.trip_state, pb.trip_state]), full.trip_state)
    assert torch.equal(oa["swaps_attempted"] + ob["swaps_attempted"], of["swaps_attempted"])
    assert torch.equal(oa["swaps_accepted"] + ob["swaps_accepted"], of["swaps_accepted"])
    assert torch.equal(torch.cat([oa["round_trips"], ob["round_trips"]]), of["round_trips"])
    assert 0 < int(of["swaps_accepted"].sum()) < int(of["swaps_attempted"].sum())


def test_resume_through_state_dict_on_a_fresh_ladder():
    c, dyn, _ = _base()
    temps, nl, Rr, Mm = [1.0, 1.2, 1.5, 2.0], 10, 10, 1
    x0 = to_dev(c.x0)
    one = ParallelTempering(dyn, temps, nl, seed=31)
    o1 = one.run(x0, Rr, Mm)
    first = ParallelTempering(dyn, temps, nl, seed=31)
    oa = first.run(x0, Rr // 2, Mm)
    sd = first.state_dict()
    assert int(sd["trip_state"].abs().sum()) > 0                    # rows half-way through a round trip at the cut ...
    assert not torch.equal(sd["rung_of_row"], (torch.arange(4 * nl) % 4).to(torch.int8))      # ... and away from their first rungs
    second = ParallelTempering(dyn, temps, nl, seed=0)               # (seed, counters, labels: all from the state)
    second.load_state_dict(sd)
    ob = second.run(oa["x"], Rr - Rr // 2, Mm)
    torch.cuda.synchronize()
    assert torch.equal(ob["x"], o1["x"]) and torch.equal(ob["p"], o1["p"][(Rr // 2) * Mm:])
    assert torch.equal(oa["p"], o1["p"][:(Rr // 2) * Mm])
    assert torch.equal(second.rung_of_row, one.rung_of_row) and torch.equal(second.trip_state, one.trip_state)
    assert int(oa["round_trips"].sum() + ob["round_trips"].sum()) == int(o1["round_trips"].sum())
    assert torch.equal(oa["swaps_accepted"] + ob["swaps_accepted"], o1["swaps_accepted"])
    assert second.round == one.round == Rr and second.proposal == one.proposal == Rr * Mm


def test_nothing_is_written_past_row_n():
    """The half-live last tile: labels, round-trip states and x live in buffers 16 rows longer than N (so a store that misses
    its `live` guard lands in allocated memory and shows)."""
    c, dyn, temps = _base()
    K, nl, N, d = 8, 5, 40, c.d
    kw = dict(record_cold=True, record_rungs=True, record_states=True)
    exact = ParallelTempering(dyn, temps, nl, seed=5)
    oe = exact.run(to_dev(c.x0), R, M, **kw)
    padded = ParallelTempering(dyn, temps, nl, seed=5)
    rung_buf = torch.full((N + 16,), 77, dtype=torch.int8, device="cuda")
    trip_buf = torch.full((N + 16,), 77, dtype=torch.int8, device="cuda")
    rung_buf[:N] = padded.rung_of_row
    trip_buf[:N] = padded.trip_state
    padded.rung_of_row, padded.trip_state = rung_buf[:N], trip_buf[:N]
    x_buf = torch.full((N + 16, d), float("nan"), dtype=torch.float32, device="cuda")
    x_buf[:N] = to_dev(c.x0)
    op = padded.run(x_buf[:N], R, M, **kw)
    torch.cuda.synchronize()
    assert torch.all(rung_buf[N:] == 77) and torch.all(trip_buf[N:] == 77)
    assert bool(torch.isnan(x_buf[N:]).all()) and torch.equal(x_buf[:N], to_dev(c.x0))
    for k in ("x", "p", "x_hist", "cold_hist", "rung_hist", "swaps_accepted", "swaps_attempted", "round_trips"):
        assert torch.equal(op[k], oe[k]), k
    assert torch.equal(padded.rung_of_row, exact.rung_of_row) and torch.equal(padded.trip_state, exact.trip_state)
    assert bool(torch.isfinite(op["x"]).all()) and int(oe["swaps_accepted"].sum()) > 0


def test_a_non_finite_row_rejects_its_swaps_and_stays_in_its_lane():
    """traj_body.inc at the swap rule: "a NaN on either side rejects"."""
    c, dyn, temps = _base()
    K, nl, N = 8, 5, 40
    bad = 19                                                        # ladder 2: lanes 0 ... 7 of tile 1, next to ladder 3
    kw = dict(record_rungs=True, record_states=True)
    clean = ParallelTempering(dyn, temps, nl, seed=5)
    oc = clean.run(to_dev(c.x0), R, M, **kw)
    x0 = c.x0.copy()
    x0[bad] = np.nan
    pois = ParallelTempering(dyn, temps, nl, seed=5)
    op = pois.run(to_dev(x0), R, M, **kw)
    torch.cuda.synchronize()
    rh = to_np(op["rung_hist"]).astype(np.int64)
    assert np.all(rh[:, bad] == bad % K)                             # its label never changes
    want_att = [nl * sum(1 for j in range(R) if j % 2 == k % 2) for k in range(K - 1)]
    assert to_np(op["swaps_attempted"]).tolist() == want_att
    others = np.array([r for r in range(N) if r // K != bad // K])
    assert len(others) == N - K
    assert np.array_equal(to_np(op["x"])[others], to_np(oc["x"])[others])
    assert np.array_equal(to_np(op["x_hist"])[:, others], to_np(oc["x_hist"])[:, others])
    assert np.array_equal(to_np(op["p"])[:, others], to_np(oc["p"])[:, others])
    assert np.array_equal(rh[:, others], to_np(oc["rung_hist"]).astype(np.int64)[:, others])
    assert np.array_equal(to_np(pois.rung_of_row)[others], to_np(clean.rung_of_row)[others])
    mates = np.array([r for r in range(N) if r // K == bad // K and r != bad])
    assert np.all(np.isfinite(to_np(op["x_hist"])[:, mates])) and np.all(np.isfinite(to_np(op["p"])[:, mates]))
    assert np.all(np.isnan(to_np(op["x"])[bad]))
