"""Every compiled form of the one-wave-per-tile kernel (csrc/traj_tile.hpp) and the one-chain-per-lane kernel (csrc/traj_lane.hpp)
against the float64 numpy oracle, at the launches of tests/sampler_geometry_cases.py.

The forms differ where kernels go wrong: the live width of the padded last dimension slice (klast, the HALF arithmetic), `t < NT`
against `t < DT` in the staging loops, the KH loops of the hidden layer, waves that leave a workgroup after its prologue's
barriers, Rough Well's masked U over padded dimensions, the lane layout's zero-padded rows and pairs.  Per case:

  a. `_ffi.last_kernel()` names the form the table says;
  b. one direction-mixed proposal with an MH step: Lx and p inside the float64 bracket of test_full_size_configs_against_oracle
     (per chain at most 3 x the float32 oracle's own worst error + the suite's tolerance), the selected state, the log-Jacobian;
  c. M = 3 proposals in one launch == three single launches bit for bit, and == the oracle loop away from accept ties;
  d. the in-kernel Philox draws == the same draws injected;
  e. the chains split at chain 24 into two launches == the one launch bit for bit (every chain changes its lane and tile);
  f. partial trajectories (step_begin = 2) in both directions against the oracle's composition of single steps.

The cases beyond 100 chains (eight tiles per workgroup, the planner's chain-count thresholds) are held to the oracle on their first
192 and last 40 chains and, on every chain, to the same inputs run in two halves under the forced family.

Measured on an MI355X under (b), the largest ratio of the HIP error to the float32 oracle's error against float64 (a record for
later work; the gate is the bracket above): tile kernel 1.41 in Lx (t_g35_h11: 4.3e-7 against 3.0e-7) and 1.56 in p (t_g49_h11:
8.2e-6 against 5.3e-6); lane kernel 1.33 in Lx (l_gd_d4_h15: 5.7e-7 against 4.3e-7) and 3.50 in p (l_gmm3_d2_h11: 3.9e-6 against
1.1e-6).  Every test (b) prints its figures.
"""
import numpy as np
import pytest

from oracle import l2hmc_oracle as O
from tests import helpers
from tests import sampler_geometry_cases as C
from tests.helpers import abs_err, check_x_next, rel_err, to_dev, to_np

pytestmark = pytest.mark.gpu

STEP_TOL, TRAJ_TOL, P_TOL = 3e-5, 1e-4, 1e-4
LOOPS = C.SMALL + list(C.TPW8)              # (c), (d): every form; the threshold cases launch forms the small cases already loop
HALVES = sorted(n for n in C.BIG if C.CASES[n].get("forced"))

_runs = {}


def _case(name, monkeypatch):
    """The case, with L2HMC_LANE_RES as its row says for the launches of this test (the planner reads it per call)."""
    import torch
    c = C.case(name, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    if c.lane_res is None:
        monkeypatch.delenv("L2HMC_LANE_RES", raising=False)
    else:
        monkeypatch.setenv("L2HMC_LANE_RES", c.lane_res)
    return c


def _propose(c, dyn, lo=0, hi=None, m=0, x=None):
    """Banked proposal m on chains [lo, hi) (from state x): (Lx, p, x_next, kernel name)."""
    from l2hmc_amd import _ffi, propose
    hi = c.N if hi is None else hi
    xs = to_dev(c.x[lo:hi]) if x is None else x
    Lx, _, px, outs = propose(xs, dyn, do_mh_step=True, direction=to_dev(c.dr[m, lo:hi]), v=to_dev(c.v[m, lo:hi]),
                              u=to_dev(c.u[m, lo:hi]))
    return Lx, px, outs[0], _ffi.last_kernel()


def _first(c):
    """The case's first banked proposal on all chains, launched once and shared by (a), (b), (e) and the halves."""
    if c.name not in _runs:
        _runs[c.name] = _propose(c, c.hip_dynamics())
    return _runs[c.name]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_kernel_name(name, monkeypatch):
    c = _case(name, monkeypatch)
    assert _first(c)[3] == c.kernel, (name, _first(c)[3])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_first_proposal_against_float64(name, monkeypatch):
    c = _case(name, monkeypatch)
    Lx, px, xn, _ = _first(c)
    i = c.idx
    Lx, px, xn = to_np(Lx)[i], to_np(px)[i], to_np(xn)[i]
    tLx, tp, _ = c.first_proposal(np.float64)
    rLx, rp, _ = c.first_proposal(np.float32)
    fin = np.all(np.isfinite(tLx), axis=1) & (np.abs(tLx).max(axis=1) < 1e4)
    assert fin.mean() > 0.95
    scale = np.maximum(1.0, np.abs(tLx).max(axis=1))
    e_hip = (np.abs(Lx - tLx).max(axis=1) / scale)[fin]
    e_o32 = (np.abs(rLx - tLx).max(axis=1) / scale)[fin]
    ep_hip, ep_o32 = np.abs(px - tp)[fin], np.abs(rp - tp)[fin]
    print("GEOMETRY %s %s: Lx err vs float64 hip %.2e oracle32 %.2e ratio %.2f | p hip %.2e oracle32 %.2e ratio %.2f"
          % (name, c.kernel, e_hip.max(), e_o32.max(), e_hip.max() / e_o32.max(), ep_hip.max(), ep_o32.max(),
             ep_hip.max() / ep_o32.max()))
    assert np.quantile(e_hip, 0.99) < TRAJ_TOL
    assert e_hip.max() <= 3 * e_o32.max() + TRAJ_TOL
    assert np.quantile(ep_hip, 0.99) < P_TOL
    assert ep_hip.max() <= 3 * ep_o32.max() + P_TOL
    check_x_next(xn, c.x[i], tLx, tp, c.u[0][i], P_TOL)
    # the log-Jacobian of the all-forward trajectory (on every chain: the same launch shape, so the same kernel)
    from l2hmc_amd import _ffi
    X, V, lj = c.hip_dynamics().forward(to_dev(c.x), init_v=to_dev(c.v[0]), log_jac=True)
    assert _ffi.last_kernel() == c.kernel
    with np.errstate(all="ignore"):
        tX, tV, tlj = c.oracle_dynamics(np.float64).forward(c.x[i].astype(np.float64), c.v[0][i].astype(np.float64), log_jac=True)
    assert rel_err(to_np(lj)[i], tlj) < TRAJ_TOL
    assert rel_err(to_np(X)[i], tX) < TRAJ_TOL and rel_err(to_np(V)[i], tV) < TRAJ_TOL


@pytest.mark.parametrize("name", LOOPS)
def test_loop_equals_single_launches_and_the_oracle_loop(name, monkeypatch):
    import torch
    from l2hmc_amd import _ffi, sample_chain
    c = _case(name, monkeypatch)
    dyn = c.hip_dynamics()
    xf, p, xh = sample_chain(to_dev(c.x), dyn, C.M, direction=to_dev(c.dr), v=to_dev(c.v), u=to_dev(c.u), record=True)
    assert _ffi.last_kernel() == c.kernel
    xs = to_dev(c.x)
    for m in range(C.M):
        _, pm, xn, kern = _propose(c, dyn, m=m, x=xs)
        assert kern == c.kernel
        assert torch.equal(pm, p[m]) and torch.equal(xn, xh[m]), (name, m)
        xs = xn
    assert torch.equal(xs, xf)
    acc = to_np(p) >= c.u
    assert 0.05 < acc.mean() < 0.95, acc.mean()              # both the accept and the reject-and-restore path ran
    i, od = c.idx, c.oracle_dynamics()
    xo, ok = c.x[i], np.ones(len(i), dtype=bool)
    with np.errstate(all="ignore"):
        for m in range(C.M):
            _, _, po, xo = O.propose(xo, od, c.v[m][i], c.v[m][i], c.dr[m][i], c.u[m][i], both_directions=False)
            ok &= np.abs(po - c.u[m][i]) > 1e-3
            assert abs_err(to_np(p[m])[i][ok], po[ok]) < 5 * P_TOL, (name, m)
    assert ok.mean() > 0.7 and rel_err(to_np(xf)[i][ok], xo[ok]) < 5 * TRAJ_TOL


@pytest.mark.parametrize("name", LOOPS)
def test_in_kernel_philox_equals_injected_draws(name, monkeypatch):
    import torch
    from l2hmc_amd import _ffi, sample_chain
    from l2hmc_amd.sampler import philox_draws
    c = _case(name, monkeypatch)
    dyn = c.hip_dynamics()
    xr, pr, _ = sample_chain(to_dev(c.x), dyn, C.M, seed=99)
    assert _ffi.last_kernel() == c.kernel
    v, dr, u = philox_draws(99, c.N, c.d, C.M)
    xi, pi, _ = sample_chain(to_dev(c.x), dyn, C.M, v=v, u=u, direction=dr)
    assert _ffi.last_kernel() == c.kernel
    assert torch.equal(pr, pi) and torch.equal(xr, xi)


@pytest.mark.parametrize("name", C.SMALL)
def test_chains_never_interact(name, monkeypatch):
    import torch
    c = _case(name, monkeypatch)
    Lx, px, xn, _ = _first(c)
    dyn = c.hip_dynamics()
    for lo, hi in ((0, C.SPLIT), (C.SPLIT, c.N)):
        Lh, ph, xh, kern = _propose(c, dyn, lo, hi)
        assert kern == c.kernel
        assert torch.equal(Lh, Lx[lo:hi]) and torch.equal(ph, px[lo:hi]) and torch.equal(xh, xn[lo:hi]), (name, lo)


@pytest.mark.parametrize("name", HALVES)
def test_threshold_launch_equals_two_forced_halves(name, monkeypatch):
    """The chains of an automatic (`variant = 0`) launch at a threshold of the planner, run as two halves under the forced family --
    below the eight-tile threshold the four-tile form of the same kernel, for the lane kernel the same form: bit for bit."""
    import torch
    c = _case(name, monkeypatch)
    Lx, px, xn, kern = _first(c)
    assert kern == c.kernel
    forced = c.hip_dynamics(variant=c.forced)
    h = c.N // 2
    for lo, hi in ((0, h), (h, c.N)):
        Lh, ph, xh, kern = _propose(c, forced, lo, hi)
        assert kern == c.kernel.replace(", 8, ", ", 4, "), (name, kern)
        assert torch.equal(Lh, Lx[lo:hi]) and torch.equal(ph, px[lo:hi]) and torch.equal(xh, xn[lo:hi]), (name, lo)


@pytest.mark.parametrize("name", C.TPW8)
def test_eight_tile_threshold_in_the_schedule_length(name, monkeypatch):
    """The schedule length the table records is where the planner's LDS rule turns: one step shorter still launches four tiles per
    workgroup (`t_below`); where every length launches eight, T = 1 does (`t_floor`)."""
    from l2hmc_amd import _ffi, propose
    c = _case(name, monkeypatch)
    x, v, dr = to_dev(c.x), to_dev(c.v[0]), to_dev(c.dr[0])
    if c.t_below is not None:
        propose(x, c.hip_dynamics(T=c.t_below), direction=dr, v=v)
        assert _ffi.last_kernel() == c.kernel.replace(", 8, ", ", 4, ")
    if c.t_floor is not None:
        propose(x, c.hip_dynamics(T=c.t_floor), direction=dr, v=v)
        assert _ffi.last_kernel() == c.kernel


@pytest.mark.parametrize("n_steps", [2, 1])
@pytest.mark.parametrize("fwd", [1, 0])
@pytest.mark.parametrize("name", C.PARTIAL)
def test_partial_trajectories(name, fwd, n_steps, monkeypatch):
    """Leapfrog iterations [2, 2 + n_steps) of the T = 5 schedule: forward they are the schedule rows 2, 3; backward, iteration i is
    the step at schedule row T - 1 - i (include/l2hmc.h) -- rows 2, 1."""
    from l2hmc_amd import _ffi
    c = _case(name, monkeypatch)
    begin = 2
    o = c.hip_dynamics().run(to_dev(c.x), to_dev(c.v[0]), begin, n_steps, direction_all=fwd)
    assert _ffi.last_kernel() == c.kernel
    od = c.oracle_dynamics(np.float64)
    X, V, lj = c.x.astype(np.float64), c.v[0].astype(np.float64), np.zeros(c.N)
    for it in range(begin, begin + n_steps):
        if fwd:
            X, V, l1 = od.forward_step(X, V, np.float64(it))
        else:
            X, V, l1 = od.backward_step(X, V, np.float64(c.T - 1 - it))
        lj = lj + l1
    tol = STEP_TOL * n_steps
    assert rel_err(to_np(o["x"]), X) < tol and rel_err(to_np(o["v"]), V) < tol and rel_err(to_np(o["logjac"]), lj) < tol


def test_forced_families_refuse_what_they_do_not_serve():
    from l2hmc_amd import propose

    def launch(g, variant):
        N = g["x"].shape[0]
        propose(to_dev(g["x"]), helpers.hip_dynamics(g, variant), direction=to_dev(np.ones(N, np.uint8)), v=to_dev(g["v"]))
    for d, variant in ((32, 16), (65, 16), (40, 216)):       # two and five dimension slices; f32 asked of an f16x2-only kernel
        with pytest.raises(RuntimeError, match="variant 16"):
            launch(helpers.synthetic_case("gauss_diag", d, H=10, T=5, N=40, seed=d), variant)
    with pytest.raises(RuntimeError, match="variant 32"):
        launch(helpers.synthetic_case("gauss_diag", 5, H=10, T=5, N=40, seed=5), 32)
    g = helpers.synthetic_case("gauss_diag", 3, H=10, T=5, N=40, seed=3)
    for k in ("energy.mu", "energy.i_sigma"):
        del g[k]
    g.update({"energy.kind": "funnel", "energy.sigma": np.float32(2.0)})
    with pytest.raises(RuntimeError, match="variant 32"):
        launch(g, 32)
