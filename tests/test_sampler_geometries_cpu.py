"""The inputs of tests/sampler_geometry_cases.py exercise what the GPU tests are about -- checked with the numpy oracle alone, no GPU.

A case whose proposals are all accepted never runs the reject-and-restore path; one whose trajectories blow up compares
infinities; one with accept probabilities on top of their uniforms flips decisions on float32 noise.  A case that misses a
condition gets another seed or step size in the table, never a wider condition here.
"""
import numpy as np
import pytest

from tests import sampler_geometry_cases as C


def test_the_table_covers_every_compiled_form():
    """All 16 four-tile forms and the two eight-tile forms of the tile kernel, all 16 base forms of the lane kernel and the
    resident forms the planner picks at d <= 2, H <= 10; the boundary widths and hidden sizes each appear."""
    names = {c["kernel"] for c in C.CASES.values()}
    for ek in (1, 4):
        for dt in (3, 4):
            for kh in (3, 4):
                for half in ("true", "false"):
                    assert "traj_tile_kernel<%d, %d, %d, 4, %s>" % (ek, dt, kh, half) in names
    assert {"traj_tile_kernel<1, 3, 3, 8, false>", "traj_tile_kernel<4, 4, 4, 8, false>"} <= names
    for ek in (1, 2, 3, 4):
        for dp in (2, 4):
            for hpr in (5, 8):
                assert "traj_lane_kernel<%d, %d, %d>" % (ek, dp, hpr) in names
        assert "traj_lane_kernel<%d, 2, 5, %d>" % (ek, 2 if ek == 1 else 1) in names
    tiles = [c for c in C.CASES.values() if c["variant"] == 16]
    assert {33, 35, 48, 49, 51, 64} <= {c["d"] for c in tiles} and {11, 12} <= {c["H"] for c in tiles}
    for c in C.CASES.values():           # the names follow the planner's arithmetic (plan_trajectory, l2hmc_abi.hip)
        if c["kernel"].startswith(C.TILE):
            dt, kh = (c["d"] + 15) // 16, (c["H"] + 4) // 4
            half = "true" if c["d"] - 16 * (dt - 1) <= 2 else "false"
            assert c["kernel"].startswith("%s<%d, %d, %d, " % (C.TILE, {"gauss_diag": 1, "roughwell_easy": 4}[c["kind"]], dt, kh))
            assert c["kernel"].endswith(", %s>" % half), c
        if c["kernel"].startswith(C.LANE):
            assert ", %d, %d" % (2 if c["d"] <= 2 else 4, 5 if c["H"] <= 10 else 8) in c["kernel"], c


@pytest.mark.parametrize("name", C.SMALL)
def test_case_inputs_meet_their_conditions(name):
    c = C.case(name)
    acc, near, e_x, e_p = c.check_inputs()
    print("%s: accepted %.2f  near ties %d  float32 oracle vs float64: Lx %.1e  p %.1e" % (name, acc, near, e_x, e_p))
    assert c.x.shape == (c.N, c.d) and c.v.shape == (C.M, c.N, c.d) and c.dr.shape == c.u.shape == (C.M, c.N)
    assert set(np.unique(c.dr[0])) == {0, 1}                                # both directions among the chains
    assert 0 < C.SPLIT < c.N and C.SPLIT % 16 != 0
