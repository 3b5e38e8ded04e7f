"""Taking launch- and proposal-invariant work out of the sampler kernel (traj_fast.hpp: no look-ahead tail on a proposal's last
step, no arithmetic on the dead hidden row, a body compiled for the common launch, a prologue whose loads are in flight
together) changes NO result bit.

Two layers:
  * tests/golden/sampler_boundary/parent.npz holds what the commit BEFORE that work computed for the launches of
    tests/sampler_boundary_cases.py (recorded on an MI355X with that commit's library); every output must be equal bit for bit
    (a sub-directory of tests/golden: the top level is globbed for trajectory goldens by tests/helpers.py);
  * M proposals in one launch equal M chained single-proposal launches: the first carries state in registers across the
    proposal boundary, the second runs the prologue every time.
"""
import os

import numpy as np
import pytest

from tests import helpers
from tests import sampler_boundary_cases as C

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(helpers.GOLDEN, "sampler_boundary", "parent.npz")


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def runs():
    """Every case launched once, shared by the tests below."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = C.launch(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_bits_of_the_parent(name, parent, runs):
    o, kern = runs(name)
    assert kern == str(parent[name + ".kernel"])
    if name in C.KERNELS:
        assert kern == C.KERNELS[name]
    keys = sorted(k.split(".", 1)[1] for k in parent.files if k.startswith(name + ".") and not k.endswith(".kernel"))
    assert keys == sorted(o), (keys, sorted(o))
    assert "x_next" in keys and "p" in keys
    for k in keys:
        assert np.array_equal(o[k], parent[name + "." + k], equal_nan=True), (name, k)


def test_poisoned_chain_is_loud(runs):
    """One chain started beyond L2HMC_F16_STATE_MAX: accept probability 0 in every proposal, so the chain stays where it started;
    the other chains of its tile are untouched by it (finite)."""
    o, _ = runs("poison_m3")
    g, _ = C._case("icg50_poison")
    assert np.all(o["p"][:, 5] == 0.0)
    assert np.array_equal(o["x_next"][5], g["x"][5])
    keep = np.arange(C.N) != 5
    assert np.all(np.isfinite(o["x_next"][keep])) and np.all(np.isfinite(o["p"][:, keep]))


@pytest.mark.parametrize("name", ["rng_s10_m3", "rng_s1_m3", "rng_s0_m2", "rng_b3_s4_m3", "bank_mixed", "h14_m3", "d20_m3", "d16_m3",
                                  "roughwell8_m3", "v204_m3"])
def test_one_launch_equals_chained_launches(name, runs):
    o, _ = runs(name)
    M = C.CASES[name][3]
    x = None
    for m in range(M):
        om, _ = C.launch(name, x=x, M=1, proposal0=m, m0=m)
        x = om["x_next"]
        assert np.array_equal(om["p"], o["p"][m], equal_nan=True), (name, m)
        if "x_hist" in o:
            assert np.array_equal(om["x_next"], o["x_hist"][m], equal_nan=True), (name, m)
            assert np.array_equal(om["logjac"], o["logjac"][m], equal_nan=True), (name, m)
    assert np.array_equal(x, o["x_next"], equal_nan=True), name
    if "x" in o:          # x_out / v_out are the last proposal's end point
        assert np.array_equal(om["x"], o["x"], equal_nan=True) and np.array_equal(om["v"], o["v"], equal_nan=True)
