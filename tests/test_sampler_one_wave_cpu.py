"""CPU: the resources of the sampler kernel's one-workgroup-per-CU body (traj_fast_cc_kernel, csrc/traj_f16_one_wave.hip), read
from the listing the Makefile's own compile of that unit writes (its flags: -mllvm -amdgpu-mfma-vgpr-form).

What the body is for is a step loop that is NOT longer than the two-wave kernel's: with AGPRs in its budget and without the flag the
compiler takes the AGPR form of every MFMA result and copies each out again, 60 VALU instructions more per leapfrog step.  So:
no scratch, no AGPR copy inside the step loop (they belong at the proposal boundary), and a step loop of at most the two-wave
kernel's static instruction count from the same build.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "l2hmc_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def listings():
    """(one-wave unit's listing, two-wave unit's listing): made by the Makefile's rule, a no-op on a built tree."""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run(["make", "-C", CSRC, "-j2", "ARCH=gfx950", "traj_f16_one_wave.o", "traj_f16_ek1.o"], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "build", "asm", "traj_f16_one_wave.s"), os.path.join(CSRC, "build", "asm", "traj_f16_ek1.s")


def _step_loop(path, kernel):
    """the instructions (mnemonics) of the kernel's innermost loop: the leapfrog step"""
    import isa_hist
    L = isa_hist.kernel_lines(path, kernel)
    i0, i1 = isa_hist.innermost_region(L)
    ops = []
    for ln in L[i0:i1]:
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        if re.match(r"^[a-z]", s.split()[0]):
            ops.append(s.split()[0])
    return ops


def _descriptor(path, kernel):
    txt = open(path).read()
    m = re.search(r"\.amdhsa_kernel \S*" + kernel + r"\S*\n(.*?)\.end_amdhsa_kernel", txt, re.S)
    assert m, kernel
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\n", m.group(1))}


@pytest.mark.parametrize("KH", [3, 4])
def test_step_loop_and_registers_of_the_one_wave_body(KH, listings):
    one, two = listings
    new = "traj_fast_cc_kernelILi1ELi1ELi4ELi%dELi1ELi1E" % KH
    old = "traj_fast_kernelILi1ELi1ELi4ELi%dELi1E" % KH
    d = _descriptor(one, new)
    assert d["private_segment_fixed_size"] == 0, d
    assert d["next_free_vgpr"] <= 512
    loop_new, loop_old = _step_loop(one, "^_ZN5l2hmc\\d+" + new), _step_loop(two, "^_ZN5l2hmc\\d+" + old)
    assert sum(op.startswith("v_mfma") for op in loop_new) == sum(op.startswith("v_mfma") for op in loop_old) == 40     # (it IS the step)
    assert not [op for op in loop_new if op.startswith("v_accvgpr_read") or op.startswith("v_accvgpr_write")]
    assert not [op for op in loop_new if op.startswith("scratch_") or op.startswith("buffer_")]
    assert len(loop_new) <= len(loop_old), (len(loop_new), len(loop_old))
