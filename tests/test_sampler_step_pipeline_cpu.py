"""CPU: what the step-loop items of the sampler kernel's one-workgroup-per-CU body (traj_fast_cc_kernel, L2HMC_ONE_WAVE_ITEMS in
csrc/traj_fast.hpp; profiles/sampler_step_pipeline.txt) claim, read from the listing the Makefile's own compile of the unit writes,
and the host's LDS plan for that body (l2hmc_sampler_lds_plan: the planner's own function, no GPU).

The parent's step loop had 464 instructions at KH = 3 and 483 at KH = 4 (tools/isa_hist.py); the rule for this kernel is a step
loop no longer than that, no scratch and no AGPR copy in it.  The static exchange buffers (bit 1) and the per-wave schedule
records behind one pointer (bit 2) remove the loop's address arithmetic: what is left is the record pointer's advance and the
compiler's re-forming of the ds_write address (two v_add_u32 where the parent has seven and a v_lshl_add_u32), one s_add_i32 (the
loop counter) and no shift or xor; the complement of the mask is read, not computed, so the loop has one ds_read_b128 more (16)
and its only v_sub_f32 are the four of grad U = P (x - mu).  The look-ahead split (bit 3) and the log-det adds under the reads
(bit 5) move instructions, they add none: the arithmetic mnemonics keep the parent's counts.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "l2hmc_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

PARENT_LOOP = {3: 464, 4: 483}
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def listing():
    """the one-wave unit's listing: made by the Makefile's rule, a no-op on a built tree"""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run(["make", "-C", CSRC, "-j2", "ARCH=gfx950", "traj_f16_one_wave.o"], check=True, env=env, stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "build", "asm", "traj_f16_one_wave.s")


def _step_loop(path, kernel):
    """the instructions (mnemonics, without the encoding suffix) of the kernel's innermost loop: the leapfrog step"""
    import isa_hist
    L = isa_hist.kernel_lines(path, kernel)
    i0, i1 = isa_hist.innermost_region(L)
    ops = []
    for ln in L[i0:i1]:
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        if re.match(r"^[a-z]", s.split()[0]):
            ops.append(re.sub(r"_e(32|64)$", "", s.split()[0]))
    return ops


def _descriptor(path, kernel):
    txt = open(path).read()
    m = re.search(r"\.amdhsa_kernel \S*" + kernel + r"\S*\n(.*?)\.end_amdhsa_kernel", txt, re.S)
    assert m, kernel
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\n", m.group(1))}


def _items():
    m = re.search(r"#define L2HMC_ONE_WAVE_ITEMS (\d+)", open(os.path.join(CSRC, "traj_fast.hpp")).read())
    return int(m.group(1))


def test_the_kept_items():
    # tails once per launch | static exchange buffers | per-wave records | look-ahead split | log-det adds under the reads
    assert _items() == 1 + 2 + 4 + 8 + 32


@pytest.mark.parametrize("KH", [3, 4])
def test_step_loop_of_the_kept_build(KH, listing):
    name = "traj_fast_cc_kernelILi1ELi1ELi4ELi%dELi1ELi1E" % KH
    d = _descriptor(listing, name)
    assert d["private_segment_fixed_size"] == 0, d
    assert d["next_free_vgpr"] <= 512
    loop = _step_loop(listing, "^_ZN5l2hmc\\d+" + name)
    n = lambda op: sum(o == op for o in loop)
    assert sum(o.startswith("v_mfma") for o in loop) == 40          # (it IS the step)
    assert len(loop) <= PARENT_LOOP[KH], len(loop)
    assert not [o for o in loop if o.startswith("v_accvgpr")]
    assert not [o for o in loop if o.startswith("scratch_") or o.startswith("buffer_")]
    # bits 1 and 2: the addresses are a base plus an immediate
    assert n("v_add_u32") <= 2 and n("v_lshl_add_u32") == 0, (n("v_add_u32"), n("v_lshl_add_u32"))
    assert n("s_lshl_b32") == 0 and n("s_xor_b32") == 0 and n("s_add_i32") <= 1      # (the loop counter)
    assert n("s_barrier") == 3 and n("ds_write_b128") == 3
    assert n("ds_read_b128") == 16          # 3 x 4 partial sums, tbx, tbv_n, k1 -- and up = 1 - k1, read instead of computed
    assert n("v_sub_f32") == 4
    # bits 3 and 5 move work, they add none (the parent's counts: 64 / 32 / 40, and 40 | 48 residuals of the splits at KH = 3 | 4)
    assert n("v_exp_f32") == 64 and n("v_rcp_f32") == 32 and n("v_cvt_pk_f16_f32") == 40
    assert n("v_fma_mixlo_f16") + n("v_fma_mixhi_f16") + n("v_fma_mix_f32") == {3: 40, 4: 48}[KH]


def test_lds_plan_of_the_two_bodies():
    from l2hmc_amd import _ffi
    L = _ffi.lib()
    for d in (20, 50, 64):
        for T in (1, 10, 25):
            two = [L.l2hmc_sampler_lds_plan(d, T, 0, w) for w in range(3)]
            one = [L.l2hmc_sampler_lds_plan(d, T, 1, w) for w in range(3)]
            assert two[1] == 2 and one[1] == 3, (two, one)
            # records: two directions of T + 2 rows (+ 16 floats); 96 floats per row, and four wave blocks of 64 in the one-wave body
            assert two[2] == 4 * 2 * ((T + 2) * 96 + 16) and one[2] == 4 * 2 * ((T + 2) * 256 + 16)
            assert one[0] - two[0] == 4096 + one[2] - two[2]
            assert 0 < two[0] and (T > 10 or 2 * two[0] <= LDS_CU)          # two workgroups of the two-wave kernel share a CU
            assert one[0] <= LDS_CU
    # the bench's shape: 19 456 bytes more (4096 for the third buffer, 15 360 for the records), 95 376 of the CU's 163 840
    assert L.l2hmc_sampler_lds_plan(50, 10, 0, 0) == 75920 and L.l2hmc_sampler_lds_plan(50, 10, 1, 0) == 95376
    assert L.l2hmc_sampler_lds_plan(0, 10, 1, 0) == -1 and L.l2hmc_sampler_lds_plan(50, 10, 1, 3) == -1
    assert L.l2hmc_sampler_lds_plan(65, 10, 0, 0) == -1
