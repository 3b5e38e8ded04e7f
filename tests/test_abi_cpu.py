"""CPU: the C-ABI library loads and exports every symbol include/l2hmc.h declares; host-side
argument validation works without a GPU (no compute calls)."""
import ctypes
import os
import re

import pytest

from l2hmc_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    declared = set(re.findall(r"\b(l2hmc_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no prototypes found in the header"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "missing export %s" % name
    assert declared == set(_ffi.SYMBOLS), (declared ^ set(_ffi.SYMBOLS))


def test_abi_version_and_size_queries():
    L = _ffi.lib()
    assert L.l2hmc_abi_version() == 6 == _ffi.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "l2hmc.h")).read()
    assert int(re.search(r"#define L2HMC_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION
    # MFMA fragments (5 NT + 2 groups of 256 + 32 NT scales per net) + the lane layout (traj_lane.hpp: rows of RS = 12)
    lane = (2 * 50 * 12 + 3 * 12 + 10 * 12 + 12 + 25 * (6 * 10 + 12) + 3) // 4 * 4      # DP = 50 rows, 10 units
    # ... + (round 6) the same groups once more as f16x2 fragment pairs (2 x 16 bytes per lane: 512 floats per group)
    assert L.l2hmc_packed_nets_floats(50, 10) == 2 * ((5 * 4 + 2) * 256 + 32 * 4) + 2 * lane + 2 * (5 * 4 + 2) * 512
    lane2 = (2 * 2 * 12 + 3 * 12 + 10 * 12 + 12 + 1 * (6 * 10 + 12) + 3) // 4 * 4       # DP = 2
    assert L.l2hmc_packed_nets_floats(2, 10) == 2 * (7 * 256 + 32) + 2 * lane2 + 2 * 7 * 512
    assert L.l2hmc_packed_gaussian_floats(50) == 16 * 256
    assert L.l2hmc_packed_nets_floats(50, 16) == -2          # unsupported hidden width
    assert b"H <= 15" in L.l2hmc_last_error()


def test_argument_validation_without_gpu():
    L = _ffi.lib()
    a = _ffi.L2hmcTrajectoryArgs()
    assert L.l2hmc_trajectory(None, None) == -1
    a.n_chains, a.d, a.T = 16, 2, 10
    assert L.l2hmc_trajectory(a, None) == -1                 # x, v, masks, trig missing
    assert b"required" in L.l2hmc_last_error()
    with pytest.raises(RuntimeError, match="libl2hmc_hip"):
        _ffi.check(L.l2hmc_trajectory(a, None))
    assert L.l2hmc_mh_select(None, None, None, None, 4, 2, None, None) == -1
    assert L.l2hmc_loss_terms(None, 4, 0.1, 0.25, None, None) == -1
    # which training shapes a fused kernel holds (the host hands the others to the GEMM-engine trainer): pure host logic
    G, D, M, R, F = (_ffi.ENERGY_GAUSS_DIAG, _ffi.ENERGY_GAUSS_DENSE, _ffi.ENERGY_GMM, _ffi.ENERGY_ROUGHWELL, _ffi.ENERGY_FUNNEL)
    assert L.l2hmc_train_fused_lds_bytes(D, 1, 2, 10, 10) > 0            # notebook config: the d <= 4 kernel
    assert L.l2hmc_train_fused_lds_bytes(M, 2, 2, 10, 10) > 0            # mixtures on it too
    assert 0 < L.l2hmc_train_fused_lds_bytes(G, 1, 50, 10, 10) <= 160 * 1024      # ICG-50: register-resident, one workgroup per CU
    assert L.l2hmc_train_fused_lds_bytes(R, 1, 128, 10, 10) == -2        # beyond the 16-chain tile's LDS plan
    assert L.l2hmc_train_fused_lds_bytes(G, 1, 50, 40, 10) == -2         # wide nets
    assert L.l2hmc_train_fused_lds_bytes(F, 1, 16, 10, 10) > 0 and L.l2hmc_train_fused_lds_bytes(F, 1, 20, 10, 10) == -2
    assert L.l2hmc_train_fused_lds_bytes(99, 1, 2, 10, 10) == -2 and L.l2hmc_train_fused_lds_bytes(G, 1, 0, 10, 10) == -1


def test_fused_trainer_query_pins_each_family_and_refusal():
    """`l2hmc_train_fused_lds_bytes` answers from the launch's own plan (`plan_train`, csrc/train.hip): the dynamic LDS of
    the kernel it picks -- the d <= 4 kernel (train_small.hpp), the register-resident kernel with one or four waves
    (train_fast.hpp), the general tile kernel -- or the rule that refused.  Pure host logic, no launch."""
    L = _ffi.lib()
    G, D, M, R, F = (_ffi.ENERGY_GAUSS_DIAG, _ffi.ENERGY_GAUSS_DENSE, _ffi.ENERGY_GMM, _ffi.ENERGY_ROUGHWELL, _ffi.ENERGY_FUNNEL)
    for args, lds in (((G, 1, 2, 10, 10), 31728), ((D, 1, 4, 15, 5), 30976),            # d <= 4
                      ((G, 1, 16, 10, 10), 26512), ((F, 1, 16, 10, 40), 32512),         # register-resident, one wave
                      ((G, 1, 50, 10, 10), 89488),                                      # ... four waves
                      ((M, 2, 5, 10, 10), 31232), ((R, 1, 17, 16, 10), 67888)):         # general tile kernel
        assert L.l2hmc_train_fused_lds_bytes(*args) == lds, args
    for args, msg in (((F, 1, 17, 10, 10), b"funnel: the fused trainer holds 2 <= d <= 16"),
                      ((R, 1, 128, 10, 10), b"needs 300144 bytes of LDS (> 160 KiB)"),
                      ((G, 1, 4097, 10, 10), b"d / H too large"),
                      ((99, 1, 2, 10, 10), b"no fused training kernel for this energy kind")):
        assert L.l2hmc_train_fused_lds_bytes(*args) == -2, args
        assert msg in L.l2hmc_last_error(), (args, L.l2hmc_last_error())


def test_struct_layout_matches_header():
    # field order / sizes of the ctypes mirrors (x86-64: pointers 8, ints 4, natural alignment)
    assert ctypes.sizeof(_ffi.L2hmcNet) == 16 * 8
    assert ctypes.sizeof(_ffi.L2hmcEnergy) == 56
    assert _ffi.L2hmcTrajectoryArgs.energy.offset == 8
    assert _ffi.L2hmcTrajectoryArgs.n_chains.offset == 8 + 56 + 3 * 8 + 8
    assert _ffi.L2hmcTrajectoryArgs.ais_alpha.offset == ctypes.sizeof(_ffi.L2hmcTrajectoryArgs) - 8
    assert _ffi.L2hmcTrajectoryArgs.ais_beta.offset == _ffi.L2hmcTrajectoryArgs.chain_offset.offset + 8
    assert _ffi.L2hmcTrajectoryArgs.rng_seed.offset == _ffi.L2hmcTrajectoryArgs.x_hist.offset + 16
    # `net_mode` (round 5) took the padding behind `gemm_mode`: the callbacks that follow keep their offsets
    T = _ffi.L2hmcTrainSplitArgs
    assert T.net_mode.offset == T.gemm_mode.offset + 4 and T.energy_cb.offset == T.gemm_mode.offset + 8
    # ABI 6: three trailing pointers (net_cb, net_vjp_cb, net_cb_user) -- every earlier offset is unchanged
    assert T.net_cb.offset == 312 and T.net_cb_user.offset == 328 and ctypes.sizeof(T) == 336


def test_struct_sizes_are_checked_against_the_library():
    """include/l2hmc.h `l2hmc_struct_bytes`: the binding's mirrors and the compiled structs agree (checked at load too),
    an unknown id is an argument error."""
    L = _ffi.lib()
    for which, mirror in enumerate(_ffi.STRUCTS):
        assert L.l2hmc_struct_bytes(which) == ctypes.sizeof(mirror), mirror.__name__
    assert L.l2hmc_struct_bytes(99) == -1


def test_graft_entry_build_is_consistent_with_the_library():
    """The driver's build check: `__graft_entry__.build()` (make is a no-op on an up-to-date tree) must accept the
    library it has just built -- its ABI assertion follows the binding's version."""
    import __graft_entry__ as ge
    ge.build()


def test_hot_kernels_keep_their_register_budgets():
    """Round 6's two occupancy findings as a build check (tools/kernel_resources.py reads the compiler's listings; skipped when the
    library was not built here): the f16x2 kernels that run a step loop per launch do not spill to scratch inside it, and every kernel
    whose design counts on two waves per SIMD fits 256 registers (the four-wave wide kernel sat at 314-324 = one workgroup per CU
    for four rounds; the two-tiles-per-wave f16x2 kernels spilled 220-630 bytes per lane under a bound meant for one tile)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    res = kr.resources()
    if not res.get("traj_f16_ek1.s"):
        import pytest
        pytest.skip("no compiler listings under l2hmc_amd/csrc/build/asm (library built elsewhere)")
    rows = {(f, k): (vg, sc) for f, ks in res.items() for k, vg, sc, _ in ks}
    # the bench kernel and its relatives: no scratch, two waves per SIMD
    for k in ("traj_fast_kernel<1, 1, 4, 3, 1>", "traj_fast_kernel<1, 1, 4, 4, 1>", "traj_fast_kernel<1, 1, 1, 3, 1>"):
        vg, sc = rows[("traj_f16_ek1.s", k)]
        assert sc == 0 and vg <= 256, (k, vg, sc)
    # two tiles per wave, f16x2: one wave per SIMD by design, the overflow in AGPRs -- never scratch
    for f in ("traj_f16_ek1.s", "traj_f16_ek4.s"):
        for (ff, k), (vg, sc) in rows.items():
            if ff == f and k.startswith("traj_fast_kernel<") and k.split(", ")[1] == "2":
                assert sc == 0 and vg <= 512, (k, vg, sc)
    for (f, k), (vg, sc) in rows.items():
        if k.startswith("traj_tile_kernel<1,") or k.startswith("traj_small_kernel<"):
            assert sc == 0 and vg <= 256, (k, vg, sc)
        if k.startswith("traj_tile_kernel<") or k.startswith("gemm_xlp_kernel<") or k.startswith("net_eval_kernel<2, 8"):
            assert vg <= 256, (k, vg)
        if k.startswith("traj_wide_kernel<") and k.split(", ")[2].rstrip(">") == "4":      # NW = 4: two workgroups per CU
            assert vg <= 256, (k, vg)
        if f in ("train.s", "split.s", "l2hmc_abi.s"):
            assert sc == 0, (f, k, sc)
