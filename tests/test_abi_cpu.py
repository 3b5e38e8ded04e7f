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


# ---- the GEMM engine's host path (csrc/split.hip, csrc/train_split.hpp): its plan and its refusals, pinned --------------------
_HOST = (ctypes.c_float * 16)()                      # stands in for every device pointer: nothing below reaches a launch
_PTR = ctypes.addressof(_HOST)
_ENERGY_CB = _ffi.ENERGY_CALLBACK(lambda *a: 1)
_NET_CB = _ffi.NET_CALLBACK(lambda *a: 1)
_NET_VJP_CB = _ffi.NET_VJP_CALLBACK(lambda *a: 1)


def _fn(cb):
    return ctypes.cast(cb, ctypes.c_void_p).value


def _mlp3(n_in, n_h1, n_h2, n_out):
    m = _ffi.L2hmcMlp3()
    for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
        setattr(m, k, _PTR)
    m.n_in, m.n_h1, m.n_h2, m.n_out = n_in, n_h1, n_h2, n_out
    return m


def _engine_floats(query, N, d, H, T, enc, dec):
    enc, dec = (_mlp3(*enc) if enc else None), (_mlp3(*dec) if dec else None)
    return query(N, d, H, T, ctypes.byref(enc) if enc else None, ctypes.byref(dec) if dec else None)


IMAGE16 = (32, 4, 8, 5, (16, 8, 8, 8), (4, 8, 8, 16))          # image branch + decoder: 16 pixels, latent 4, H = 8
ENGINE_SHAPES = (
    ("no decoder: d = 10, H = 32, T = 5", (64, 10, 32, 5, None, None)),
    ("image branch + decoder: 16 pixels", IMAGE16),
    ("config-5 widths, 3071 chains: no planes", (3071, 50, 200, 2, (784, 512, 512, 200), (50, 1024, 1024, 784))),
    ("config-5 widths, 3072 chains: planes", (3072, 50, 200, 2, (784, 512, 512, 200), (50, 1024, 1024, 784))),
    ("caller-supplied nets: H = 4", (64, 4, 4, 5, None, None)),
)
# (l2hmc_split_workspace_floats, l2hmc_train_split_workspace_floats) of the library before the two entry points shared one
# host path: SplitPlan / TrainSplitPlan offsets and totals are part of what that refactor had to leave alone
ENGINE_PLAN = {
    "no decoder: d = 10, H = 32, T = 5": (18112, 1343808),
    "image branch + decoder: 16 pixels": (6352, 1110160),
    "config-5 widths, 3071 chains: no planes": (47913268, 174088528),
    "config-5 widths, 3072 chains: planes": (47926048, 174138816),
    "caller-supplied nets: H = 4": (5416, 1117896),
}


def test_gemm_engine_workspace_plan_is_pinned():
    """The two workspace queries make no HIP call: one row per family of slices the plan takes or leaves out (no decoder;
    image branch + decoder; config 5's widths on either side of the planes threshold; the H = 4 plan of caller-supplied nets)."""
    L = _ffi.lib()
    for name, shape in ENGINE_SHAPES:
        got = (_engine_floats(L.l2hmc_split_workspace_floats, *shape), _engine_floats(L.l2hmc_train_split_workspace_floats, *shape))
        assert got == ENGINE_PLAN[name], (name, got)


def _engine_block(which):
    """An argument block of the 16-pixel image sampler that passes every check of its entry point (the first HIP call would
    follow); returns it with the host objects it points to."""
    N, d, H, T, enc, dec = IMAGE16
    a = _ffi.L2hmcSplitArgs() if which == "sampler" else _ffi.L2hmcTrainSplitArgs()
    keep = dict(enc=_mlp3(*enc), dec=_mlp3(*dec), xnet=_ffi.L2hmcNet(), vnet=_ffi.L2hmcNet())
    a.xnet, a.vnet, a.H = ctypes.pointer(keep["xnet"]), ctypes.pointer(keep["vnet"]), H
    a.aux_encoder, a.decoder = ctypes.pointer(keep["enc"]), ctypes.pointer(keep["dec"])
    a.aux = a.masks = a.trig = a.x = a.v = a.workspace = _PTR
    a.eps_host, a.n_chains, a.d, a.T, a.workspace_floats = 0.1, N, d, T, 1 << 40
    if which == "sampler":
        a.n_steps = T
    else:
        a.Lx = a.p = a.v1 = a.grad = _PTR
        a.scale, a.inv_n = 1.0, 1.0 / N
    return a, keep


def _builtin(a, k, kind, **fields):
    """the block's target becomes a built-in energy (no decoder, no image branch, no images)"""
    e = k["energy"] = _ffi.L2hmcEnergy(kind=kind, mu=_PTR, prec=_PTR, temperature=1.0, **fields)
    a.energy, a.decoder, a.aux_encoder, a.aux = ctypes.pointer(e), None, None, None


def _set(**fields):
    def edit(a, k):
        for name, value in fields.items():
            setattr(a, name, value)
    return edit


def _enc_out_9(a, k):
    k["enc"].n_out = 9


def _net_cbs(a, k):
    a.net_cb = _fn(_NET_CB)
    if hasattr(a, "net_vjp_cb"):
        a.net_vjp_cb = _fn(_NET_VJP_CB)


# (case, edit of the passing block, return code, l2hmc_last_error) -- the texts as the library gave them before the refactor
_SHARED_WORDING = (
    ("aux_encoder output width != H", _enc_out_9, -1, "aux_encoder must map (N, n_pix) -> (N, H)"),
    ("decoder input width != d", _set(d=5), -1, "decoder input width != d"),
    ("eps_host = 0 without alpha", _set(eps_host=0.0), -1, "eps must be > 0"),
)
ENGINE_REFUSALS = {
    "sampler": _SHARED_WORDING + (
        ("gemm_mode 4", _set(gemm_mode=4), -1,
         "gemm_mode must be 0 (f32 MFMA), 1 (bf16x3), 2 (bf16x3, split in the loop) or 3 (f16x2 planes)"),
        ("energy_cb with a decoder", _set(energy_cb=_fn(_ENERGY_CB)), -1, "energy_cb excludes decoder and energy"),
        ("net_cb with xnet", _net_cbs, -1, "net_cb excludes xnet / vnet / aux_encoder / hmc"),
        ("workspace one float short", _set(workspace_floats=6352 - 1), -1, "workspace too small: need 6352 floats"),
    ),
    "trainer": _SHARED_WORDING + (
        ("gemm_mode 4", _set(gemm_mode=4), -1,
         "gemm_mode must be 0 (f32 MFMA), 1 (bf16x3), 2 (bf16x3, split in the loop) or 3 (f16x2 planes for the forward "
         "evaluations, bf16x3 for the reverse sweep)"),
        ("energy_cb with a decoder", _set(energy_cb=_fn(_ENERGY_CB)), -1, "energy_cb excludes a built-in energy and decoder"),
        ("net_cb with xnet", _net_cbs, -1,
         "net_cb excludes xnet / vnet / aux_encoder (an image branch is the caller's net's own business)"),
        ("workspace one float short", _set(workspace_floats=1110160 - 1), -1, "workspace too small: need 1110160 floats"),
        ("net_cb without net_vjp_cb", _set(net_cb=_fn(_NET_CB)), -1,
         "training caller-supplied nets needs BOTH net_cb and net_vjp_cb"),
        ("energy_cb without hvp_cb", _set(energy_cb=_fn(_ENERGY_CB), decoder=None), -1,
         "training on a caller-supplied energy needs hvp_cb (the loss differentiates through grad U)"),
        ("dense Gaussian without hess", lambda a, k: _builtin(a, k, _ffi.ENERGY_GAUSS_DENSE), -1,
         "dense Gaussian / mixture: hess = the RAW (n_comp, d, d) precisions"),
        ("logistic regression", lambda a, k: _builtin(a, k, _ffi.ENERGY_LOGISTIC, n_comp=8, eta=4.0), -2,
         "the GEMM engine does not train on the logistic-regression target (its Hessian-vector product lives in "
         "l2hmc_train_propose_grad's tile kernel): train there, or on the same likelihood as a caller-supplied energy"),
    ),
}


def _refusal(L, which, edit):
    a, keep = _engine_block(which)
    edit(a, keep)
    rc = (L.l2hmc_trajectory_split if which == "sampler" else L.l2hmc_train_split_grad)(ctypes.byref(a), None)
    return rc, L.l2hmc_last_error().decode()


@pytest.mark.parametrize("which", ("sampler", "trainer"))
def test_gemm_engine_refusals_are_pinned(which):
    """Argument blocks both entry points of the GEMM engine refuse before any HIP call: return code and message, word for word.
    Where the two word the same refusal differently, each keeps its own text."""
    L = _ffi.lib()
    for name, edit, rc, msg in ENGINE_REFUSALS[which]:
        assert _refusal(L, which, edit) == (rc, msg), (which, name)
