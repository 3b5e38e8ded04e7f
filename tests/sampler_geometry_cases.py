"""The launches tests/test_gpu_sampler_geometries.py holds the one-wave-per-tile kernel `traj_tile_kernel<EK, DT, KH, TPW, HALF>`
(l2hmc_amd/csrc/traj_tile.hpp) and the one-chain-per-lane kernel `traj_lane_kernel<EK, DP, HPR[, RES]>` (traj_lane.hpp) to, one
per compiled form.

One place says what a case launches, so that the CPU check of its inputs (tests/test_sampler_geometries_cpu.py) and the GPU tests
cannot drift apart.  Every case is the smallest shape at which its form can go wrong:

  * tile family, 40 chains: two full 16-chain tiles and one half-live tile in one four-tile workgroup, whose fourth wave leaves
    after the prologue's barriers (72 chains: five tiles, the second workgroup has one live wave); d picks the slice count
    DT = ceil(d / 16) and the padding of the last slice (1 or 2 live dimensions: the HALF form; 3 ... 16: the full one), H the
    hidden k-steps KH = (H + 4) / 4 with 11 | 12 as the boundary;
  * lane family, 100 chains: one full wave and a ragged one of 36 lanes; d = 1, 3 pad a dimension (DP = 2, 4), H = 7, 11, 15 pad
    hidden units (HPR = 5 serves H <= 10, 8 serves H <= 16);
  * M = 3 banked proposals cross two proposal boundaries; T = 5.

Step sizes: tile shapes at eps = 0.05 and lane shapes at eps = 0.2 keep the float64 oracle's accepted share of the first proposal
inside 0.2 ... 0.9 (at eps = 0.1 most tile shapes accept below 0.2 and most lane shapes outside the band); the rows that needed
another seed or step size to meet the conditions of tests/test_sampler_geometries_cpu.py say so beside them.

Energy kinds in the names: 1 diagonal Gaussian, 2 dense Gaussian, 3 mixture, 4 Rough Well.  A one-dimensional Gaussian has no
off-diagonal to be free of: `distributions.Gaussian` hands d = 1 to the dense kernels (kind 2) whatever its covariance, so the
`gauss_diag` row at d = 1 launches the dense form, and the diagonal Gaussian's own resident form <1, 2, 5, 2> has a row at d = 2.
"""
import numpy as np

from oracle import l2hmc_oracle as O

from . import helpers

M = 3                       # banked proposals of the loop tests
DRAWS_SEED = 20250611       # the banked draws (v, direction, u)
SPLIT = 24                  # the two launches of "chains never interact" split here: no multiple of 16 or 64
BIG_BASE = 256              # the cases beyond 100 chains tile a synthetic case of this many chains and add NOISE of jitter
NOISE = 0.01
HEAD, TAIL = 192, 40        # ... and are held to the oracle on their first HEAD and last TAIL chains

TILE = "traj_tile_kernel"
LANE = "traj_lane_kernel"


def _tile(kind, d, H, kernel, **kw):
    return dict(dict(kind=kind, d=d, H=H, T=5, eps=0.05, N=40, variant=16, kernel=(TILE if kernel[0] == "<" else "") + kernel), **kw)


def _lane(kind, d, H, kernel, **kw):
    return dict(dict(kind=kind, d=d, H=H, T=5, eps=0.2, N=100, variant=32, kernel=(LANE if kernel[0] == "<" else "") + kernel), **kw)


# name -> what the case launches.  kind: a `helpers.synthetic_case` kind; N: a chain count, or (chains per CU, extra chains) for the
# cases whose point is a threshold of the planner (plan_trajectory, l2hmc_abi.hip: its thresholds are chains per compute unit);
# kernel: what `_ffi.last_kernel()` must report after the launch (note_plan, l2hmc_abi.hip); lane_res: L2HMC_LANE_RES for the launch
# (the planner's own rule picks a resident form at d <= 2, H <= 10 below 196 608 chains: "0" is how few chains reach the base form)
CASES = {
    # ---- one wave per tile, four tiles per workgroup: EK x DT x KH x HALF ----------------------------------------------------
    "t_g33_h10": _tile("gauss_diag", 33, 10, "<1, 3, 3, 4, true>"),          # one live dimension in the last slice
    "t_g34_h12": _tile("gauss_diag", 34, 12, "<1, 3, 4, 4, true>"),
    "t_g35_h11": _tile("gauss_diag", 35, 11, "<1, 3, 3, 4, false>"),
    "t_g48_h15": _tile("gauss_diag", 48, 15, "<1, 3, 4, 4, false>"),         # no padding
    "t_g49_h11": _tile("gauss_diag", 49, 11, "<1, 4, 3, 4, true>"),
    "t_g50_h15": _tile("gauss_diag", 50, 15, "<1, 4, 4, 4, true>"),
    "t_g51_h10": _tile("gauss_diag", 51, 10, "<1, 4, 3, 4, false>"),
    "t_g64_h12": _tile("gauss_diag", 64, 12, "<1, 4, 4, 4, false>"),
    "t_rw34_h11": _tile("roughwell_easy", 34, 11, "<4, 3, 3, 4, true>"),
    "t_rw33_h15": _tile("roughwell_easy", 33, 15, "<4, 3, 4, 4, true>"),
    "t_rw48_h10": _tile("roughwell_easy", 48, 10, "<4, 3, 3, 4, false>"),
    "t_rw35_h12": _tile("roughwell_easy", 35, 12, "<4, 3, 4, 4, false>"),
    "t_rw50_h10": _tile("roughwell_easy", 50, 10, "<4, 4, 3, 4, true>"),
    "t_rw49_h12": _tile("roughwell_easy", 49, 12, "<4, 4, 4, 4, true>"),
    "t_rw64_h11": _tile("roughwell_easy", 64, 11, "<4, 4, 3, 4, false>"),
    "t_rw51_h15": _tile("roughwell_easy", 51, 15, "<4, 4, 4, 4, false>"),
    "t_g40_n72": _tile("gauss_diag", 40, 10, "<1, 3, 3, 4, false>", N=72),   # five tiles: the second workgroup has one live wave
    # ---- eight tiles per workgroup: variant 0 from 128 chains per CU once two workgroups' LDS plans no longer share a CU -------
    # plan_lds_tile at DT = 3 is 68 096 + 640 (T + 2) bytes: above half of 160 KiB from T = 20 on (T = 19 launches TPW = 4:
    # `t_below`, asserted by name); the last workgroup holds two full tiles, a half-live one and five waves that leave early
    "t8_g40": _tile("gauss_diag", 40, 10, "<1, 3, 3, 8, false>", T=20, eps=0.02, N=(128, 40), variant=0, forced=16, t_below=19),
    # at DT = 4 the staged tables alone are 89 216 bytes: every schedule length, T = 1 included, plans TPW = 8 (asserted by name at
    # T = 1: `t_floor`); the case keeps the family's T = 5
    "t8_rw64_h12": _tile("roughwell_easy", 64, 12, "<4, 4, 4, 8, false>", N=(128, 40), variant=0, forced=16, t_floor=1),
    # ---- one chain per lane: EK x DP x HPR, and the resident forms of DP = 2, HPR = 5 ---------------------------------------------
    "l_gd_d1_h7": _lane("gauss_diag", 1, 7, "<2, 2, 5, 1>"),                 # (d = 1: the dense kind, see the module docstring)
    "l_gd_d2_h9": _lane("gauss_diag", 2, 9, "<1, 2, 5, 2>"),
    "l_gd_d2_h11": _lane("gauss_diag", 2, 11, "<1, 2, 8>"),
    "l_gd_d3_h10": _lane("gauss_diag", 3, 10, "<1, 4, 5>"),
    "l_gd_d4_h15": _lane("gauss_diag", 4, 15, "<1, 4, 8>"),
    "l_dense_d1_h7": _lane("gauss_dense", 1, 7, "<2, 2, 5, 1>"),
    "l_dense_d2_h11": _lane("gauss_dense", 2, 11, "<2, 2, 8>"),
    "l_dense_d3_h10": _lane("gauss_dense", 3, 10, "<2, 4, 5>"),
    "l_dense_d4_h15": _lane("gauss_dense", 4, 15, "<2, 4, 8>"),
    "l_gmm3_d1_h7": _lane("gmm3", 1, 7, "<3, 2, 5, 1>"),
    "l_gmm3_d2_h11": _lane("gmm3", 2, 11, "<3, 2, 8>"),
    "l_gmm3_d3_h10": _lane("gmm3", 3, 10, "<3, 4, 5>"),
    "l_gmm3_d4_h15": _lane("gmm3", 4, 15, "<3, 4, 8>"),
    "l_rw_d1_h7": _lane("roughwell_easy", 1, 7, "<4, 2, 5, 1>"),
    "l_rw_d2_h11": _lane("roughwell_easy", 2, 11, "<4, 2, 8>"),
    "l_rw_d3_h10": _lane("roughwell_easy", 3, 10, "<4, 4, 5>"),
    "l_rw_d4_h15": _lane("roughwell_easy", 4, 15, "<4, 4, 8>"),
    "l_gmm8_d4_h10": _lane("gmm8", 4, 10, "<3, 4, 5>"),
    # the base forms of DP = 2, HPR = 5 (weights by scalar loads in the loop): the same inputs as the resident rows above
    "l_gd_d2_h9_res0": _lane("gauss_diag", 2, 9, "<1, 2, 5>", lane_res="0", like="l_gd_d2_h9"),
    "l_dense_d1_h7_res0": _lane("gauss_dense", 1, 7, "<2, 2, 5>", lane_res="0", like="l_dense_d1_h7"),
    "l_gmm3_d1_h7_res0": _lane("gmm3", 1, 7, "<3, 2, 5>", lane_res="0", like="l_gmm3_d1_h7"),
    "l_rw_d1_h7_res0": _lane("roughwell_easy", 1, 7, "<4, 2, 5>", lane_res="0", like="l_rw_d1_h7"),
    # ---- the planner's thresholds (variant 0): the first chain count of the family, and 16 chains fewer ---------------------------
    # 64 chains per CU, 3-4 dimension slices, an elementwise target: one wave per tile; below, four waves per tile (f16x2)
    "p_tile": _tile("gauss_diag", 40, 10, "<1, 3, 3, 4, false>", N=(64, 0), variant=0, forced=16),
    "p_tile_below": _tile("gauss_diag", 40, 10, "traj_fast_kernel<1, 1, 4, 3, 1>", N=(64, -16), variant=0),
    # 512 chains per CU at d <= 4: one chain per lane; below, the d <= 4 MFMA kernel (f16x2 nets)
    "p_lane": _lane("roughwell_easy", 3, 10, "<4, 4, 5>", N=(512, 0), variant=0, forced=32),
    "p_lane_below": _lane("roughwell_easy", 3, 10, "traj_small_kernel<4, 3, 1>", N=(512, -16), variant=0),
}

SMALL = sorted(n for n, c in CASES.items() if isinstance(c["N"], int))            # N <= 100: every test, the CPU conditions
BIG = sorted(n for n, c in CASES.items() if not isinstance(c["N"], int))
TPW8 = ("t8_g40", "t8_rw64_h12")
PARTIAL = ("t_g35_h11", "l_gd_d3_h10")                                            # partial trajectories: one tile, one lane case
assert all(CASES[n]["N"] <= 100 for n in SMALL)

# per case: synthetic_case seed (nets, mask, energy parameters, x).  The default is the case's position in the table; a row here
# replaces it where the default missed a condition of tests/test_sampler_geometries_cpu.py (the reason beside it)
SEEDS = {
    "l_gmm3_d1_h7": 1111,       # (the default seed's mixture accepts 0.92 of the first proposal)
}


class Case(object):
    """One row of CASES with its inputs: g (golden-shaped dict: nets, mask, step size, energy parameters), and the host arrays
    x (N, d), v (M, N, d), dr (M, N) u8, u (M, N).  `cus`: the device's compute units, for the rows whose N is per CU."""

    def __init__(self, name, cus=None):
        c = CASES[name]
        self.name, self.kernel, self.variant = name, c["kernel"], int(c["variant"])
        self.kind, self.d, self.H, self.T, self.eps = c["kind"], int(c["d"]), int(c["H"]), int(c["T"]), float(c["eps"])
        self.lane_res, self.forced = c.get("lane_res"), c.get("forced")
        self.t_below, self.t_floor = c.get("t_below"), c.get("t_floor")
        like = c.get("like", name)                              # (a row may share another row's inputs)
        seed = SEEDS.get(like, 100 + sorted(CASES).index(like))
        rng = np.random.RandomState(DRAWS_SEED)
        if isinstance(c["N"], int):
            self.N = c["N"]
            self.g = helpers.synthetic_case(self.kind, self.d, H=self.H, T=self.T, N=self.N, seed=seed, eps=self.eps)
            self.x = self.g["x"]
            self.idx = np.arange(self.N)
        else:
            assert cus is not None, "the chain count of %s is per compute unit" % name
            self.N = c["N"][0] * int(cus) + c["N"][1]
            self.g = helpers.synthetic_case(self.kind, self.d, H=self.H, T=self.T, N=BIG_BASE, seed=seed, eps=self.eps)
            reps = (self.N + BIG_BASE - 1) // BIG_BASE
            self.x = (np.tile(self.g["x"], (reps, 1))[:self.N] + NOISE * rng.randn(self.N, self.d)).astype(np.float32)
            self.idx = np.r_[np.arange(HEAD), np.arange(self.N - TAIL, self.N)]
        self.v = rng.randn(M, self.N, self.d).astype(np.float32)
        self.dr = rng.randint(0, 2, size=(M, self.N)).astype(np.uint8)
        self.u = rng.uniform(size=(M, self.N)).astype(np.float32)
        self._first = {}

    # ---- the numpy side ---------------------------------------------------------------------------------------------------
    def oracle_dynamics(self, dtype=np.float32):
        return helpers.oracle_dynamics(self.g, dtype)

    def first_proposal(self, dtype):
        """(Lx, p, x_next) of the first banked proposal at `dtype`, on the chains `idx`; computed once."""
        key = np.dtype(dtype).name
        if key not in self._first:
            i = self.idx
            v = self.v[0][i].astype(dtype)
            with np.errstate(all="ignore"):
                Lx, _, p, xn = O.propose(self.x[i].astype(dtype), self.oracle_dynamics(dtype), v, v, self.dr[0][i],
                                         self.u[0][i].astype(dtype), both_directions=False)
            self._first[key] = (Lx, p, xn)
        return self._first[key]

    def check_inputs(self):
        """The conditions on a case's inputs, from the oracle's first proposal: every float64 trajectory finite with |Lx| < 1e3; an
        accepted share in 0.2 ... 0.9 (the accept and the reject-and-restore path both run); at most 2 % of the chains within 1e-4
        of a tie.  Returns (accepted share, near ties, the float32 oracle's relative error in Lx, its error in p)."""
        Lx, p, _ = self.first_proposal(np.float64)
        Lx32, p32, _ = self.first_proposal(np.float32)
        u = self.u[0][self.idx].astype(np.float64)
        assert np.all(np.isfinite(Lx)) and np.all(np.isfinite(p)) and float(np.abs(Lx).max()) < 1e3, self.name
        acc = float((p >= u).mean())
        assert 0.2 <= acc <= 0.9, (self.name, acc)
        near = int((np.abs(p - u) < 1e-4).sum())
        assert near <= 0.02 * len(u), (self.name, near)
        return acc, near, helpers.rel_err(Lx32, Lx), helpers.abs_err(p32, p)

    # ---- the HIP side -----------------------------------------------------------------------------------------------------
    def hip_dynamics(self, variant=None, T=None):
        """`T`: the same target and nets under another schedule length (the TPW = 8 thresholds; only the kernel's name is read)."""
        g = self.g
        if T is not None and T != self.T:
            g = helpers.synthetic_case(self.kind, self.d, H=self.H, T=T, N=16, seed=1, eps=self.eps)
        return helpers.hip_dynamics(g, variant=self.variant if variant is None else variant)


_cache = {}


def case(name, cus=None):
    if name not in _cache:
        _cache[name] = Case(name, cus)
    return _cache[name]
