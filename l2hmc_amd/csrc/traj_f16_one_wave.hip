// traj_fast_cc_kernel<1, 1, 4, ., 1, 1>: the common-launch body of the diagonal Gaussian's one-tile f16x2 kernel (the bench workload
// and its H = 11 ... 15 relative) under __launch_bounds__(256, 1), for grids of at most one workgroup per CU.  A translation unit of
// its own because the Makefile gives it -mllvm -amdgpu-mfma-vgpr-form (traj_fast.hpp, the note at L2HMC_FAST_WAVES).
#include "traj_launch.hpp"

namespace l2hmc {
int launch_fast16_one_wave(const TrajPlan& p, const KArgs& k, hipStream_t s) {
  if (p.ek != L2HMC_ENERGY_GAUSS_DIAG || p.DT != 1 || p.NW != 4 || !p.f16)
    return fail(L2HMC_ERR_UNSUPPORTED, "no one-workgroup-per-CU kernel for this plan%s");
  return on_either<3, 4>(p.KH == 3, [&](auto KH) {
    return launch_tiles(traj_fast_cc_kernel<L2HMC_ENERGY_GAUSS_DIAG, 1, 4, KH, 1, 1>, 4, p, k, s);
  });
}
}  // namespace l2hmc
