// one-chain-per-lane kernels (traj_lane.hpp): dense Gaussian and mixtures, and which (energy kind, d, H) have one
#include "traj_lane_inst.hpp"
namespace l2hmc {
template int launch_lane_ek<2>(const TrajPlan& p, const KArgs& k, hipStream_t s);
template int launch_lane_ek<3>(const TrajPlan& p, const KArgs& k, hipStream_t s);

bool lane_supported(int ek, int d, int H, int ncomp) {
  if (H < 1 || H > 16) return false;
  switch (ek) {
    case L2HMC_ENERGY_GAUSS_DIAG:
    case L2HMC_ENERGY_ROUGHWELL:
    case L2HMC_ENERGY_GAUSS_DENSE: return d <= 4;
    case L2HMC_ENERGY_GMM: return d <= 4 && ncomp >= 1;
    default: return false;
  }
}
}  // namespace l2hmc
