// Fused L2HMC kernels specialised for energy kind 1 (gauss_diag): the general, instruction-lean (f32-input MFMA), small, energy and
// p_accept kernels; see l2hmc_kernels.hpp, traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<1>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
