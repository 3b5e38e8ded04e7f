// Fused L2HMC kernels specialised for energy kind 5 (funnel): the general, instruction-lean (f32-input MFMA), energy and
// p_accept kernels; see l2hmc_kernels.hpp, traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<5>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
