// The ladder (parallel-tempering) form of the general trajectory kernel for energy kind 10 (probit regression); see
// l2hmc_kernels.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ladder_ek<10>(const TrajPlan& p, const KArgs& k, const LadArgs& l, hipStream_t s);
}  // namespace l2hmc
