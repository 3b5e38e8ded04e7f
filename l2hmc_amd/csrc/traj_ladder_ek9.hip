// The ladder (parallel-tempering) form of the general trajectory kernel for energy kind 9 (binomial / negative-binomial
// regression); see l2hmc_kernels.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ladder_ek<9>(const TrajPlan& p, const KArgs& k, const LadArgs& l, hipStream_t s);
}  // namespace l2hmc
