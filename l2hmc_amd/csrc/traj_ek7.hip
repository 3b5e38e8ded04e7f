// Fused L2HMC kernels specialised for energy kind 7 (Bayesian logistic regression): the general, energy and p_accept kernels;
// see l2hmc_kernels.hpp (regression_grad), traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<7>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
