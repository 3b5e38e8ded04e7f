// Fused L2HMC kernels specialised for energy kind 10 (Bayesian binomial regression with the probit link, per-row offsets and
// trials): the general, energy and p_accept kernels; see l2hmc_kernels.hpp (regression_grad, ProbitLink), traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<10>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
