// Fused L2HMC kernels specialised for energy kind 8 (Bayesian Poisson regression, log link with offsets): the general, energy
// and p_accept kernels; see l2hmc_kernels.hpp (regression_grad, PoissonLink), traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<8>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
