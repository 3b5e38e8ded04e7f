// Fused L2HMC kernels specialised for energy kind 9 (Bayesian binomial regression with trials, and negative-binomial regression
// with fixed dispersion: the logit link with per-row offsets and weights): the general, energy and p_accept kernels; see
// l2hmc_kernels.hpp (regression_grad, BinomialLink), traj_launch.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_ek<9>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
