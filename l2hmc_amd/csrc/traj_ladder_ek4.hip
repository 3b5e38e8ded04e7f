// The ladder (parallel-tempering) form of the general trajectory kernel for energy kind 4 (roughwell); see l2hmc_kernels.hpp.
#include "l2hmc_kernels.hpp"

namespace l2hmc {
L2HMC_DEFINE_LAUNCH_LADDER(4)
}  // namespace l2hmc
