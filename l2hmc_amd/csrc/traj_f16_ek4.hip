// traj_fast_kernel<4, ., ., ., 1>: the f16x2 form of the instruction-lean trajectory kernel for energy kind 4 (roughwell);
// its own translation unit so that the build stays parallel.  See traj_fast.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_fast16_ek<4>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
