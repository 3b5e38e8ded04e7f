// traj_fast_kernel<1, ., ., ., 1>: the f16x2 form of the instruction-lean trajectory kernel for energy kind 1 (gauss_diag);
// its own translation unit so that the build stays parallel.  See traj_fast.hpp.
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_fast16_ek<1>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
