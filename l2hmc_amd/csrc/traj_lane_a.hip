// one-chain-per-lane kernels (traj_lane.hpp): diagonal Gaussian
#include "traj_lane_inst.hpp"
namespace l2hmc {
template int launch_lane_ek<1>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}
