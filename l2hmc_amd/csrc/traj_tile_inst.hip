// The one-wave-per-tile kernels (traj_tile.hpp) of both elementwise targets, in a translation unit of their own: the
// instruction-lean 4-wave kernels next door (traj_ek1, traj_ek4) are compiled with LLVM's max-ILP scheduling strategy
// (+1 % on the headline configuration), which costs this kernel registers it does not have (256 VGPRs + scratch, -2 % at
// 16 384 chains: profiles/r03_exchange_variants.txt).
#include "traj_launch.hpp"

namespace l2hmc {
template int launch_tile_ek<1>(const TrajPlan& p, const KArgs& k, hipStream_t s);
template int launch_tile_ek<4>(const TrajPlan& p, const KArgs& k, hipStream_t s);
}  // namespace l2hmc
