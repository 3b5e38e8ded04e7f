// the launcher template of traj_lane.hpp, instantiated once per energy kind by traj_lane_a / _b / _c.hip (compile time)
#pragma once
#include "traj_lane.hpp"

namespace l2hmc {

// traj_lane_kernel<EK, p.DP, p.HPR, p.RES>: one chain per lane, 64 per workgroup, no dynamic LDS
template <int EK>
int launch_lane_ek(const TrajPlan& p, const KArgs& k, hipStream_t s) {
  const float* wx = k.packed + 2 * (size_t)net_floats(k.NT);
  const float* wv = wx + lane_layout(k.d, k.H).total;
  auto go = [&](auto kern) { return launch_kernel(kern, (k.N + 63) / 64, 64, 0, s, k, wx, wv, k.masks, k.trig, k.mu, k.prec, k.logc); };
  return on_either<2, 4>(p.DP == 2, [&](auto DP) {
    if constexpr (DP == 2) {                     // (the resident forms: d <= 2, H <= 10 only)
      if (p.RES == 2) return go(traj_lane_kernel<EK, 2, 5, 2>);
      if (p.RES == 1) return go(traj_lane_kernel<EK, 2, 5, 1>);
    }
    return p.HPR == 5 ? go(traj_lane_kernel<EK, DP, 5>) : go(traj_lane_kernel<EK, DP, 8>);
  });
}

}  // namespace l2hmc
