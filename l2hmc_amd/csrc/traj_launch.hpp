// traj_launch.hpp -- the launcher templates declared in l2hmc_kernels.hpp for the MFMA trajectory, energy and p_accept kernels.
// Included by the translation units that instantiate them (traj_ek<k>.hip, traj_f16_ek<k>.hip, traj_ladder_ek<k>.hip,
// traj_tile_inst.hip) and by nothing else: a unit compiles exactly the kernels its explicit instantiations name.
#pragma once
#include "traj_small.hpp"
#include "traj_tile.hpp"

namespace l2hmc {

// (k.N chains in 16-chain tiles, one workgroup of NW waves per tile)
template <class K, class... X>
int launch_tiles(K kern, int NW, const TrajPlan& p, const KArgs& k, hipStream_t s, const X&... extra) {
  return launch_kernel(kern, (k.N + 15) / 16, 64 * NW, p.lds, s, k, extra...);
}

// the general kernel's geometries for energy kind EK (data regression: d <= 128, at most 8 tiles per workgroup)
template <int EK>
using GeneralGeomsOf = std::conditional_t<is_data_regression(EK), LogisticGeoms, GeneralGeoms>;

template <int EK>
int launch_ek(const TrajPlan& p, const KArgs& k, hipStream_t s) {
  // (logistic / Poisson / binomial / probit regression: the general, energy and p_accept kernels only -- no instruction-lean or small-d form)
  if constexpr (is_data_regression(EK)) {
    if (p.family != FAM_GENERAL && p.family != FAM_ENERGY && p.family != FAM_PACCEPT)
      return fail(L2HMC_ERR_UNSUPPORTED, EK == L2HMC_ENERGY_PROBIT ? "the probit-regression target runs on the general kernel only%s"
                                         : EK == L2HMC_ENERGY_BINOMIAL ? "the binomial-regression target runs on the general kernel only%s"
                                         : EK == L2HMC_ENERGY_POISSON ? "the Poisson-regression target runs on the general kernel only%s"
                                                                     : "the logistic-regression target runs on the general kernel only%s");
  }
  switch (p.family) {
    case FAM_GENERAL:
      return on_geometry(GeneralGeomsOf<EK>{}, p.DT, p.NW, "", [&](auto DT, auto NW) {
        return on_either<3, 4>(p.KH == 3, [&](auto KH) { return launch_tiles(traj_kernel<EK, DT, NW, KH>, NW, p, k, s); });
      });
    case FAM_FAST:
      if constexpr (!is_data_regression(EK)) {     // (refused above: not instantiated)
        return on_geometry(FastGeoms{}, p.DT, p.NW, "fast ", [&](auto DT, auto NW) {
          return on_either<3, 4>(p.KH == 3, [&](auto KH) { return launch_tiles(traj_fast_kernel<EK, DT, NW, KH>, NW, p, k, s); });
        });
      }
      break;
    case FAM_SMALL:
      if constexpr (EK == L2HMC_ENERGY_FUNNEL || is_data_regression(EK)) {
        return fail(L2HMC_ERR_UNSUPPORTED, "no small-d kernel for the funnel%s");
      } else {
        return on_either<3, 4>(p.KH == 3, [&](auto KH) {
          return p.f16 ? launch_tiles(traj_small_kernel<EK, KH, 1>, 1, p, k, s) : launch_tiles(traj_small_kernel<EK, KH>, 1, p, k, s);
        });
      }
    case FAM_ENERGY:
      return on_geometry(GeneralGeomsOf<EK>{}, p.DT, p.NW, "", [&](auto DT, auto NW) { return launch_tiles(energy_kernel<EK, DT, NW>, NW, p, k, s); });
    case FAM_PACCEPT:
      return on_geometry(GeneralGeomsOf<EK>{}, p.DT, p.NW, "", [&](auto DT, auto NW) { return launch_tiles(paccept_kernel<EK, DT, NW>, NW, p, k, s); });
  }
  return fail(L2HMC_ERR_UNSUPPORTED, "no kernel for this plan%s");
}

template <int EK>
int launch_fast16_ek(const TrajPlan& p, const KArgs& k, hipStream_t s) {
  return on_geometry(FastGeoms{}, p.DT, p.NW, "fast ", [&](auto DT, auto NW) {
    return on_either<3, 4>(p.KH == 3, [&](auto KH) { return launch_tiles(traj_fast_kernel<EK, DT, NW, KH, 1>, NW, p, k, s); });
  });
}

template <int EK>
int launch_ladder_ek(const TrajPlan& p, const KArgs& k, const LadArgs& l, hipStream_t s) {
  return on_geometry(GeneralGeomsOf<EK>{}, p.DT, p.NW, "", [&](auto DT, auto NW) {
    return on_either<3, 4>(p.KH == 3, [&](auto KH) { return launch_tiles(traj_ladder_kernel<EK, DT, NW, KH>, NW, p, k, s, l); });
  });
}

// one wave per 16-chain tile, p.tpw tiles per workgroup
template <int EK>
int launch_tile_ek(const TrajPlan& p, const KArgs& k, hipStream_t s) {
  return on_either<3, 4>(p.DT == 3, [&](auto DT) {
    return on_either<3, 4>(p.KH == 3, [&](auto KH) {
      return on_either<8, 4>(p.tpw == 8, [&](auto TPW) {
        return on_either<true, false>(p.half, [&](auto HALF) {
          return launch_kernel(traj_tile_kernel<EK, DT, KH, TPW, HALF>, (k.N + 16 * TPW - 1) / (16 * TPW), 64 * TPW, p.lds, s, k);
        });
      });
    });
  });
}

}  // namespace l2hmc
