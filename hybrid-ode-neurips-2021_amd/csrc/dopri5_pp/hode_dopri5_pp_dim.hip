// Instantiates the per-patient dopri5 kernels for ONE latent size (-DHODE_DIM=<D>), like ../hode_dopri5_dim.hip.
#include "hode_dopri5_pp_kernels.hpp"

#ifndef HODE_DIM
#error "compile with -DHODE_DIM=<latent dim>"
#endif

namespace hode {
hipError_t HODE_CAT(pp_launch_d, HODE_DIM)(const PpLaunch& L, const PpArgs& a, hipStream_t s) {
  return pp_launch<HODE_DIM>(L, a, s);
}
}  // namespace hode
