// Instantiates the dose-gradient adjoint kernels for ONE latent size (-DHODE_DIM=<D>), like ../dopri5_pp/hode_dopri5_pp_dim.hip.
#include "hode_dose_kernels.hpp"

#ifndef HODE_DIM
#error "compile with -DHODE_DIM=<latent dim>"
#endif

namespace hode {
hipError_t HODE_CAT(dose_launch_d, HODE_DIM)(const DoseLaunch& L, const DoseArgs& a, hipStream_t s) {
  return dose_launch<HODE_DIM>(L, a, s);
}
}  // namespace hode
