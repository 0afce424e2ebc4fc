// libhode_roche_dims.so, one latent size (-DHODE_DIM=<D>): the fixed-grid Roche kernels of ../hode_rk_kernels.hpp with one
// patient per lane and with a patient per quad -- the ragged quad layout (../hode_roche.hpp) where (D - 4) % 4 != 0, the
// regular one at 16.
#include "../hode_rk_kernels.hpp"
#include "hode_roche_dims.hpp"

#ifndef HODE_DIM
#error "compile with -DHODE_DIM=<latent dim>"
#endif

namespace hode {
int HODE_CAT(roche_dims_rk_dispatch_d, HODE_DIM)(const RkLaunch& L, const RkArgs& a, hipStream_t s) {
  return dispatch_lpp_ragged<HODE_DIM>(L, a, s);
}
}  // namespace hode
