// libhode_roche_dims.so, one latent size (-DHODE_DIM=<D>): the dopri5 kernels of ../hode_dopri5_kernels.hpp as dp_dispatch
// instantiates them -- the owner layout at 16, one patient per lane at every other size.
#include "../hode_dopri5_kernels.hpp"
#include "hode_roche_dims.hpp"

#ifndef HODE_DIM
#error "compile with -DHODE_DIM=<latent dim>"
#endif

namespace hode {
int HODE_CAT(roche_dims_dp_dispatch_d, HODE_DIM)(const DpLaunch& L, const DpArgs& a, hipStream_t s) {
  return dp_dispatch<HODE_DIM>(L, a, s);
}
}  // namespace hode
