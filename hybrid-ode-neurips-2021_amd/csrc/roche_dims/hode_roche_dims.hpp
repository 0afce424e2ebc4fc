// Internal to libhode_roche_dims.so: what the per-size units (hode_roche_dims_rk_dim.hip, hode_roche_dims_dp_dim.hip, each
// compiled once per -DHODE_DIM=<D>) give the entry points (hode_roche_dims.hip, and ../hode_dopri5.hip compiled with
// -DHODE_ROCHE_DIMS_UNIT).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/hode_roche_dims.h"
#include "../hode_host.hpp"

namespace hode {

// the latent sizes of the hybrid decoder that libhode.so does not hold, up to 16
#define HODE_ROCHE_DIMS(X) X(5) X(7) X(9) X(10) X(11) X(13) X(14) X(15) X(16)
#define HODE_ROCHE_DIMS_TEXT "5, 7, 9, 10, 11, 13, 14, 15, 16"

#define HODE_ROCHE_DIMS_DECL(n)                                                  \
  int roche_dims_rk_dispatch_d##n(const RkLaunch&, const RkArgs&, hipStream_t); \
  int roche_dims_dp_dispatch_d##n(const DpLaunch&, const DpArgs&, hipStream_t);
HODE_ROCHE_DIMS(HODE_ROCHE_DIMS_DECL)
#undef HODE_ROCHE_DIMS_DECL

// What every entry checks first: the descriptor itself, the rhs kind, the size and lanes_per_patient.  A refusal names the
// sizes of both libraries.  (hode_roche_dims.hip)
int roche_dims_check_domain(const hode_solve_desc* d);
// the dopri5 workspace (../hode_dopri5.hip)
size_t roche_dims_dopri5_workspace_bytes(const hode_solve_desc* d);

}  // namespace hode
