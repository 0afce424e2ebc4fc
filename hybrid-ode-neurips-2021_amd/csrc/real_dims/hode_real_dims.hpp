// Internal to libhode_real_dims.so: what the per-hidden-tile units (hode_real_dims_ht.hip, compiled once per
// -DHODE_REAL_DIMS_HT=<1 .. 4>, the HODE_REAL_SIDE_HTS of ../hode_real_side_host.hpp) give the entry points
// (hode_real_dims.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../../include/hode_real_dims.h"
#include "../hode_real_side_host.hpp"

namespace hode {

// the domain: latent sizes (M = latent_dim - 4 = 1 .. 16 GRU states in ONE 16-row tile) and hidden sizes (1 .. 4 tiles)
constexpr int kRealDimsMinLatent = 5, kRealDimsMaxLatent = 20, kRealDimsMaxHidden = 64;
#define HODE_REAL_DIMS_TEXT "latent_dim 5 .. 20 with hidden_dim 1 .. 64"
#define HODE_REAL_DIMS_LIBHODE_TEXT "libhode.so has latent_dim 4 and 20"

// Launch real_dims_kernel<HT, method, bwd> over ceil(B / 16) waves and, after a backward, real_dims_fold_kernel<HT> into
// the flat weight gradient `grad_w`.  `M` = latent_dim - 4.  One definition per unit.
#define HODE_REAL_DIMS_DECL(n) \
  int real_dims_launch_ht##n(int method, bool bwd, const RealArgs& a, int M, float* grad_w, hipStream_t s);
HODE_REAL_SIDE_HTS(HODE_REAL_DIMS_DECL)
#undef HODE_REAL_DIMS_DECL

}  // namespace hode
