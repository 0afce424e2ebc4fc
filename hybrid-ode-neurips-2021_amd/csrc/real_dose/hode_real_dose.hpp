// Internal to libhode_real_dose.so: what the per-hidden-tile units (hode_real_dose_ht.hip, compiled once per
// -DHODE_REAL_DOSE_HT=<1 .. 4>, the HODE_REAL_SIDE_HTS of ../hode_real_side_host.hpp) give the entry points
// (hode_real_dose.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../../include/hode_real_dose.h"
#include "../hode_real_side_host.hpp"

namespace hode {

// the domain: latent sizes (M = latent_dim - 4 = 1 .. 16 GRU states in ONE 16-row tile) and hidden sizes (1 .. 4 tiles)
constexpr int kRealDoseMinLatent = 5, kRealDoseMaxLatent = 20, kRealDoseMaxHidden = 64;
#define HODE_REAL_DOSE_TEXT "latent_dim 5 .. 20 with hidden_dim 1 .. 64, methods euler / midpoint / rk4"

// Launch real_dose_bwd_kernel<HT, method> over ceil(B / 16) waves and real_dose_fold_kernel<HT> into the flat weight
// gradient `grad_w`.  `M` = latent_dim - 4; `grad_act` is the [Ta][B] output.  One definition per unit.
#define HODE_REAL_DOSE_DECL(n) \
  int real_dose_launch_ht##n(int method, const RealArgs& a, int M, float* grad_act, float* grad_w, hipStream_t s);
HODE_REAL_SIDE_HTS(HODE_REAL_DOSE_DECL)
#undef HODE_REAL_DOSE_DECL

}  // namespace hode
