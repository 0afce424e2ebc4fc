// Internal to libhode_real_pp.so: what the per-hidden-tile units (hode_real_pp_ht.hip, compiled once per
// -DHODE_REAL_PP_HT=<1 .. 4>, the HODE_REAL_SIDE_HTS of ../hode_real_side_host.hpp) give the entry points
// (hode_real_pp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../../include/hode_real_pp.h"
#include "../hode_real_side_host.hpp"

namespace hode {

// the domain: latent sizes (M = latent_dim - 4 = 1 .. 16 GRU states in ONE 16-row tile) and hidden sizes (1 .. 4 tiles)
constexpr int kRealPpMinLatent = 5, kRealPpMaxLatent = 20, kRealPpMaxHidden = 64;
#define HODE_REAL_PP_TEXT "latent_dim 5 .. 20 with hidden_dim 1 .. 64, dopri5 with per-patient step control"

// the kernels' arguments: those of the fixed-grid kernels (r.tape holds the per-wave weight-gradient blocks of the sweep)
// and the controller's
struct RealPpArgs {
  RealArgs r;
  int* status;                // [1] OR of all patients
  int* __restrict__ n_acc;    // [B]
  int* __restrict__ n_rej;    // [B]
  int* __restrict__ pstatus;  // [B]
  double* tape_t;             // [max_steps][B]
  double* tape_dt;            // [max_steps][B]: the clipped length
  int* tape_j;                // [max_steps][B]: the output index the step reached, or -1
  float* tape_y;              // [max_steps][B][D]: the state at the START of the step
  int max_steps, max_attempts, no_tape;
  float rtol, atol;
};

// Forward: real_pp_fwd_kernel<HT> over ceil(B / 16) waves.  Backward: real_pp_bwd_kernel<HT> over the same waves and
// real_pp_fold_kernel<HT> into the flat weight gradient `grad_w`.  `M` = latent_dim - 4.  One definition per unit.
#define HODE_REAL_PP_DECL(n) int real_pp_launch_ht##n(bool bwd, const RealPpArgs& a, int M, float* grad_w, hipStream_t s);
HODE_REAL_SIDE_HTS(HODE_REAL_PP_DECL)
#undef HODE_REAL_PP_DECL

}  // namespace hode
