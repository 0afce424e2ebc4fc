// Internal to libhode_real_step.so: what the per-hidden-tile units (hode_real_step_ht.hip, compiled once per
// -DHODE_REAL_STEP_HT=<1 .. 4>, the HODE_REAL_SIDE_HTS of ../hode_real_side_host.hpp) give the entry points
// (hode_real_step.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../../include/hode_real_step.h"
#include "../hode_real_side_host.hpp"

namespace hode {

// the domain: latent sizes (M = latent_dim - 4 = 1 .. 16 GRU states in ONE 16-row tile), hidden sizes (1 .. 4 tiles) and
// solver steps per interval
constexpr int kRealStepMinLatent = 5, kRealStepMaxLatent = 20, kRealStepMaxHidden = 64, kRealStepMaxSub = 8;
#define HODE_REAL_STEP_TEXT "latent_dim 5 .. 20 with hidden_dim 1 .. 64 and 1 .. 8 solver steps per interval"

// the launch rule's two numbers: the card's SIMDs (one wave each: the kernels are compiled for one wave per SIMD) and the
// fixed cost of a wave in units of one interval's work (DESIGN.md 4.6c holds the measurement behind the number)
constexpr long kRealStepSimds = 1024, kRealStepWaveCost = 2;

// how the N intervals are cut into runs: wave (x, y) owns patients 16 x .. 16 x + 15 and the intervals y C .. y C + C - 1
struct RealStepGeom {
  int N, S, C;
  float* sub;  // backward: [N][S - 1][B][D], the states at the start of the sub-steps 1 .. S - 1 of every interval
};

// Launch real_step_kernel<HT, method, bwd> over ceil(B / 16) x ceil(N / C) waves and, after a backward,
// real_step_fold_kernel<HT> into the flat weight gradient `grad_w`.  `M` = latent_dim - 4.  One definition per unit.
#define HODE_REAL_STEP_DECL(n) \
  int real_step_launch_ht##n(int method, bool bwd, const RealArgs& a, const RealStepGeom& geo, int M, float* grad_w, hipStream_t s);
HODE_REAL_SIDE_HTS(HODE_REAL_STEP_DECL)
#undef HODE_REAL_STEP_DECL

}  // namespace hode
