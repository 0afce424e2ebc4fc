// Discrete adjoint of the fixed-grid Roche solve WITH the gradient of every patient's dosage, gfx950 (C ABI:
// include/hode_dose.h).
//
// The sweep is rk_bwd_body (../hode_rk_kernels.hpp) itself in the lane-per-patient layout (LaneMap<1>), instantiated with
// the dose hook below, which carries one more per-lane accumulator.  The dose enters the rhs in one place,
// k[3] = kel * Dose(t) - kel * Y[3] with Dose(t) = dosage * s_p(t), so with g the cotangent handed to the VJP at a stage
// evaluated at time ts
//     gdosage += g[3] * kel * s_p(ts),    s_p(t) = sum_k 1[t >= tau_k] exp(kel (tau_k - t)).
// s_p is evaluated ONCE per stage by a DoseSched whose dosage is 1; the DoseVal the rhs and its VJP take is dosage times
// that (the same product DoseSched::at forms, so the stage states are those of rk_bwd_kernel<D, 1, ...>).  A patient's lane
// stores its own gdosage: nothing crosses lanes before the per-wave fold of the parameter gradients.
#pragma once
#include "../../../include/hode_dose.h"
#include "../hode_rk_kernels.hpp"

namespace hode {

struct DoseArgs {
  RkArgs rk;                          // t, dosage, dose_times, theta, w1, b1, h, grad_h, grad_y0, partials, status, B, T, K, perturb, ppw
  float* __restrict__ grad_dosage;    // [B]
};

struct DoseLaunch {
  int method;  // HODE_METHOD_*
  int n_waves;
  bool ablate, need_th;
};

// the DoseVal of a stage with s_p(ts) beside it
struct DoseStage : DoseVal {
  float unit;
};

// rk_bwd_body's dose hook: the stage doses, the accumulator of this lane's patient and the end of the sweep
template <bool ABLATE>
struct DoseGrad {
  static constexpr bool kGrad = true;
  float* __restrict__ grad_dosage;  // [B]
  float gd = 0.f;                   // d loss / d dosage of this lane's patient

  // dosage * s_p(ts), and its kel-derivative as DoseSched::at forms it
  template <bool K1>
  HODE_DEV DoseStage at(const DoseSched<K1>& ds, float ts, float kel) const {
    DoseStage r;
    if constexpr (ABLATE) {  // the dose does not enter the rhs
      r.unit = r.v = r.dk = 0.f;
    } else {
      DoseSched<K1> us = ds;
      us.dosage = 1.0f;  // the schedule at unit dosage
      const DoseVal u = us.at(ts, kel);
      r.unit = u.v;
      r.v = ds.dosage * u.v;
      r.dk = K1 ? (ds.tau0 - ts) * r.v : ds.dosage * u.dk;
    }
    return r;
  }

  // g3: the cotangent of k[3] handed to the VJP of that stage
  HODE_DEV void tap(const DoseStage& stage, float g3, float kel) {
    if constexpr (!ABLATE) gd = __builtin_fmaf(g3, kel * stage.unit, gd);
  }

  template <int D>
  HODE_DEV void finish(const RkArgs& a, const LaneMap<1>& lm, const float (&lam)[D]) const {
    if (lm.live) grad_dosage[lm.p] = gd;  // the patient's own lane; an idle lane writes nothing
    if (a.status) {
      // x * 0 is 0 for a finite x and NaN otherwise: one comparison for the D + 1 values.  (D + 1 class tests and their
      // OR-chain here cost the D = 12 rk4 sweep 650 bytes of scratch per lane, profiles/lane_sweep_ab.txt.)
      float z = gd * 0.f;
#pragma unroll
      for (int i = 0; i < D; ++i) z = __builtin_fmaf(lam[i], 0.f, z);
      const bool bad = !(z == 0.f);
      if (bad && lm.live) atomicOr(a.status, HODE_STATUS_NONFINITE);
    }
  }
};

template <int D, int METHOD, bool ABLATE, bool NEED_TH>
__global__ __launch_bounds__(64) void dose_bwd_kernel(DoseArgs a) {
  // the Hill-2 body and the one-dose fast path, chosen at run time as rk_bwd_kernel does (wave-uniform branches)
  const bool hill2 = ABLATE || (a.rk.theta[0] == 2.0f && a.rk.theta[1] == 2.0f);
  const DoseGrad<ABLATE> dose{a.grad_dosage};
  if (hill2 && a.rk.K == 1) rk_bwd_body<D, 1, METHOD, ABLATE, true, NEED_TH, true>(a.rk, dose);
  else if (hill2) rk_bwd_body<D, 1, METHOD, ABLATE, true, NEED_TH, false>(a.rk, dose);
  else rk_bwd_body<D, 1, METHOD, ABLATE, false, NEED_TH, false>(a.rk, dose);
}

template <int D, int METHOD>
hipError_t dose_launch_method(const DoseLaunch& L, const DoseArgs& a, hipStream_t s) {
  const dim3 grid(L.n_waves), block(64);
  if (L.ablate) {
    if (L.need_th) hipLaunchKernelGGL((dose_bwd_kernel<D, METHOD, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dose_bwd_kernel<D, METHOD, true, false>), grid, block, 0, s, a);
  } else {
    if (L.need_th) hipLaunchKernelGGL((dose_bwd_kernel<D, METHOD, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dose_bwd_kernel<D, METHOD, false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

// one launch of the sweep for latent size D; the caller turns the hipError_t into the library's message
template <int D>
hipError_t dose_launch(const DoseLaunch& L, const DoseArgs& a, hipStream_t s) {
  switch (L.method) {
    case HODE_METHOD_EULER: return dose_launch_method<D, HODE_METHOD_EULER>(L, a, s);
    case HODE_METHOD_MIDPOINT: return dose_launch_method<D, HODE_METHOD_MIDPOINT>(L, a, s);
    case HODE_METHOD_RK4_38: return dose_launch_method<D, HODE_METHOD_RK4_38>(L, a, s);
  }
  return hipErrorInvalidValue;
}

// one entry per compiled latent size (hode_dose_dim.hip, -DHODE_DIM=<D>)
hipError_t dose_launch_d4(const DoseLaunch&, const DoseArgs&, hipStream_t);
hipError_t dose_launch_d6(const DoseLaunch&, const DoseArgs&, hipStream_t);
hipError_t dose_launch_d8(const DoseLaunch&, const DoseArgs&, hipStream_t);
hipError_t dose_launch_d12(const DoseLaunch&, const DoseArgs&, hipStream_t);

}  // namespace hode
