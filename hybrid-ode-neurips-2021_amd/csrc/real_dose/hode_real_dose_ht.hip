// The kernels of libhode_real_dose.so at one hidden-tile count HT = HODE_REAL_DOSE_HT (hidden_dim <= 16 HT): the discrete
// adjoint of the chained fixed-grid solve of the real-data hybrid rhs that also gives d loss / d act of the dose table.
// The sweep is real_mf_body's on-chip backward (../hode_real_mf.hpp with the ragged tile, M = latent_dim - 4 at run time),
// the code libhode.so and libhode_real_dims.so run; what is here is its dose hook: the tap of the dose cotangent after a
// stage's VJP and the reverse scan over the action rows, fused into the sweep.
#include <hip/hip_runtime.h>

#include "../hode_real_mf.hpp"
#include "hode_real_dose.hpp"

#ifndef HODE_REAL_DOSE_HT
#error "compile with -DHODE_REAL_DOSE_HT=<1 .. 4>"
#endif

namespace hode {

constexpr int kHT = HODE_REAL_DOSE_HT;
static_assert(kHT >= 1 && kHT <= 4, "hidden tiles");
static_assert(RealGradAcc<kHT>::NP == real_side_partial_floats(kHT), "partial block size");

// a.h / a.grad_h [T][B][D], a.grad_y0 [B][D], grad_act [Ta][B]; a.y0 is not read (h[0] is the start state).
// Dose(ts) = exp(kel (n - ts)) S_n, n = min(Ta, floor(ts)), S_n = act[n-1] + E S_{n-1}: a stage at ts with cotangent gX adds
// gX[3] kel exp(kel (n - ts)) to the cotangent of S_n, and grad_act[n-1] = S^_n, S^_{n-1} += E S^_n.  The sweep meets the
// stage times in non-increasing order (steps last to first, stages last to first inside a step, the grid increasing), so
// the lane g == 0 of a patient keeps (n_cur, R): R is the cotangent of S_{n_cur} so far, and a tap at n < n_cur first
// writes the rows n_cur - 1 .. n out.  Every element of grad_act is written once, by its own patient's lane; lanes of
// patients >= B read patient B - 1 and store nothing.
struct RealDoseGrad {
  static constexpr bool kGrad = true;
  float* __restrict__ grad_act;
  size_t B;
  int Ta, p, n_cur;
  bool owner;  // the lane that writes this patient's column of grad_act
  float kel, E, R;
  HODE_DEV void begin(const RealArgs& a, int patient, bool owns, float k) {
    B = a.B; Ta = a.Ta; p = patient; owner = owns; kel = k;
    E = exp_f32(-kel);
    n_cur = Ta;
    R = 0.f;
  }
  HODE_DEV void flush_to(int n) {  // rows n_cur - 1 .. n of this patient's column; at most Ta iterations per launch
    while (n_cur > n) {
      grad_act[(size_t)(n_cur - 1) * B + p] = R;
      R *= E;
      --n_cur;
    }
  }
  HODE_DEV void tap(const RStageTimes& st, int q, float gX3) {  // the stage times of HODE_REAL_STEP_STAGES
    if (!owner) return;
    const float ts = q == 0 ? st.t_first : (q == 1 ? st.ta : (q == 2 ? st.tb : st.t_last));
    const int nd = min(Ta, (int)__builtin_floorf(ts));
    if (nd >= 1) {
      flush_to(nd);
      R = __builtin_fmaf(gX3 * kel, exp_f32(kel * ((float)nd - ts)), R);
    }
  }
  HODE_DEV void finish() {
    if (owner) flush_to(0);
  }
};

template <int HT, int METHOD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_dose_bwd_kernel(RealArgs a, int M,
                                                                                                       float* __restrict__ grad_act) {
  __shared__ __attribute__((aligned(16))) float lds[RealGradAcc<HT>::kLdsFloats];
  real_mf_body<HT, METHOD, true, true>(a, RealTileRagged{M}, lds, RealDoseGrad{grad_act});
}

// the three M x M blocks are written with M as row stride; padded rows and columns of the tiles are never written
template <int HT>
__global__ __launch_bounds__(64) void real_dose_fold_kernel(const float* __restrict__ partials, int n_waves, int H, int M,
                                                            float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, M, gw);
}

int HODE_CAT(real_dose_launch_ht, HODE_REAL_DOSE_HT)(int method, const RealArgs& a, int M, float* grad_act, float* grad_w, hipStream_t s) {
  const dim3 grid((a.B + 15) / 16);
  switch (method) {
    case HODE_METHOD_EULER:
      hipLaunchKernelGGL((real_dose_bwd_kernel<kHT, HODE_METHOD_EULER>), grid, dim3(64), 0, s, a, M, grad_act);
      break;
    case HODE_METHOD_MIDPOINT:
      hipLaunchKernelGGL((real_dose_bwd_kernel<kHT, HODE_METHOD_MIDPOINT>), grid, dim3(64), 0, s, a, M, grad_act);
      break;
    default:
      hipLaunchKernelGGL((real_dose_bwd_kernel<kHT, HODE_METHOD_RK4_38>), grid, dim3(64), 0, s, a, M, grad_act);
      break;
  }
  hipLaunchKernelGGL((real_dose_fold_kernel<kHT>), dim3(RealGradAcc<kHT>::NP), dim3(64), 0, s, a.tape, (int)grid.x, a.H, M, grad_w);
  return hip_fail(hipGetLastError(), "real dose kernel launch");
}

}  // namespace hode
