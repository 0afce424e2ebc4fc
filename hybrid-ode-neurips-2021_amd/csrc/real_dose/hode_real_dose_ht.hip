// The kernels of libhode_real_dose.so at one hidden-tile count HT = HODE_REAL_DOSE_HT (hidden_dim <= 16 HT): the discrete
// adjoint of the chained fixed-grid solve of the real-data hybrid rhs that also gives d loss / d act of the dose table.
// The rhs, its VJP, the stages of a solver step, the cotangent chain, the gradient accumulator and its fold are
// ../hode_real_mf.hpp with the ragged tile (M = latent_dim - 4 at run time), the code libhode.so and libhode_real_dims.so
// run; what is here is the reverse time loop of real_mf_body's on-chip backward with one more thing in it: the tap of the
// dose cotangent in the VJP callback and the reverse scan over the action rows, fused into the sweep.
#include <hip/hip_runtime.h>

#include "../hode_real_mf.hpp"
#include "hode_real_dose.hpp"

#ifndef HODE_REAL_DOSE_HT
#error "compile with -DHODE_REAL_DOSE_HT=<1 .. 4>"
#endif

namespace hode {

constexpr int kHT = HODE_REAL_DOSE_HT;
static_assert(kHT >= 1 && kHT <= 4, "hidden tiles");
static_assert(RealGradAcc<kHT>::NP == real_dose_partial_floats(kHT), "partial block size");

// a.h / a.grad_h [T][B][D], a.grad_y0 [B][D], grad_act [Ta][B]; a.y0 is not read (h[0] is the start state).
// Dose(ts) = exp(kel (n - ts)) S_n, n = min(Ta, floor(ts)), S_n = act[n-1] + E S_{n-1}: a stage at ts with cotangent gX adds
// gX[3] kel exp(kel (n - ts)) to the cotangent of S_n, and grad_act[n-1] = S^_n, S^_{n-1} += E S^_n.  The sweep meets the
// stage times in non-increasing order (steps last to first, stages last to first inside a step, the grid increasing), so
// the lane g == 0 of a patient keeps (n_cur, R): R is the cotangent of S_{n_cur} so far, and a tap at n < n_cur first
// writes the rows n_cur - 1 .. n out.  Every element of grad_act is written once, by its own patient's lane; lanes of
// patients >= B read patient B - 1 and store nothing.
template <int HT, int METHOD>
HODE_DEV void real_dose_body(const RealArgs& a, const RealTileRagged tile, float* __restrict__ grad_act, float* lds) {
  typedef RealMf<HT, RealTileRagged> Net;
  typedef typename Net::Stage Stage;
  constexpr int NT2 = 2 * HT;
  constexpr int NS = real_stages(METHOD);
  const int M = tile.m(), D = M + 4;
  const int lane = threadIdx.x;
  Net nn;
  nn.load(a, tile, lane);
  const int g = nn.g;
  const bool g0 = g == 0;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const size_t B = a.B;
  const size_t row = B * D;
  const size_t po = (size_t)p * D;
  RealGradAcc<HT> acc;
  acc.init(lds);
  if (g0) real_dose_table(a, p, nn.kel);  // each lane reads back only its own column
  auto set_dose = [&](Stage& s, float t) { real_set_dose(a, p, nn.kel, g0, s, t); };

  const bool owner = g0 && live;  // the lane that writes this patient's column of grad_act
  const float E = exp_f32(-nn.kel);
  int n_cur = a.Ta;
  float R = 0.f;
  auto flush_to = [&](int n) {  // rows n_cur - 1 .. n of this patient's column; at most Ta iterations per launch
    while (n_cur > n) {
      grad_act[(size_t)(n_cur - 1) * B + p] = R;
      R *= E;
      --n_cur;
    }
  };

  const float lv = live ? 1.0f : 0.0f;
  float dth[3] = {0.f, 0.f, 0.f};
  v4 lamX, lamH;
  real_load_state(tile, g, a.grad_h + (size_t)(a.T - 1) * row + po, lamX, lamH);
  lamX = lv * lamX; lamH = lv * lamH;
  for (int n = a.T - 2; n >= 0; --n) {
    const RStageTimes st(a.t, n, a.perturb, METHOD);
    v4 X, Hs;
    real_load_state(tile, g, a.h + (size_t)n * row + po, X, Hs);
    Stage s[NS];
    v4 kH[NS];
    HODE_REAL_STEP_STAGES(METHOD, nn, s, kH, st, X, Hs, set_dose)
    auto vjp = [&](int q, const v4& gX, const v4& gH, v4& aX, v4& aH) {
      v4 U1[NT2], ur, uz, uh;
      float u12, u22;
      nn.vjp(s[q], gX, gH, aX, aH, U1, u12, u22, ur, uz, uh, dth);
      acc.add(U1, s[q].ah, s[q].X, u12, u22, uh, uz, ur, s[q].RH, s[q].Hs, g, nn.n);
      if (owner) {  // the tap: the stage times of HODE_REAL_STEP_STAGES
        const float ts = q == 0 ? st.t_first : (q == 1 ? st.ta : (q == 2 ? st.tb : st.t_last));
        const int nd = min(a.Ta, (int)__builtin_floorf(ts));
        if (nd >= 1) {
          flush_to(nd);
          R = __builtin_fmaf(gX[3] * nn.kel, exp_f32(nn.kel * ((float)nd - ts)), R);
        }
      }
    };
    HODE_REAL_STEP_CHAIN(METHOD, st.dt, lamX, lamH, vjp)
    v4 ghX, ghH;
    real_load_state(tile, g, a.grad_h + (size_t)n * row + po, ghX, ghH);
    lamX = lamX + lv * ghX; lamH = lamH + lv * ghH;
  }
  if (owner) flush_to(0);
  if (live) real_store_state(tile, g, a.grad_y0 + po, lamX, lamH);
  // only lanes g == 0 of live patients carry scalar-gradient terms (X, gX are zero elsewhere; lv zeroes dead patients)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float v = wave_sum(g0 ? dth[j] : 0.f);
    if (lane == 0) a.partials[(size_t)blockIdx.x * 3 + j] = v;
  }
  acc.store(a.tape + (size_t)blockIdx.x * RealGradAcc<HT>::NP, lane);
}

template <int HT, int METHOD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_dose_bwd_kernel(RealArgs a, int M,
                                                                                                       float* __restrict__ grad_act) {
  __shared__ __attribute__((aligned(16))) float lds[RealGradAcc<HT>::kLdsFloats];
  real_dose_body<HT, METHOD>(a, RealTileRagged{M}, grad_act, lds);
}

// the three M x M blocks are written with M as row stride; padded rows and columns of the tiles are never written
template <int HT>
__global__ __launch_bounds__(64) void real_dose_fold_kernel(const float* __restrict__ partials, int n_waves, int H, int M,
                                                            float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, M, gw);
}

#define HODE_REAL_DOSE_CAT2(a, b) a##b
#define HODE_REAL_DOSE_CAT(a, b) HODE_REAL_DOSE_CAT2(a, b)
int HODE_REAL_DOSE_CAT(real_dose_launch_ht, HODE_REAL_DOSE_HT)(int method, const RealArgs& a, int M, float* grad_act, float* grad_w,
                                                               hipStream_t s) {
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
