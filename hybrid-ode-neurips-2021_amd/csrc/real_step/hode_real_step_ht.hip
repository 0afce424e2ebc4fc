// The kernels of libhode_real_step.so at one hidden-tile count HT = HODE_REAL_STEP_HT (hidden_dim <= 16 HT): the one-step-
// ahead solve of the real-data hybrid rhs.  N independent intervals per patient, each from a start state of its own over S
// solver steps; a wave owns 16 patients x a run of C consecutive intervals, loads the weights once and walks its run.  The
// rhs, its VJP, the stage arithmetic of a solver step, the gradient accumulator and its fold are ../hode_real_mf.hpp with
// the ragged tile (M = latent_dim - 4 at run time), the code libhode.so and libhode_real_dims.so run for the chained
// solve; what is here is the walk over intervals.  The dose table is read only: real_step_dose_kernel
// (hode_real_step.hip) wrote it before this launch.
#include <hip/hip_runtime.h>

#include "../hode_real_mf.hpp"
#include "hode_real_step.hpp"

#ifndef HODE_REAL_STEP_HT
#error "compile with -DHODE_REAL_STEP_HT=<1 .. 4>"
#endif

namespace hode {

constexpr int kHT = HODE_REAL_STEP_HT;
static_assert(kHT >= 1 && kHT <= 4, "hidden tiles");
static_assert(RealGradAcc<kHT>::NP == real_side_partial_floats(kHT), "partial block size");

// a.y0 [N][B][D] start states, a.t [N][S + 1], a.h / a.grad_h [N + 1][B][D], a.grad_y0 [N][B][D]; a.T is not read.
// Every load and store of a state row is element-wise and guarded (real_load_state / real_store_state of the ragged
// tile); lanes of patients >= B read patient B - 1 and store nothing.
template <int HT, int METHOD, bool BWD>
HODE_DEV void real_step_body(const RealArgs& a, const RealStepGeom geo, const RealTileRagged tile, float* lds) {
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
  const int S = geo.S;
  const int i0 = blockIdx.y * geo.C;
  const int i1 = min(geo.N, i0 + geo.C);
  auto set_dose = [&](Stage& s, float t) { real_set_dose(a, p, nn.kel, g0, s, t); };

  if constexpr (!BWD) {
    if (blockIdx.y == 0 && live) {  // the padding row h[0]
      const v4 z = v4{0.f, 0.f, 0.f, 0.f};
      real_store_state(tile, g, a.h + po, z, z);
    }
    v4 X, Hs;
    real_load_state(tile, g, a.y0 + (size_t)i0 * row + po, X, Hs);
    Stage s;
    for (int i = i0; i < i1; ++i) {
      v4 nX, nH;  // the next interval's start state is on its way while this one is integrated
      real_load_state(tile, g, a.y0 + (size_t)(i + 1 < i1 ? i + 1 : i) * row + po, nX, nH);
      const float* tg = a.t + (size_t)i * (S + 1);
      for (int k = 0; k < S; ++k) {
        const RStageTimes st(tg, k, a.perturb, METHOD);
        real_step_fwd<METHOD>(nn, s, st, X, Hs, set_dose);
      }
      if (live) real_store_state(tile, g, a.h + (size_t)(i + 1) * row + po, X, Hs);
      X = nX; Hs = nH;
    }
  } else {
    RealGradAcc<HT> acc;
    acc.init(lds);
    const float lv = live ? 1.0f : 0.0f;
    float dth[3] = {0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
      const float* tg = a.t + (size_t)i * (S + 1);
      float* sub = geo.sub + (size_t)i * (S - 1) * row + po;  // this patient's sub-step states of interval i
      v4 lamX, lamH, X, Hs;
      real_load_state(tile, g, a.grad_h + (size_t)(i + 1) * row + po, lamX, lamH);
      real_load_state(tile, g, a.y0 + (size_t)i * row + po, X, Hs);
      lamX = lv * lamX; lamH = lv * lamH;
      {
        Stage s;
        for (int k = 0; k + 1 < S; ++k) {  // S > 1: the states the steps 1 .. S - 1 start from, written and read back by the same lanes
          const RStageTimes st(tg, k, a.perturb, METHOD);
          real_step_fwd<METHOD>(nn, s, st, X, Hs, set_dose);
          if (live) real_store_state(tile, g, sub + (size_t)k * row, X, Hs);
        }
      }
      for (int k = S - 1; k >= 0; --k) {
        const RStageTimes st(tg, k, a.perturb, METHOD);
        if (k + 1 < S) real_load_state(tile, g, k > 0 ? sub + (size_t)(k - 1) * row : a.y0 + (size_t)i * row + po, X, Hs);
        Stage s[NS];
        v4 kH[NS];
        HODE_REAL_STEP_STAGES(METHOD, nn, s, kH, st, X, Hs, set_dose)
        auto vjp = [&](int q, const v4& gX, const v4& gH, v4& aX, v4& aH) {
          v4 U1[NT2], ur, uz, uh;
          float u12, u22;
          nn.vjp(s[q], gX, gH, aX, aH, U1, u12, u22, ur, uz, uh, dth);
          acc.add(U1, s[q].ah, s[q].X, u12, u22, uh, uz, ur, s[q].RH, s[q].Hs, g, nn.n);
        };
        HODE_REAL_STEP_CHAIN(METHOD, st.dt, lamX, lamH, vjp)
      }
      if (live) real_store_state(tile, g, a.grad_y0 + (size_t)i * row + po, lamX, lamH);
    }
    // only lanes g == 0 of live patients carry scalar-gradient terms (X, gX are zero elsewhere; lv zeroes dead patients)
    const size_t wave = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = wave_sum(g0 ? dth[j] : 0.f);
      if (lane == 0) a.partials[wave * 3 + j] = v;
    }
    acc.store(a.tape + wave * RealGradAcc<HT>::NP, lane);
  }
}

template <int HT, int METHOD, bool BWD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_step_kernel(RealArgs a, RealStepGeom geo, int M) {
  __shared__ __attribute__((aligned(16))) float lds[BWD ? RealGradAcc<HT>::kLdsFloats : 4];
  real_step_body<HT, METHOD, BWD>(a, geo, RealTileRagged{M}, lds);
}

// the three M x M blocks are written with M as row stride; padded rows and columns of the tiles are never written
template <int HT>
__global__ __launch_bounds__(64) void real_step_fold_kernel(const float* __restrict__ partials, int n_waves, int H, int M,
                                                            float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, M, gw);
}

template <int METHOD>
static void launch_method(bool bwd, const RealArgs& a, const RealStepGeom& geo, int M, dim3 grid, hipStream_t s) {
  if (bwd) hipLaunchKernelGGL((real_step_kernel<kHT, METHOD, true>), grid, dim3(64), 0, s, a, geo, M);
  else hipLaunchKernelGGL((real_step_kernel<kHT, METHOD, false>), grid, dim3(64), 0, s, a, geo, M);
}

int HODE_CAT(real_step_launch_ht, HODE_REAL_STEP_HT)(int method, bool bwd, const RealArgs& a, const RealStepGeom& geo, int M,
                                                    float* grad_w, hipStream_t s) {
  const dim3 grid((a.B + 15) / 16, (geo.N + geo.C - 1) / geo.C);
  switch (method) {
    case HODE_METHOD_EULER: launch_method<HODE_METHOD_EULER>(bwd, a, geo, M, grid, s); break;
    case HODE_METHOD_MIDPOINT: launch_method<HODE_METHOD_MIDPOINT>(bwd, a, geo, M, grid, s); break;
    default: launch_method<HODE_METHOD_RK4_38>(bwd, a, geo, M, grid, s); break;
  }
  if (bwd)
    hipLaunchKernelGGL((real_step_fold_kernel<kHT>), dim3(RealGradAcc<kHT>::NP), dim3(64), 0, s, a.tape, (int)(grid.x * grid.y), a.H,
                       M, grad_w);
  return hip_fail(hipGetLastError(), "real step kernel launch");
}

}  // namespace hode
