// Discrete adjoint of the fixed-grid Roche solve WITH the gradient of every patient's dosage, gfx950 (C ABI:
// include/hode_dose.h).
//
// The sweep is rk_bwd_body's (../hode_rk_kernels.hpp) in the lane-per-patient layout (LaneMap<1>): stages recomputed from
// h[n], no tape, the same stage algebra in the same order.  It carries one more per-lane accumulator.  The dose enters the
// rhs in one place, k[3] = kel * Dose(t) - kel * Y[3] with Dose(t) = dosage * s_p(t), so with g the cotangent handed to
// roche_vjp at a stage evaluated at time ts
//     gdosage += g[3] * kel * s_p(ts),    s_p(t) = sum_k 1[t >= tau_k] exp(kel (tau_k - t)).
// s_p is evaluated ONCE per stage by a DoseSched whose dosage is 1; the DoseVal the rhs and its VJP take is dosage times
// that (the same product DoseSched::at forms, so the stage states are those of rk_bwd_kernel<D, 1, ...>).  A patient's lane
// stores its own gdosage: nothing crosses lanes before the per-wave fold of the parameter gradients.
//
// The rhs, its VJP, the dose schedule, the stage times, the lane map, the vector loads and the partial row are those
// headers' own code, compiled here.
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

// s_p(ts) and the DoseVal of the stage: dosage * s_p, and its kel-derivative as DoseSched::at forms it
template <bool ABLATE, bool K1>
struct DoseStage {
  float unit;  // s_p(ts)
  DoseVal val;
  HODE_DEV DoseStage(const DoseSched<K1>& us, float dosage, float ts, float kel) {
    if constexpr (ABLATE) {  // the dose does not enter the rhs
      unit = 0.f;
      val.v = 0.f;
      val.dk = 0.f;
    } else {
      const DoseVal u = us.at(ts, kel);
      unit = u.v;
      val.v = dosage * u.v;
      val.dk = K1 ? (us.tau0 - ts) * val.v : dosage * u.dk;
    }
  }
};

template <int D, int METHOD, bool ABLATE, bool HILL2, bool NEED_TH, bool K1>
HODE_DEV void dose_bwd_body(const DoseArgs& da) {
  const RkArgs& a = da.rk;
  using Ml = MlSlice<D, 1>;
  using Stage = DoseStage<ABLATE, K1>;
  constexpr int MR = Ml::MR;
  constexpr int M = D - 4;
  const LaneMap<1> lm(a.B, a.ppw);
  const RocheTheta th = load_theta(a.theta, ABLATE);
  Ml ml;
  ml.load(a.w1, a.b1, 0);
  MlColSlice<D, 1> mc;
  mc.load(a.w1, 0);
  const float ln_ec50 = log_f32(th.ec50);
  DoseSched<K1> us = load_dose<K1>(a, lm.p);
  const float dosage = us.dosage;
  us.dosage = 1.0f;  // the schedule at unit dosage
  GradAcc<D, 1> acc;
  acc.zero();
  float gd = 0.f;  // d loss / d dosage of this lane's patient

  const size_t row = (size_t)a.B * D;
  const float* hp = a.h + (size_t)(a.T - 1) * row + (size_t)lm.p * D;
  const float* gp = a.grad_h + (size_t)(a.T - 1) * row + (size_t)lm.p * D;
  const float live = lm.live ? 1.0f : 0.0f;

  float lam[D];
  load_vec<D>(gp, lam);
#pragma unroll
  for (int i = 0; i < D; ++i) lam[i] *= live;

  float y[D], gh[D];
  if (a.T > 1) {
    load_vec<D>(hp - row, y);
    load_vec<D>(gp - row, gh);
  }
  for (int n = a.T - 2; n >= 0; --n) {
    hp -= row;
    gp -= row;
    // prefetch the operands of the next (earlier) step while this one computes
    float y_nx[D], gh_nx[D];
    if (n > 0) {
      load_vec<D>(hp - row, y_nx);
      load_vec<D>(gp - row, gh_nx);
    }
    const StageTimes st(a.t, n, a.perturb, METHOD);
    const float dt = st.dt;
    float k1[D], s1[MR], a_[D], g[D];
    const Stage d1(us, dosage, st.t_first, th.kel);
    roche_rhs<D, 1, ABLATE, HILL2>(th, ml, d1.val.v, y, k1, s1);
    if constexpr (METHOD == HODE_METHOD_EULER) {
#pragma unroll
      for (int i = 0; i < D; ++i) g[i] = dt * lam[i];
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d1.val, y, s1, g, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g[3], th.kel * d1.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) lam[i] += a_[i];
    } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      float Y2[D], k2[D], s2[MR];
      const float half = 0.5f * dt;
#pragma unroll
      for (int i = 0; i < D; ++i) Y2[i] = __builtin_fmaf(k1[i], half, y[i]);
      const Stage d2(us, dosage, st.ta, th.kel);
      roche_rhs<D, 1, ABLATE, HILL2>(th, ml, d2.val.v, Y2, k2, s2);
#pragma unroll
      for (int i = 0; i < D; ++i) g[i] = dt * lam[i];
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d2.val, Y2, s2, g, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g[3], th.kel * d2.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        lam[i] += a_[i];
        g[i] = half * a_[i];
      }
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d1.val, y, s1, g, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g[3], th.kel * d1.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) lam[i] += a_[i];
    } else {
      float Y2[D], Y3[D], Y4[D], k2[D], k3[D], k4[D], s2[MR], s3[MR], s4[MR];
#pragma unroll
      for (int i = 0; i < D; ++i) Y2[i] = __builtin_fmaf(dt * k1[i], kOneThird, y[i]);
      const Stage d2(us, dosage, st.ta, th.kel);
      roche_rhs<D, 1, ABLATE, HILL2>(th, ml, d2.val.v, Y2, k2, s2);
#pragma unroll
      for (int i = 0; i < D; ++i) Y3[i] = __builtin_fmaf(dt, __builtin_fmaf(-k1[i], kOneThird, k2[i]), y[i]);
      const Stage d3(us, dosage, st.tb, th.kel);
      roche_rhs<D, 1, ABLATE, HILL2>(th, ml, d3.val.v, Y3, k3, s3);
#pragma unroll
      for (int i = 0; i < D; ++i) Y4[i] = __builtin_fmaf(dt, (k1[i] - k2[i]) + k3[i], y[i]);
      const Stage d4(us, dosage, st.t_last, th.kel);
      roche_rhs<D, 1, ABLATE, HILL2>(th, ml, d4.val.v, Y4, k4, s4);  // only s4 is needed (k4 is dead code)

      const float w1 = dt * 0.125f, w3 = dt * 0.375f;
      float g1[D], g2[D];
      // stage 4
#pragma unroll
      for (int i = 0; i < D; ++i) g[i] = w1 * lam[i];
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d4.val, Y4, s4, g, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g[3], th.kel * d4.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const float da_ = dt * a_[i];
        g1[i] = __builtin_fmaf(w1, lam[i], da_);
        g2[i] = __builtin_fmaf(w3, lam[i], -da_);
        g[i] = __builtin_fmaf(w3, lam[i], da_);
        lam[i] += a_[i];
      }
      // stage 3
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d3.val, Y3, s3, g, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g[3], th.kel * d3.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const float da_ = dt * a_[i];
        g2[i] += da_;
        g1[i] = __builtin_fmaf(-kOneThird, da_, g1[i]);
        lam[i] += a_[i];
      }
      // stage 2
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d2.val, Y2, s2, g2, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g2[3], th.kel * d2.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        g1[i] = __builtin_fmaf(kOneThird, dt * a_[i], g1[i]);
        lam[i] += a_[i];
      }
      // stage 1
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, d1.val, y, s1, g1, 0, a_, acc);
      if constexpr (!ABLATE) gd = __builtin_fmaf(g1[3], th.kel * d1.unit, gd);
#pragma unroll
      for (int i = 0; i < D; ++i) lam[i] += a_[i];
    }
    // cotangent of the output sample at t_n
#pragma unroll
    for (int i = 0; i < D; ++i) lam[i] = __builtin_fmaf(gh[i], live, lam[i]);
    if (n > 0) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        y[i] = y_nx[i];
        gh[i] = gh_nx[i];
      }
    }
  }
  store_vec<D, 1>(a.grad_y0 + (size_t)lm.p * D, lam, 0, lm.live);
  if (lm.live) da.grad_dosage[lm.p] = gd;  // the patient's own lane; an idle lane writes nothing
  if (a.status) {
    bool bad = !__builtin_isfinite(gd);
#pragma unroll
    for (int i = 0; i < D; ++i) bad |= !__builtin_isfinite(lam[i]);
    if (bad && lm.live) atomicOr(a.status, HODE_STATUS_NONFINITE);
  }

  // ---- fold the per-lane parameter gradients over the patients of this wave, one partial row per wave (an idle lane's
  // cotangents are zero, so it adds zeros)
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  float* out = a.partials + (size_t)wave * n_partials<D, 1>();
  if constexpr (M > 0) {
#pragma unroll
    for (int r = 0; r < MR; ++r) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const float s = wave_sum(acc.dw[r][i]);
        if (lane == 0) out[r * D + i] = s;
      }
      const float sb = wave_sum(acc.db[r]);
      if (lane == 0) out[M * D + r] = sb;
    }
  }
#pragma unroll
  for (int i = 0; i < kNTheta; ++i) {
    const float v = wave_sum(NEED_TH ? acc.dth[i] : 0.f);
    if (lane == 0) out[M * D + M + i] = v;
  }
}

template <int D, int METHOD, bool ABLATE, bool NEED_TH>
__global__ __launch_bounds__(64) void dose_bwd_kernel(DoseArgs a) {
  // the Hill-2 body and the one-dose fast path, chosen at run time as rk_bwd_kernel does (wave-uniform branches)
  const bool hill2 = ABLATE || (a.rk.theta[0] == 2.0f && a.rk.theta[1] == 2.0f);
  if (hill2 && a.rk.K == 1) dose_bwd_body<D, METHOD, ABLATE, true, NEED_TH, true>(a);
  else if (hill2) dose_bwd_body<D, METHOD, ABLATE, true, NEED_TH, false>(a);
  else dose_bwd_body<D, METHOD, ABLATE, false, NEED_TH, false>(a);
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
