// Kernel templates of the fixed-grid NeuralODE solve on the matrix cores (hode_neural_mf.hip has the description of the
// layout), and the host templates that launch them.  Instantiated by hode_neural_mf.hip for libhode.so (even latent
// dimensions) and by neural_odd/hode_neural_odd_dim.hip for libhode_neural_odd.so (odd ones).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_host.hpp"
#include "hode_neural_args.hpp"
#include "hode_neural_mf.hpp"

namespace hode {

template <int D, int METHOD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void neural_mf_fwd_kernel(NeuralArgs a) {
  const int lane = threadIdx.x;
  NeuralMf<D> nn;
  nn.load(a, lane);
  const int g = nn.g;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const float dosage = a.dosage[p];
  const size_t row = (size_t)a.B * D;
  v4 y = mf_load_rows<D>(a.y0 + (size_t)p * D, g);
  float* hp = a.h + (size_t)p * D;
  mf_store_rows<D>(hp, g, y, live);
  v4 a1[NeuralMf<D>::HT];
  for (int nstep = 0; nstep + 1 < a.T; ++nstep) {
    const NStageTimes st(a.t, nstep, a.perturb, METHOD);
    const float dt = st.dt;
    const v4 k1 = nn.rhs(mf_with_dose<D>(y, neural_dose(a, p, dosage, st.t_first), g), a1);
    if constexpr (METHOD == HODE_METHOD_EULER) {
      y = y + dt * k1;
    } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      const v4 Y = y + (0.5f * dt) * k1;
      const v4 k2 = nn.rhs(mf_with_dose<D>(Y, neural_dose(a, p, dosage, st.ta), g), a1);
      y = y + dt * k2;
    } else {
      v4 Y = y + (dt * k1) * kThird;
      const v4 k2 = nn.rhs(mf_with_dose<D>(Y, neural_dose(a, p, dosage, st.ta), g), a1);
      Y = y + dt * (k2 - k1 * kThird);
      const v4 k3 = nn.rhs(mf_with_dose<D>(Y, neural_dose(a, p, dosage, st.tb), g), a1);
      Y = y + dt * ((k1 - k2) + k3);
      const v4 k4 = nn.rhs(mf_with_dose<D>(Y, neural_dose(a, p, dosage, st.t_last), g), a1);
      y = y + ((k1 + 3.0f * (k2 + k3)) + k4) * (dt * 0.125f);
    }
    hp += row;
    mf_store_rows<D>(hp, g, y, live);
  }
}

// ONCHIP: the weight gradients are accumulated by the wave on the matrix cores (NeuralGradAcc, hode_neural_mf.hpp) and
// leave as one partial block per wave in a.a1t (folded by neural_grad_fold_kernel); otherwise their operands are taped
// patient-minor for the caller's GEMMs (the contract of hode_neural_tape_offsets, kept for the lane-per-patient kernels).
template <int D, int METHOD, bool ONCHIP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void neural_mf_bwd_kernel(NeuralArgs a) {
  constexpr int HD = 10 * D;
  constexpr int HT = NeuralMf<D>::HT;
  __shared__ __attribute__((aligned(16))) float lds[ONCHIP ? NeuralGradAcc<D>::kLdsFloats : 4];
  NeuralGradAcc<D> acc;
  if constexpr (ONCHIP) acc.init(lds);
  constexpr int NS = METHOD == HODE_METHOD_EULER ? 1 : (METHOD == HODE_METHOD_MIDPOINT ? 2 : 4);
  const int lane = threadIdx.x;
  NeuralMf<D> nn;
  nn.load(a, lane);
  const int g = nn.g;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const float lv = live ? 1.0f : 0.0f;
  const size_t B = a.B;
  const float dosage = a.dosage[p];
  const size_t row = B * D;
  v4 lam = lv * mf_load_rows<D>(a.grad_h + (size_t)(a.T - 1) * row + (size_t)p * D, g);

  // tapes: operand rows patient-minor, [inst][rows][B]
  auto tape_hidden = [&](float* base, size_t inst, const v4 (&v)[HT]) {
    if (!live) return;
    float* dst = base + inst * HD * B + p;
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rw = 16 * i + 4 * g + r;
        if (rw < HD) dst[(size_t)rw * B] = v[i][r];
      }
  };
  auto tape_rows = [&](float* base, size_t inst, int nrows, const v4& v) {
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rw = 4 * g + r;
      if (rw < nrows) base[(inst * nrows + rw) * B + p] = v[r];
    }
  };

  for (int nstep = a.T - 2; nstep >= 0; --nstep) {
    const NStageTimes st(a.t, nstep, a.perturb, METHOD);
    const float dt = st.dt;
    const size_t i0 = (size_t)nstep * NS;
    const v4 y = mf_load_rows<D>(a.h + (size_t)nstep * row + (size_t)p * D, g);
    v4 e[NS], k[NS], a1[ONCHIP ? 1 : NS][HT];  // ONCHIP: only the last stage's activations stay, the VJPs recompute theirs
    // ---- recompute the stages (inputs and hidden activations go to the tape as they are formed)
    e[0] = mf_with_dose<D>(y, neural_dose(a, p, dosage, st.t_first), g);
    k[0] = nn.rhs(e[0], a1[0]);
    if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      e[1] = mf_with_dose<D>(y + (0.5f * dt) * k[0], neural_dose(a, p, dosage, st.ta), g);
      k[1] = nn.rhs(e[1], a1[ONCHIP ? 0 : 1]);
    } else if constexpr (METHOD == HODE_METHOD_RK4_38) {
      e[1] = mf_with_dose<D>(y + (dt * k[0]) * kThird, neural_dose(a, p, dosage, st.ta), g);
      k[1] = nn.rhs(e[1], a1[ONCHIP ? 0 : 1]);
      e[2] = mf_with_dose<D>(y + dt * (k[1] - k[0] * kThird), neural_dose(a, p, dosage, st.tb), g);
      k[2] = nn.rhs(e[2], a1[ONCHIP ? 0 : 2]);
      e[3] = mf_with_dose<D>(y + dt * ((k[0] - k[1]) + k[2]), neural_dose(a, p, dosage, st.t_last), g);
      k[3] = nn.rhs(e[3], a1[ONCHIP ? 0 : 3]);
    }
    if constexpr (!ONCHIP) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        tape_rows(a.yet, i0 + s, D + 1, e[s]);
        tape_hidden(a.a1t, i0 + s, a1[s]);
      }
    }
    // ---- adjoint of the stages
    auto vjp = [&](int s, const v4& gk) {
      v4 u2, u1[HT];
      if constexpr (ONCHIP) {
        if (s != NS - 1) nn.hidden(e[s], a1[0]);  // 384 registers of activations would not fit next to the accumulators
      }
      v4 av = nn.vjp(a1[ONCHIP ? 0 : s], k[s], gk, u2, u1);
      if constexpr (ONCHIP) {
        acc.add(u1, e[s], u2, a1[0], g, nn.n);
      } else {
        tape_rows(a.u2t, i0 + s, D, u2);
        tape_hidden(a.u1t, i0 + s, u1);
      }
      if (g == NeuralMf<D>::GD) av[NeuralMf<D>::RD] = 0.f;  // the Dose input is not a state
      return av;
    };
    if constexpr (METHOD == HODE_METHOD_EULER) {
      lam = lam + vjp(0, dt * lam);
    } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      const v4 a1v = vjp(1, dt * lam);
      lam = lam + a1v;
      lam = lam + vjp(0, (0.5f * dt) * a1v);
    } else {
      const float w1 = dt * 0.125f, w3 = dt * 0.375f;
      const v4 a3 = vjp(3, w1 * lam);
      v4 da = dt * a3;
      v4 g1 = w1 * lam + da;
      v4 g2 = w3 * lam - da;
      const v4 gg = w3 * lam + da;
      lam = lam + a3;
      const v4 a2 = vjp(2, gg);
      da = dt * a2;
      g2 = g2 + da;
      g1 = g1 - kThird * da;
      lam = lam + a2;
      const v4 a1v = vjp(1, g2);
      g1 = g1 + kThird * (dt * a1v);
      lam = lam + a1v;
      lam = lam + vjp(0, g1);
    }
    lam = lam + lv * mf_load_rows<D>(a.grad_h + (size_t)nstep * row + (size_t)p * D, g);
  }
  mf_store_rows<D>(a.grad_y0 + (size_t)p * D, g, lam, live);
  if constexpr (ONCHIP) acc.store(a.a1t + (size_t)blockIdx.x * NeuralGradAcc<D>::NP, lane);
}

// ------------------------------------------------------------------------------------------------ host side
// (internal linkage: helpers of the unit that instantiates them, not names of its library)
// bytes of per-wave gradient partials the on-chip backward needs (it uses the a1t slot of the workspace for them)
template <int D>
static size_t neural_mf_partial_bytes_d(const hode_solve_desc* d) {
  return (size_t)((d->batch + 15) / 16) * NeuralGradAcc<D>::NP * sizeof(float);
}

// One fixed-grid solve or its backward.  With grad_w1 the backward accumulates the weight gradients on chip and folds the
// per-wave partials; without it, it tapes their operands for the caller -- an instantiation that exists only where
// OPERAND_TAPE is set (libhode.so; libhode_neural_odd.so holds the on-chip backward alone and refuses such a call).
template <int D, bool OPERAND_TAPE>
static int launch_neural_mf_d(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) {
  const dim3 grid((d->batch + 15) / 16), block(64);
  const bool onchip = bwd && d->grad_w1 != nullptr;
  if (!OPERAND_TAPE && bwd && !onchip) return fail(HODE_E_UNSUPPORTED, "neural MFMA backward: the operand-tape mode is not built here");
#define HODE_NEURAL_MF_LAUNCH(M)                                                                      \
  if (bwd && onchip) hipLaunchKernelGGL((neural_mf_bwd_kernel<D, M, true>), grid, block, 0, s, a);     \
  else if (bwd) {                                                                                     \
    if constexpr (OPERAND_TAPE) hipLaunchKernelGGL((neural_mf_bwd_kernel<D, M, false>), grid, block, 0, s, a); \
  } else hipLaunchKernelGGL((neural_mf_fwd_kernel<D, M>), grid, block, 0, s, a);
  switch (d->method) {
    case HODE_METHOD_EULER: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_EULER) break;
    case HODE_METHOD_MIDPOINT: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_MIDPOINT) break;
    default: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_RK4_38) break;
  }
#undef HODE_NEURAL_MF_LAUNCH
  if (onchip)
    hipLaunchKernelGGL((neural_grad_fold_kernel<D>), dim3(NeuralGradAcc<D>::NP), block, 0, s, a.a1t, (int)grid.x, d->grad_w1,
                       d->grad_b1, d->grad_w2, d->grad_b2);
  return hip_fail(hipGetLastError(), "neural MFMA kernel launch");
}

}  // namespace hode
