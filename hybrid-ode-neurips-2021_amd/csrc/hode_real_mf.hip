// Real-data hybrid rhs (two small MLPs + GRU-ODE block, reference model.py:613-645) on the matrix cores, inside the
// fixed-grid euler / midpoint / rk4(3/8) loop and its discrete adjoint, gfx950.  Same C-ABI contract, tape rows and
// arithmetic (up to summation order) as the one-patient-per-lane kernels of hode_real.hip, which stay as the fallback
// (lanes_per_patient = 1, and for shapes outside D = 20, hidden <= 64).
//
// Recipe of hode_neural_mf.hip: a wave owns 16 patients for the whole time loop; with v_mfma_f32_16x16x4_f32 a vector over
// <= 16 rows is one accumulator tile (lane (g, n): rows 4g + r of patient n in register r), every contraction is ordered
// so that k-chunk r is the rows {4g + r}, hence the B fragment of a product IS a register the lane already holds; all
// weight operands are gathered once per launch into that order and stay in registers.  The state is two tiles:
//   X = [x1, x2, x3, Dose2, 0...]  (only lanes g == 0 carry data)          H = the M = 16 GRU states
// and one rhs evaluation is
//   hidden(2 HP)  = tanh([W11; W21] X + [b11; b21])     5 HT MFMAs  (HP = 16 HT >= hidden_dim, both MLPs side by side)
//   (s1, s2)      = [w12 | w22] hidden + (b12, b22)     8 HT MFMAs  -> dx1 = tanh(s1), dx2 = tanh(s2)
//   r, z = sigma(Whr H), sigma(Whz H);  u = tanh(Whh (r*H));  dH = (1 - z)(u - H)      12 MFMAs
//   dx3 = x2 k_immunity,  dx4 = kel Dose(t) - kel2 Dose2          (VALU, lanes g == 0; Dose(t) from the per-patient table)
// i.e. 51 MFMAs instead of ~3 000 fmas with memory-sourced weights per lane; the VJP is 42 MFMAs.
#include <hip/hip_runtime.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_host.hpp"
#include "hode_real_args.hpp"
#include "hode_real_mf.hpp"  // RealMf, RealGradAcc, real_grad_fold, real_mf_body: shared with libhode_real_dims.so

namespace hode {

// fixed-order fold of the per-wave blocks into the flat weight gradient (RealW order); one wave per slot of a block
template <int HT>
__global__ __launch_bounds__(64) void real_grad_fold_kernel(const float* __restrict__ partials, int n_waves, int H,
                                                            float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, 16, gw);
}

// ONCHIP (backward): weight gradients accumulated by the wave (RealGradAcc), one partial block per wave in a.tape;
// otherwise the GEMM operands are taped for the caller (contract of the lane-per-patient kernels).
template <int HT, int METHOD, bool BWD, bool ONCHIP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_mf_kernel(RealArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[(BWD && ONCHIP) ? RealGradAcc<HT>::kLdsFloats : 4];
  real_mf_body<HT, METHOD, BWD, ONCHIP>(a, RealTileFull{}, lds);
}

bool real_mf_supported(const hode_solve_desc* d) {
  return d->latent_dim == 20 && d->hidden_dim >= 1 && d->hidden_dim <= 64;
}

template <int HT, bool BWD>
int launch_real_mf_ht(const hode_solve_desc* d, const RealArgs& a, hipStream_t s) {
  const dim3 grid((d->batch + 15) / 16), block(64);
  const bool onchip = BWD && d->grad_w1 != nullptr;
#define HODE_REAL_MF_LAUNCH(M)                                                                        \
  if (onchip) hipLaunchKernelGGL((real_mf_kernel<HT, M, BWD, BWD>), grid, block, 0, s, a);              \
  else hipLaunchKernelGGL((real_mf_kernel<HT, M, BWD, false>), grid, block, 0, s, a);
  switch (d->method) {
    case HODE_METHOD_EULER: HODE_REAL_MF_LAUNCH(HODE_METHOD_EULER) break;
    case HODE_METHOD_MIDPOINT: HODE_REAL_MF_LAUNCH(HODE_METHOD_MIDPOINT) break;
    default: HODE_REAL_MF_LAUNCH(HODE_METHOD_RK4_38) break;
  }
  if (onchip)
    hipLaunchKernelGGL((real_grad_fold_kernel<HT>), dim3(RealGradAcc<HT>::NP), block, 0, s, a.tape, (int)grid.x, d->hidden_dim,
                       d->grad_w1);
  return hip_fail(hipGetLastError(), "real MFMA kernel launch");
}

// bytes of per-wave gradient partials of the on-chip backward (they take the tape's place in the workspace)
size_t real_mf_partial_bytes(const hode_solve_desc* d) {
  const size_t nw = (d->batch + 15) / 16;
  switch ((d->hidden_dim + 15) / 16) {
    case 1: return nw * RealGradAcc<1>::NP * sizeof(float);
    case 2: return nw * RealGradAcc<2>::NP * sizeof(float);
    case 3: return nw * RealGradAcc<3>::NP * sizeof(float);
    default: return nw * RealGradAcc<4>::NP * sizeof(float);
  }
}

int launch_real_mf(const hode_solve_desc* d, const RealArgs& a, bool bwd, hipStream_t s) {
  const int ht = (d->hidden_dim + 15) / 16;
  switch (ht) {
    case 1: return bwd ? launch_real_mf_ht<1, true>(d, a, s) : launch_real_mf_ht<1, false>(d, a, s);
    case 2: return bwd ? launch_real_mf_ht<2, true>(d, a, s) : launch_real_mf_ht<2, false>(d, a, s);
    case 3: return bwd ? launch_real_mf_ht<3, true>(d, a, s) : launch_real_mf_ht<3, false>(d, a, s);
    default: return bwd ? launch_real_mf_ht<4, true>(d, a, s) : launch_real_mf_ht<4, false>(d, a, s);
  }
}

}  // namespace hode
