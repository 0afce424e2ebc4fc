// NeuralODE rhs on the matrix cores: dy/dt = tanh(W2 tanh(W1 [y, Dose(t)] + b1) + b2) (reference model.py:969-1026) inside
// the fixed-grid euler / midpoint / rk4(3/8) loop and its discrete adjoint, gfx950.  Same C-ABI contract, tape format and
// arithmetic (up to summation order) as the one-patient-per-lane kernels in hode_neural.hip, which stay as the fallback
// (lanes_per_patient = 1).
//
// A wave owns 16 patients for the whole time loop; the state never leaves registers.  With v_mfma_f32_16x16x4_f32
// (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], C/D rows 4 (lane >> 4) + reg, column lane & 15) and
// g = lane >> 4, n = lane & 15 (the patient):
//   * a vector over at most 16 "rows" (the input e = [y, Dose, 0..], an output, a cotangent) is ONE accumulator tile:
//     lane (g, n) holds rows 4g + r in register r;
//   * the contraction index of every product is ordered so that k-chunk r consists of the rows {4g + r : g = 0..3}: then
//     the B fragment of chunk r IS register r of the tile the previous product (or the element-wise step) left -- no
//     cross-lane traffic, no LDS, anywhere in the loop;
//   * the four weight operands (W1, W2, W2^T, W1^T, zero padded to 16-row tiles) are gathered once per launch into
//     that fragment order and stay in registers: 4 x 4 x HT floats per lane, HT = ceil(10 D / 16) hidden tiles.
// Per rhs evaluation: 4 HT MFMAs for the hidden layer, 4 HT for the output layer (4 partial accumulators: a single
// dependent chain would serialise on the MFMA latency), tanh on 4 HT + 4 values per lane; the VJP costs the same again.
// The weight gradients are outer products summed over patients: as in hode_neural.hip the backward tapes their operands
// patient-minor for the caller's BLAS GEMMs (hode/neural.py) -- same offsets, same layout.
//
// The two kernel templates are in hode_neural_mf_kernels.hpp; this file keeps the launcher and the dispatch over the latent
// dimensions libhode.so holds (the odd ones 5 .. 15: neural_odd/hode_neural_odd_dim.hip, libhode_neural_odd.so).
#include <hip/hip_runtime.h>

#include "hode_neural_mf_kernels.hpp"

namespace hode {

template <int D>
int launch_neural_mf_d(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) {
  const dim3 grid((d->batch + 15) / 16), block(64);
  const bool onchip = bwd && d->grad_w1 != nullptr;
#define HODE_NEURAL_MF_LAUNCH(M)                                                                   \
  if (bwd && onchip) hipLaunchKernelGGL((neural_mf_bwd_kernel<D, M, true>), grid, block, 0, s, a);  \
  else if (bwd) hipLaunchKernelGGL((neural_mf_bwd_kernel<D, M, false>), grid, block, 0, s, a);      \
  else hipLaunchKernelGGL((neural_mf_fwd_kernel<D, M>), grid, block, 0, s, a);
  switch (d->method) {
    case HODE_METHOD_EULER: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_EULER) break;
    case HODE_METHOD_MIDPOINT: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_MIDPOINT) break;
    default: HODE_NEURAL_MF_LAUNCH(HODE_METHOD_RK4_38) break;
  }
  if (onchip)
    hipLaunchKernelGGL((neural_grad_fold_kernel<D>), dim3(NeuralGradAcc<D>::NP), block, 0, s, a.a1t, (int)grid.x, d->grad_w1,
                       d->grad_b1, d->grad_w2, d->grad_b2);
  return hip_fail(hipGetLastError(), "neural MFMA kernel launch");
}

// bytes of per-wave gradient partials the on-chip backward needs (it uses the a1t slot of the workspace for them)
size_t neural_mf_partial_bytes(const hode_solve_desc* d) {
  const size_t nw = (d->batch + 15) / 16;
  switch (d->latent_dim) {
    case 4: return nw * NeuralGradAcc<4>::NP * sizeof(float);
    case 6: return nw * NeuralGradAcc<6>::NP * sizeof(float);
    case 8: return nw * NeuralGradAcc<8>::NP * sizeof(float);
    case 10: return nw * NeuralGradAcc<10>::NP * sizeof(float);
    case 14: return nw * NeuralGradAcc<14>::NP * sizeof(float);
    default: return nw * NeuralGradAcc<12>::NP * sizeof(float);
  }
}

int launch_neural_mf(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) {
  switch (d->latent_dim) {   // check_neural admits 4, 6, ..., 14: [y, Dose, 1] fits one 16-row tile
    case 4: return launch_neural_mf_d<4>(d, a, bwd, s);
    case 6: return launch_neural_mf_d<6>(d, a, bwd, s);
    case 8: return launch_neural_mf_d<8>(d, a, bwd, s);
    case 10: return launch_neural_mf_d<10>(d, a, bwd, s);
    case 14: return launch_neural_mf_d<14>(d, a, bwd, s);
    default: return launch_neural_mf_d<12>(d, a, bwd, s);
  }
}

}  // namespace hode
