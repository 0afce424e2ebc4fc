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
// The two kernel templates and their launcher are in hode_neural_mf_kernels.hpp; this file keeps the dispatch over the latent
// dimensions libhode.so holds (HODE_NEURAL_DIMS; the odd ones 5 .. 15: neural_odd/hode_neural_odd_dim.hip,
// libhode_neural_odd.so).
#include <hip/hip_runtime.h>

#include "hode_neural_mf_kernels.hpp"

namespace hode {

// hode_workspace_bytes asks for the partials of any latent_dim, also one nobody serves (the launch is refused by
// check_neural): such a size has always been answered, and launched, as this one
constexpr int kUnlistedDim = 12;

size_t neural_mf_partial_bytes(const hode_solve_desc* d) {
  switch (d->latent_dim) {
#define HODE_NEURAL_MF_CASE(n) case n: return neural_mf_partial_bytes_d<n>(d);
    HODE_NEURAL_DIMS(HODE_NEURAL_MF_CASE)
#undef HODE_NEURAL_MF_CASE
  }
  return neural_mf_partial_bytes_d<kUnlistedDim>(d);
}

int launch_neural_mf(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) {
  switch (d->latent_dim) {   // check_neural admits 4, 6, ..., 14: [y, Dose, 1] fits one 16-row tile
#define HODE_NEURAL_MF_CASE(n) case n: return launch_neural_mf_d<n, true>(d, a, bwd, s);
    HODE_NEURAL_DIMS(HODE_NEURAL_MF_CASE)
#undef HODE_NEURAL_MF_CASE
  }
  return launch_neural_mf_d<kUnlistedDim, true>(d, a, bwd, s);
}

}  // namespace hode
