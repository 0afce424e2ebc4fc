// Adaptive Dormand-Prince 5(4) solve of the NeuralODE rhs dy/dt = tanh(W2 tanh(W1 [y, Dose(t)] + b1) + b2) and its discrete
// adjoint on the matrix cores, gfx950.
//
// Replaces torchdiffeq.odeint(NeuralODE, ..., method="dopri5") -- what run_simulation --method=neural reaches with the
// reference's default solver (sim_config.py:50; rhs model.py:969-1026, call site :1116) -- and autograd's replay of its
// accepted steps.  CPU restatement: oracle/rhs.py::NeuralRHS + oracle/solvers.py::_odeint_dopri5.
//
// Controller, tape and launch structure are those of the Roche kernels (hode_dopri5_kernels.hpp): one
// launch per attempted step, controller record in device memory, batch-global RMS error norm through per-wave partials
// that every wave of the next launch folds in a fixed order, accepted states appended to tape_y.  The rhs is
// hode_neural_mf.hpp's register-resident MFMA product: a wave owns 16 patients, lane (g, n) holds rows 4g .. 4g+3 of
// patient n of every vector (state, stage derivative, cotangent) -- the solver algebra around the rhs is element-wise on
// those four registers.
//
// Backward: one launch walks the tape in reverse (same recurrences as dp_bwd_body_own, including sigma = d loss / d dt_0,
// which for this rhs has no stage-time term: Dose(t) is an impulse, `times == t`, without a derivative).  The stage VJPs
// recompute the hidden activations from the stage state instead of holding seven sets of them.  WEIGHT GRADIENTS ARE
// ACCUMULATED ON CHIP: they are outer products summed over patients, i.e. 16 x 16 x (16 patients) matrix products per wave
// and stage -- the pre-activation cotangents and the layer inputs are transposed through two LDS images (patient-major) so
// that the patient index becomes the MFMA contraction index, and the wave keeps dW1 | db1 (a ones row appended to the
// layer-1 input) and dW2 in 2 x HT accumulator tiles for the whole sweep.  One partial block per wave, folded in a fixed
// order by neural_grad_fold_kernel (deterministic; no operand tape in HBM, no host GEMM).
//
// The kernel templates and the host templates that launch them (nd_fwd, nd_bwd) are in hode_neural_dopri5_kernels.hpp; this
// file keeps the dispatch over the latent dimensions libhode.so holds (HODE_NEURAL_DIMS, hode_host.hpp; the odd ones
// 5 .. 15 are instantiated from the same header by neural_odd/hode_neural_odd_dim.hip for libhode_neural_odd.so).
#include <hip/hip_runtime.h>

#include "hode_neural_dopri5_kernels.hpp"

namespace hode {

size_t neural_dopri5_workspace_bytes(const hode_solve_desc* d) {
  switch (d->latent_dim) {
#define HODE_ND_CASE(n) case n: return nd_layout<n>(d).total;
    HODE_NEURAL_DIMS(HODE_ND_CASE)
#undef HODE_ND_CASE
  }
  return 0;
}

int neural_dopri5_tape_offsets(const hode_solve_desc* d, size_t* out5) {
  switch (d->latent_dim) {
#define HODE_ND_CASE(n) case n: adaptive_tape_offsets(nd_layout<n>(d), out5); return 0;
    HODE_NEURAL_DIMS(HODE_ND_CASE)
#undef HODE_ND_CASE
  }
  return fail(HODE_E_UNSUPPORTED, "neural dopri5: latent_dim %d has no compiled kernel (have 4, 6, 8, 10, 12, 14)", d->latent_dim);
}

int neural_dopri5(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (d->hidden_dim != 10 * d->latent_dim)
    return fail(HODE_E_UNSUPPORTED, "neural dopri5: hidden_dim %d != 10 * latent_dim (model.py:992)", d->hidden_dim);
  if (!d->w1 || !d->b1 || !d->w2 || !d->b2) return fail(HODE_E_NULL, "neural dopri5: w1 / b1 / w2 / b2 required");
  switch (d->latent_dim) {
#define HODE_ND_CASE(n) case n: return bwd ? nd_bwd<n>(d, s) : nd_fwd<n>(d, s);
    HODE_NEURAL_DIMS(HODE_ND_CASE)
#undef HODE_ND_CASE
  }
  return fail(HODE_E_UNSUPPORTED, "neural dopri5: latent_dim %d has no compiled kernel (have 4, 6, 8, 10, 12, 14)", d->latent_dim);
}

}  // namespace hode
