// libhode_neural_odd.so, one latent dimension (-DHODE_DIM=<D>, D odd, 5 .. 15): the NeuralODE kernels of
// ../hode_neural_mf_kernels.hpp (fixed grid) and ../hode_neural_dopri5_kernels.hpp (adaptive) instantiated at D through
// the host launchers of those headers.  Only the on-chip backward (weight gradients accumulated by the wave) is
// instantiated: launch_neural_mf_d<D, false>.
#include <hip/hip_runtime.h>

#include "../hode_neural_dopri5_kernels.hpp"
#include "../hode_neural_mf_kernels.hpp"
#include "hode_neural_odd.hpp"

#ifndef HODE_DIM
#error "compile with -DHODE_DIM=<latent dimension>"
#endif

namespace hode {

namespace {

constexpr int kD = HODE_DIM;
static_assert(kD % 2 == 1 && kD >= 5 && kD + 1 <= 16, "odd latent dimensions whose [y, Dose] fits one 16-row tile");

size_t rk_partial_bytes(const hode_solve_desc* d) { return neural_mf_partial_bytes_d<kD>(d); }

int rk(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) { return launch_neural_mf_d<kD, false>(d, a, bwd, s); }

size_t dopri5_workspace_bytes(const hode_solve_desc* d) { return nd_layout<kD>(d).total; }

void dopri5_tape_offsets(const hode_solve_desc* d, size_t* out5) { adaptive_tape_offsets(nd_layout<kD>(d), out5); }

int dopri5(const hode_solve_desc* d, bool bwd, hipStream_t s) { return bwd ? nd_bwd<kD>(d, s) : nd_fwd<kD>(d, s); }

}  // namespace

#define HODE_NEURAL_ODD_CAT2(a, b) a##b
#define HODE_NEURAL_ODD_CAT(a, b) HODE_NEURAL_ODD_CAT2(a, b)
const NeuralOddDim* HODE_NEURAL_ODD_CAT(neural_odd_d, HODE_DIM)() {
  static const NeuralOddDim entry = {kD, rk_partial_bytes, rk, dopri5_workspace_bytes, dopri5_tape_offsets, dopri5};
  return &entry;
}

}  // namespace hode
