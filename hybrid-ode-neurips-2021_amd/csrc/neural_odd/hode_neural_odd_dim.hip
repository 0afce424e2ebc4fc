// libhode_neural_odd.so, one latent dimension (-DHODE_DIM=<D>, D odd, 5 .. 15): the NeuralODE kernels of
// ../hode_neural_mf_kernels.hpp (fixed grid) and ../hode_neural_dopri5_kernels.hpp (adaptive) instantiated at D, behind
// short host launchers.  Only the on-chip backward (weight gradients accumulated by the wave) is instantiated.
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

size_t rk_partial_bytes(const hode_solve_desc* d) {
  return (size_t)((d->batch + 15) / 16) * NeuralGradAcc<kD>::NP * sizeof(float);
}

int rk(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s) {
  const dim3 grid((d->batch + 15) / 16), block(64);
#define HODE_NEURAL_ODD_LAUNCH(M)                                                            \
  if (bwd) hipLaunchKernelGGL((neural_mf_bwd_kernel<kD, M, true>), grid, block, 0, s, a);     \
  else hipLaunchKernelGGL((neural_mf_fwd_kernel<kD, M>), grid, block, 0, s, a);
  switch (d->method) {
    case HODE_METHOD_EULER: HODE_NEURAL_ODD_LAUNCH(HODE_METHOD_EULER) break;
    case HODE_METHOD_MIDPOINT: HODE_NEURAL_ODD_LAUNCH(HODE_METHOD_MIDPOINT) break;
    default: HODE_NEURAL_ODD_LAUNCH(HODE_METHOD_RK4_38) break;
  }
#undef HODE_NEURAL_ODD_LAUNCH
  if (bwd)
    hipLaunchKernelGGL((neural_grad_fold_kernel<kD>), dim3(NeuralGradAcc<kD>::NP), block, 0, s, a.a1t, (int)grid.x, d->grad_w1,
                       d->grad_b1, d->grad_w2, d->grad_b2);
  return hip_fail(hipGetLastError(), "neural MFMA kernel launch");
}

size_t dopri5_workspace_bytes(const hode_solve_desc* d) { return nd_layout<kD>(d).total; }

void dopri5_tape_offsets(const hode_solve_desc* d, size_t* out5) {
  const NdLayout L = nd_layout<kD>(d);
  out5[0] = L.ctrl + kNdInitOffset; out5[1] = L.tape_t; out5[2] = L.tape_dt; out5[3] = L.tape_j; out5[4] = L.tape_y;
}

// the launch sequence of hode_neural_dopri5.hip's nd_bwd
int dopri5_bwd(const hode_solve_desc* d, hipStream_t s) {
  const NdLayout lay = nd_layout<kD>(d);
  if (!d->workspace || d->workspace_bytes < lay.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, lay.total);
  NdpArgs a = nd_args<kD>(d, lay);
  a.n_acc = *d->host_n_accepted;
  if (a.n_acc < 0 || a.n_acc > d->max_steps) return fail(HODE_E_SIZE, "n_accepted %d outside the tape", a.n_acc);
  const dim3 grid(a.n_waves), block(64), fgrid(NeuralGradAcc<kD>::NP);
  hipLaunchKernelGGL((ndp_bwd_kernel<kD>), grid, block, 0, s, a);
  hipLaunchKernelGGL((neural_grad_fold_kernel<kD>), fgrid, block, 0, s, a.grad_partials, a.n_waves, a.grad_w1, a.grad_b1, a.grad_w2, a.grad_b2);
  if (a.n_acc > 0 && !(d->flags & HODE_FLAG_DETACH_FIRST_STEP)) {
    hipLaunchKernelGGL((ndp_initbwd_kernel<kD, 1>), grid, block, 0, s, a);
    hipLaunchKernelGGL((ndp_initbwd_kernel<kD, 2>), grid, block, 0, s, a);
    hipLaunchKernelGGL((neural_grad_fold_kernel<kD>), fgrid, block, 0, s, a.grad_partials, a.n_waves, a.grad_w1, a.grad_b1, a.grad_w2, a.grad_b2);
  }
  return hip_fail(hipGetLastError(), "neural dopri5 backward launch");
}

int dopri5(const hode_solve_desc* d, bool bwd, hipStream_t s) { return bwd ? dopri5_bwd(d, s) : nd_fwd<kD>(d, s); }

}  // namespace

#define HODE_NEURAL_ODD_CAT2(a, b) a##b
#define HODE_NEURAL_ODD_CAT(a, b) HODE_NEURAL_ODD_CAT2(a, b)
const NeuralOddDim* HODE_NEURAL_ODD_CAT(neural_odd_d, HODE_DIM)() {
  static const NeuralOddDim entry = {kD, rk_partial_bytes, rk, dopri5_workspace_bytes, dopri5_tape_offsets, dopri5};
  return &entry;
}

}  // namespace hode
