// Internal to libhode_neural_odd.so: what hode_neural_odd_dim.hip (compiled once per -DHODE_DIM=<D>) gives the entry
// points in hode_neural_odd.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/hode_neural_odd.h"

namespace hode {

struct NeuralArgs;

// the odd latent dimensions: [y, Dose] fits one 16-row tile up to D = 15
#define HODE_NEURAL_ODD_DIMS(X) X(5) X(7) X(9) X(11) X(13) X(15)

struct NeuralOddDim {
  int latent_dim;
  size_t (*rk_partial_bytes)(const hode_solve_desc* d);  // per-wave gradient partials of the fixed-grid backward
  int (*rk)(const hode_solve_desc* d, const NeuralArgs& a, bool bwd, hipStream_t s);
  size_t (*dopri5_workspace_bytes)(const hode_solve_desc* d);
  void (*dopri5_tape_offsets)(const hode_solve_desc* d, size_t* out5);
  int (*dopri5)(const hode_solve_desc* d, bool bwd, hipStream_t s);
};

// (functions, not tables: a const table of host function pointers would be emitted for the device too)
#define HODE_NEURAL_ODD_DECL(n) const NeuralOddDim* neural_odd_d##n();
HODE_NEURAL_ODD_DIMS(HODE_NEURAL_ODD_DECL)
#undef HODE_NEURAL_ODD_DECL

}  // namespace hode
