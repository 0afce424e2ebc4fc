// The kernels of libhode_real_dims.so at one hidden-tile count HT = HODE_REAL_DIMS_HT (hidden_dim <= 16 HT): the real-data
// hybrid rhs on the matrix cores with the GRU block as a RAGGED 16-row tile, M = latent_dim - 4 a runtime argument, so that
// one set of instantiations (method x forward / backward, plus the fold) serves every latent size 5 .. 20.  The device
// code is ../hode_real_mf.hpp, which libhode.so's M = 16 kernels (../hode_real_mf.hip) instantiate with the full tile.
// The backward accumulates the weight gradients on chip; there is no operand-tape variant here.
#include <hip/hip_runtime.h>

#include "../hode_real_mf.hpp"
#include "hode_real_dims.hpp"

#ifndef HODE_REAL_DIMS_HT
#error "compile with -DHODE_REAL_DIMS_HT=<1 .. 4>"
#endif

namespace hode {

constexpr int kHT = HODE_REAL_DIMS_HT;
static_assert(kHT >= 1 && kHT <= 4, "hidden tiles");
static_assert(RealGradAcc<kHT>::NP == real_side_partial_floats(kHT), "partial block size");

template <int HT, int METHOD, bool BWD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_dims_kernel(RealArgs a, int M) {
  __shared__ __attribute__((aligned(16))) float lds[BWD ? RealGradAcc<HT>::kLdsFloats : 4];
  real_mf_body<HT, METHOD, BWD, BWD>(a, RealTileRagged{M}, lds);
}

// the three M x M blocks are written with M as row stride; padded rows and columns of the tiles are never written
template <int HT>
__global__ __launch_bounds__(64) void real_dims_fold_kernel(const float* __restrict__ partials, int n_waves, int H, int M,
                                                            float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, M, gw);
}

template <int METHOD>
static void launch_method(bool bwd, const RealArgs& a, int M, dim3 grid, hipStream_t s) {
  if (bwd) hipLaunchKernelGGL((real_dims_kernel<kHT, METHOD, true>), grid, dim3(64), 0, s, a, M);
  else hipLaunchKernelGGL((real_dims_kernel<kHT, METHOD, false>), grid, dim3(64), 0, s, a, M);
}

int HODE_CAT(real_dims_launch_ht, HODE_REAL_DIMS_HT)(int method, bool bwd, const RealArgs& a, int M, float* grad_w, hipStream_t s) {
  const dim3 grid((a.B + 15) / 16);
  switch (method) {
    case HODE_METHOD_EULER: launch_method<HODE_METHOD_EULER>(bwd, a, M, grid, s); break;
    case HODE_METHOD_MIDPOINT: launch_method<HODE_METHOD_MIDPOINT>(bwd, a, M, grid, s); break;
    default: launch_method<HODE_METHOD_RK4_38>(bwd, a, M, grid, s); break;
  }
  if (bwd)
    hipLaunchKernelGGL((real_dims_fold_kernel<kHT>), dim3(RealGradAcc<kHT>::NP), dim3(64), 0, s, a.tape, (int)grid.x, a.H, M, grad_w);
  return hip_fail(hipGetLastError(), "real dims kernel launch");
}

}  // namespace hode
