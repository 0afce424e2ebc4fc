// Host code of the fixed-grid Roche lane kernels (hode_rk_kernels.hpp) that every library holding them needs: the grid
// shape, the layout rule, the per-wave partial row and its fold, the kernel arguments and the argument checks.  The
// functions hode_host.hpp declares have external linkage, so this header is included by exactly ONE unit per library
// (hode_api.hip of libhode.so, roche_dims/hode_roche_dims.hip of libhode_roche_dims.so, and real_dims/hode_real_dims.hip of
// libhode_real_dims.so, which needs the partial fold alone), like hode_error_state.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hode_host.hpp"
#include "hode_roche.hpp"

namespace hode {

// out[j] += sum over waves of partials[w][j].  One wave per output element: lane l adds rows l, l+64, ... in order,
// then a fixed-shape butterfly folds the 64 lane sums -- the summation tree depends only on (n_waves), so the
// result is bit-reproducible run to run (no float atomics).
__global__ __launch_bounds__(64) void fold_partials_kernel(const float* __restrict__ partials, int n_waves, int P,
                                                           int n_w, int n_b, float* __restrict__ gw,
                                                           float* __restrict__ gb, float* __restrict__ gth, int need_th) {
  const int j = blockIdx.x;
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int w = lane; w < n_waves; w += 64) s += partials[(size_t)w * P + j];
  s = wave_sum(s);
  if (lane != 0) return;
  if (j < n_w) {
    if (gw) gw[j] += s;
  } else if (j < n_w + n_b) {
    if (gb) gb[j - n_w] += s;
  } else if (need_th && gth) {
    gth[j - n_w - n_b] += s;
  }
}

// patients per wave: as many waves as it takes to put one on (almost) every SIMD, then whole rounds of 1024
int patients_per_wave(int B, int lpp) {
  const int cap = 64 / lpp;
  const long long simds = 1024;
  const long long rounds = (B + simds * cap - 1) / (simds * cap);
  long long ppw = (B + simds * rounds - 1) / (simds * rounds);
  if (ppw < 1) ppw = 1;
  if (ppw > cap) ppw = cap;
  return (int)ppw;
}
int n_waves_for(int B, int lpp) {
  const int ppw = patients_per_wave(B, lpp);
  return (B + ppw - 1) / ppw;
}

// LPP = 4 (a patient per DPP quad, 16 patients per wave) fills the chip at the 10k-patient shape; LPP = 1 has
// the lowest total instruction count and wins once every SIMD has >= 2 waves without splitting patients
// (256 CUs x 4 SIMDs x 2 waves x 64 lanes = 131072 patients).
int choose_lpp(const hode_solve_desc* d) {
  const int M = d->latent_dim - 4;
  const bool can4 = M > 0 && M % 4 == 0;
  if (d->lanes_per_patient == 1) return 1;
  if (d->lanes_per_patient == 4) return can4 ? 4 : 1;
  if (!can4) return 1;
  return d->batch >= 131072 ? 1 : 4;
}

int n_partials(int latent_dim) {
  const int M = latent_dim - 4;
  return M * latent_dim + M + kNTheta;
}
int n_partials(const hode_solve_desc* d) { return n_partials(d->latent_dim); }


int launch_fold_partials(const float* partials, int n_waves, int P, int n_w, int n_b, float* gw, float* gb, float* gth,
                         int need_th, hipStream_t s) {
  hipLaunchKernelGGL(fold_partials_kernel, dim3(P), dim3(64), 0, s, partials, n_waves, P, n_w, n_b, gw, gb, gth, need_th);
  return hip_fail(hipGetLastError(), "fold_partials launch");
}


// the kernels' arguments; `lpp` is the layout the caller launches (it fixes the patients per wave)
static RkArgs rk_make_args(const hode_solve_desc* d, int lpp) {
  RkArgs a{};
  a.t = d->t; a.y0 = d->y0; a.dosage = d->dosage; a.dose_times = d->dose_times; a.theta = d->theta;
  a.w1 = d->w1; a.b1 = d->b1; a.h = d->h; a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.partials = (float*)d->workspace; a.status = d->status;
  a.B = d->batch; a.T = d->n_times; a.K = d->n_dose; a.perturb = d->perturb;
  a.ppw = patients_per_wave(d->batch, lpp);
  return a;
}

// what hode_rk_fwd / hode_rk_bwd check before they choose a kernel
static int check_rk(const hode_solve_desc* d, bool bwd) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE && d->rhs_kind != HODE_RHS_ROCHE_ABLATE)
    return fail(HODE_E_UNSUPPORTED, "rhs_kind %d is not handled by the fixed-grid Roche kernels", d->rhs_kind);
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "unknown fixed-grid method %d", d->method);
  if (d->batch <= 0 || d->n_times <= 0 || d->latent_dim < 4 || d->n_dose < 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d latent_dim=%d n_dose=%d", d->batch, d->n_times,
                      d->latent_dim, d->n_dose);
  if (!d->t || !d->y0 || !d->dosage || !d->theta || !d->h || (d->n_dose > 0 && !d->dose_times))
    return fail(HODE_E_NULL, "t / y0 / dosage / dose_times / theta / h must be non-NULL");
  if (d->latent_dim > 4 && (!d->w1 || !d->b1)) return fail(HODE_E_NULL, "w1 / b1 required when latent_dim > 4");
  if (bwd && (!d->grad_h || !d->grad_y0)) return fail(HODE_E_NULL, "grad_h / grad_y0 required by the backward");
  if (d->latent_dim % 4 == 0) {
    uintptr_t m = (uintptr_t)d->y0 | (uintptr_t)d->h;
    if (bwd) m |= (uintptr_t)d->grad_h | (uintptr_t)d->grad_y0;
    if (m & 15) return fail(HODE_E_ALIGN, "y0 / h / grad_h / grad_y0 must be 16-byte aligned");
  }
  return 0;
}


// HODE_FLAG_OVERWRITE_GRADS for the layouts whose fold accumulates: clear the outputs first
static int rk_clear_grads(const hode_solve_desc* d, hipStream_t s) {
  const size_t M = d->latent_dim - 4;
  if (d->grad_w1) if (int e = hip_fail(hipMemsetAsync(d->grad_w1, 0, M * d->latent_dim * sizeof(float), s), "grad_w1 clear")) return e;
  if (d->grad_b1) if (int e = hip_fail(hipMemsetAsync(d->grad_b1, 0, M * sizeof(float), s), "grad_b1 clear")) return e;
  if (d->grad_theta) if (int e = hip_fail(hipMemsetAsync(d->grad_theta, 0, kNTheta * sizeof(float), s), "grad_theta clear")) return e;
  return 0;
}

// fold the per-wave partial rows the lane kernels of layout `lpp` left in the workspace into grad_w1 / grad_b1 / grad_theta
static int rk_fold(const hode_solve_desc* d, int lpp, hipStream_t s) {
  const int M = d->latent_dim - 4;
  return launch_fold_partials((const float*)d->workspace, n_waves_for(d->batch, lpp), n_partials(d), M * d->latent_dim, M,
                              d->grad_w1, d->grad_b1, d->grad_theta, d->need_theta_grad, s);
}

}  // namespace hode
