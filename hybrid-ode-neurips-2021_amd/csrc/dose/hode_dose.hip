// C-ABI entry points of libhode_dose.so (include/hode_dose.h): the domain check with this library's refusals, the
// workspace size, the kernels' arguments and the launch (sweep + fixed-order fold).  The kernels are instantiated per
// latent size by hode_dose_dim.hip.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include "../hode_side_error.hpp"
#include "../hode_rk_host.hpp"  // patients_per_wave / n_waves_for / fold_partials_kernel / launch_fold_partials: once for this library
#include "hode_dose_kernels.hpp"

// hode_host.hpp declares these for the shared host code (launch_fold_partials reports through hip_fail); this library's
// message is hode_side's
namespace hode {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(hode_side::g_err, sizeof(hode_side::g_err), fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t e, const char* what) { return hode_side::launch_fail(e, what); }
}  // namespace hode

namespace {

using hode::DoseArgs;
using hode::DoseLaunch;
using hode_side::fail;

#define HODE_DOSE_SIZES_TEXT "latent_dim 4, 6, 8, 12 with HODE_RHS_ROCHE / HODE_RHS_ROCHE_ABLATE, methods euler / midpoint / rk4"

size_t al256(size_t x) { return (x + 255) / 256 * 256; }
int n_waves(const hode_dose_desc* d) { return hode::n_waves_for(d->batch, 1); }
int n_partials(const hode_dose_desc* d) { return hode::n_partials(d->latent_dim); }
size_t workspace_bytes(const hode_dose_desc* d) { return al256((size_t)n_waves(d) * n_partials(d) * sizeof(float)); }

// what every entry checks first: the descriptor itself, the rhs kind, the method and the sizes
int check_domain(const hode_dose_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_dose_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_dose_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE && d->rhs_kind != HODE_RHS_ROCHE_ABLATE)
    return fail(HODE_E_UNSUPPORTED, "dose gradient: rhs_kind %d is not served here (have " HODE_DOSE_SIZES_TEXT ")", d->rhs_kind);
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "dose gradient: unknown fixed-grid method %d (have " HODE_DOSE_SIZES_TEXT ")", d->method);
  if (d->latent_dim != 4 && d->latent_dim != 6 && d->latent_dim != 8 && d->latent_dim != 12)
    return fail(HODE_E_UNSUPPORTED, "dose gradient: latent_dim %d has no compiled kernel (have " HODE_DOSE_SIZES_TEXT ")", d->latent_dim);
  if (d->batch <= 0 || d->n_times <= 0 || d->n_dose < 1)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d n_dose=%d (each must be >= 1)", d->batch, d->n_times, d->n_dose);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "dose gradient: flags %d (have none)", d->flags);
  return 0;
}

int check(const hode_dose_desc* d) {
  if (int e = check_domain(d)) return e;
  if (!d->t || !d->h || !d->dosage || !d->dose_times || !d->theta)
    return fail(HODE_E_NULL, "t / h / dosage / dose_times / theta must be non-NULL");
  if (d->latent_dim > 4 && (!d->w1 || !d->b1)) return fail(HODE_E_NULL, "w1 / b1 required when latent_dim > 4");
  if (!d->grad_h || !d->grad_y0 || !d->grad_dosage) return fail(HODE_E_NULL, "grad_h / grad_y0 / grad_dosage required");
  if (d->latent_dim > 4 && (!d->grad_w1 || !d->grad_b1)) return fail(HODE_E_NULL, "grad_w1 / grad_b1 required when latent_dim > 4");
  if (d->need_theta_grad && !d->grad_theta) return fail(HODE_E_NULL, "grad_theta required with need_theta_grad");
  if (d->latent_dim % 4 == 0) {  // the refusals of check_rk: float4 rows
    const uintptr_t m = (uintptr_t)d->h | (uintptr_t)d->grad_h | (uintptr_t)d->grad_y0;
    if (m & 15) return fail(HODE_E_ALIGN, "h / grad_h / grad_y0 must be 16-byte aligned (latent_dim %d)", d->latent_dim);
  }
  const size_t need = workspace_bytes(d);
  if (!d->workspace || d->workspace_bytes < need)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B (batch=%d latent_dim=%d)", d->workspace_bytes, need, d->batch,
                d->latent_dim);
  return 0;
}

DoseArgs make_args(const hode_dose_desc* d) {
  DoseArgs a{};
  a.rk.t = d->t; a.rk.y0 = d->h; a.rk.dosage = d->dosage; a.rk.dose_times = d->dose_times; a.rk.theta = d->theta;
  a.rk.w1 = d->w1; a.rk.b1 = d->b1; a.rk.h = const_cast<float*>(d->h); a.rk.grad_h = d->grad_h; a.rk.grad_y0 = d->grad_y0;
  a.rk.partials = (float*)d->workspace; a.rk.status = d->status;
  a.rk.B = d->batch; a.rk.T = d->n_times; a.rk.K = d->n_dose; a.rk.perturb = d->perturb ? 1 : 0;
  a.rk.ppw = hode::patients_per_wave(d->batch, 1);
  a.grad_dosage = d->grad_dosage;
  return a;
}

}  // namespace

extern "C" int hode_dose_version(void) { return HODE_DOSE_ABI_VERSION; }

extern "C" const char* hode_dose_last_error_string(void) { return hode_side::g_err; }

extern "C" size_t hode_dose_workspace_bytes(const hode_dose_desc* d) {
  if (check_domain(d)) return 0;
  return workspace_bytes(d);
}

extern "C" int hode_dose_bwd(const hode_dose_desc* d, void* stream) {
  if (int e = check(d)) return e;
  hipStream_t s = (hipStream_t)stream;
  const DoseArgs a = make_args(d);
  const DoseLaunch L{d->method, n_waves(d), d->rhs_kind == HODE_RHS_ROCHE_ABLATE, d->need_theta_grad != 0};
  hipError_t e;
  switch (d->latent_dim) {
    case 4: e = hode::dose_launch_d4(L, a, s); break;
    case 6: e = hode::dose_launch_d6(L, a, s); break;
    case 8: e = hode::dose_launch_d8(L, a, s); break;
    case 12: e = hode::dose_launch_d12(L, a, s); break;
    default: return check_domain(d);
  }
  if (int err = hode_side::launch_fail(e, "dose-gradient sweep launch")) return err;
  const int M = d->latent_dim - 4;
  return hode::launch_fold_partials((const float*)d->workspace, n_waves(d), n_partials(d), M * d->latent_dim, M, d->grad_w1,
                                    d->grad_b1, d->grad_theta, d->need_theta_grad, s);
}
