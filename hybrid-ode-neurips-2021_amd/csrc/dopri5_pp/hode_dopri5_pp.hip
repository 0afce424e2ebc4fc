// C-ABI entry points of libhode_dopri5_pp.so (include/hode_dopri5_pp.h): the domain check with this library's refusals,
// the workspace layout, the kernels' arguments and the two launches (forward; sweep + fixed-order fold).  The kernels are
// instantiated per latent size by hode_dopri5_pp_dim.hip.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include "../hode_side_error.hpp"
#include "../hode_rk_host.hpp"  // fold_partials_kernel / launch_fold_partials: defined here, once for this library
#include "hode_dopri5_pp_kernels.hpp"

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

using hode::PpArgs;
using hode::PpLaunch;
using hode_side::fail;

#define HODE_PP_SIZES_TEXT "latent_dim 4, 6, 8, 12 with HODE_RHS_ROCHE / HODE_RHS_ROCHE_ABLATE"

size_t al256(size_t x) { return (x + 255) / 256 * 256; }
int n_waves(const hode_dopri5_pp_desc* d) { return (d->batch + hode::kPpLanes - 1) / hode::kPpLanes; }
int n_partials(const hode_dopri5_pp_desc* d) { return hode::n_partials(d->latent_dim); }
int max_attempts(const hode_dopri5_pp_desc* d) {
  if (d->max_attempts > 0) return d->max_attempts;
  const long long v = 8LL * d->max_steps + 1024;
  return (int)(v > 0x7fffffffLL ? 0x7fffffffLL : v);
}

// what every entry checks first: the descriptor itself, the rhs kind and the sizes
int check_domain(const hode_dopri5_pp_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_dopri5_pp_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_dopri5_pp_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE && d->rhs_kind != HODE_RHS_ROCHE_ABLATE)
    return fail(HODE_E_UNSUPPORTED, "per-patient dopri5: rhs_kind %d is not served here (have " HODE_PP_SIZES_TEXT ")", d->rhs_kind);
  if (d->latent_dim != 4 && d->latent_dim != 6 && d->latent_dim != 8 && d->latent_dim != 12)
    return fail(HODE_E_UNSUPPORTED, "per-patient dopri5: latent_dim %d has no compiled kernel (have " HODE_PP_SIZES_TEXT ")", d->latent_dim);
  if (d->batch <= 0 || d->n_times <= 0 || d->n_dose < 1 || d->max_steps <= 0 || d->max_attempts < 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d n_dose=%d max_steps=%d max_attempts=%d", d->batch, d->n_times,
                d->n_dose, d->max_steps, d->max_attempts);
  if (d->flags & ~HODE_FLAG_NO_TAPE) return fail(HODE_E_UNSUPPORTED, "per-patient dopri5: flags %d (have HODE_FLAG_NO_TAPE)", d->flags);
  return 0;
}

struct Layout {
  size_t partials, tape_t, tape_dt, tape_j, tape_y, total;
};
// [ per-wave gradient partials | tape_t | tape_dt | tape_j | tape_y ]; with HODE_FLAG_NO_TAPE the partials alone
Layout layout(const hode_dopri5_pp_desc* d) {
  Layout L{};
  size_t off = 0;
  L.partials = off; off = al256(off + (size_t)n_waves(d) * n_partials(d) * sizeof(float));
  const size_t cells = (d->flags & HODE_FLAG_NO_TAPE) ? 0 : (size_t)d->max_steps * (size_t)d->batch;
  L.tape_t = off; off = al256(off + cells * sizeof(double));
  L.tape_dt = off; off = al256(off + cells * sizeof(double));
  L.tape_j = off; off = al256(off + cells * sizeof(int2));
  L.tape_y = off; off = al256(off + cells * (size_t)d->latent_dim * sizeof(float));
  L.total = off;
  return L;
}

int check(const hode_dopri5_pp_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (!(d->rtol > 0) || !(d->atol >= 0)) return fail(HODE_E_SIZE, "rtol must be > 0 and atol >= 0");
  if (!d->t || !d->y0 || !d->dosage || !d->dose_times || !d->theta || !d->h)
    return fail(HODE_E_NULL, "t / y0 / dosage / dose_times / theta / h must be non-NULL");
  if (d->latent_dim > 4 && (!d->w1 || !d->b1)) return fail(HODE_E_NULL, "w1 / b1 required when latent_dim > 4");
  if (!d->status || !d->n_accepted || !d->n_rejected || !d->patient_status)
    return fail(HODE_E_NULL, "status / n_accepted / n_rejected / patient_status must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0)) return fail(HODE_E_NULL, "grad_h / grad_y0 required by the backward");
  if (bwd && d->latent_dim > 4 && (!d->grad_w1 || !d->grad_b1)) return fail(HODE_E_NULL, "grad_w1 / grad_b1 required when latent_dim > 4");
  if (bwd && d->need_theta_grad && !d->grad_theta) return fail(HODE_E_NULL, "grad_theta required with need_theta_grad");
  if (bwd && (d->flags & HODE_FLAG_NO_TAPE))
    return fail(HODE_E_UNSUPPORTED, "the forward ran with HODE_FLAG_NO_TAPE: there is no tape to sweep");
  uintptr_t m = (uintptr_t)d->y0 | (uintptr_t)d->h | (uintptr_t)d->workspace;
  if (bwd) m |= (uintptr_t)d->grad_h | (uintptr_t)d->grad_y0;
  if (m & 15) return fail(HODE_E_ALIGN, "y0 / h / grad_h / grad_y0 / workspace must be 16-byte aligned");
  const Layout L = layout(d);
  if (!d->workspace || d->workspace_bytes < L.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, L.total);
  return 0;
}

PpArgs make_args(const hode_dopri5_pp_desc* d, const Layout& L) {
  PpArgs a{};
  char* ws = (char*)d->workspace;
  a.t = d->t; a.y0 = d->y0; a.dosage = d->dosage; a.dose_times = d->dose_times; a.theta = d->theta;
  a.w1 = d->w1; a.b1 = d->b1; a.h = d->h;
  a.status = d->status; a.n_acc = d->n_accepted; a.n_rej = d->n_rejected; a.pstatus = d->patient_status;
  a.grad_partials = (float*)(ws + L.partials);
  a.tape_t = (double*)(ws + L.tape_t);
  a.tape_dt = (double*)(ws + L.tape_dt);
  a.tape_j = (int2*)(ws + L.tape_j);
  a.tape_y = (float*)(ws + L.tape_y);
  a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.B = d->batch; a.T = d->n_times; a.K = d->n_dose;
  a.max_steps = d->max_steps;
  a.max_attempts = max_attempts(d);
  a.no_tape = (d->flags & HODE_FLAG_NO_TAPE) ? 1 : 0;
  a.rtol = (float)d->rtol; a.atol = (float)d->atol;
  return a;
}

int launch(const hode_dopri5_pp_desc* d, const PpLaunch& L, const PpArgs& a, hipStream_t s) {
  hipError_t e;
  switch (d->latent_dim) {
    case 4: e = hode::pp_launch_d4(L, a, s); break;
    case 6: e = hode::pp_launch_d6(L, a, s); break;
    case 8: e = hode::pp_launch_d8(L, a, s); break;
    case 12: e = hode::pp_launch_d12(L, a, s); break;
    default: return check_domain(d);
  }
  return hode_side::launch_fail(e, L.bwd ? "per-patient dopri5 sweep launch" : "per-patient dopri5 forward launch");
}

}  // namespace

extern "C" int hode_dopri5_pp_version(void) { return HODE_DOPRI5_PP_ABI_VERSION; }

extern "C" const char* hode_dopri5_pp_last_error_string(void) { return hode_side::g_err; }

extern "C" size_t hode_dopri5_pp_workspace_bytes(const hode_dopri5_pp_desc* d) {
  if (check_domain(d)) return 0;
  return layout(d).total;
}

extern "C" int hode_dopri5_pp_fwd(const hode_dopri5_pp_desc* d, void* stream) {
  if (int e = check(d, false)) return e;
  const PpArgs a = make_args(d, layout(d));
  PpLaunch L{d->rhs_kind == HODE_RHS_ROCHE_ABLATE, false, false};
  return launch(d, L, a, (hipStream_t)stream);
}

extern "C" int hode_dopri5_pp_bwd(const hode_dopri5_pp_desc* d, void* stream) {
  if (int e = check(d, true)) return e;
  hipStream_t s = (hipStream_t)stream;
  const PpArgs a = make_args(d, layout(d));
  PpLaunch L{d->rhs_kind == HODE_RHS_ROCHE_ABLATE, true, d->need_theta_grad != 0};
  if (int e = launch(d, L, a, s)) return e;
  const int M = d->latent_dim - 4;
  return hode::launch_fold_partials(a.grad_partials, n_waves(d), n_partials(d), M * d->latent_dim, M, d->grad_w1, d->grad_b1,
                                    d->grad_theta, d->need_theta_grad, s);
}

extern "C" int hode_dopri5_pp_tape_offsets(const hode_dopri5_pp_desc* d, size_t* out5) {
  if (!out5) return fail(HODE_E_NULL, "out5 is NULL");
  if (int e = check_domain(d)) return e;
  const Layout L = layout(d);
  out5[0] = L.partials; out5[1] = L.tape_t; out5[2] = L.tape_dt; out5[3] = L.tape_j; out5[4] = L.tape_y;
  return 0;
}
