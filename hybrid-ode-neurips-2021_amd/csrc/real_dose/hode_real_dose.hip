// C-ABI entry points of libhode_real_dose.so (include/hode_real_dose.h): the adjoint of the chained fixed-grid solve of the
// real-data hybrid rhs with the gradient of the dose table -- the domain check with this library's refusals, the workspace
// layout (that of real_dims/hode_real_dims.hip for a backward) and the dispatch on the hidden-tile count.  The kernels
// (hode_real_dose_ht.hip) take M = latent_dim - 4 at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_host.hpp"
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "../hode_real_args.hpp"
#include "hode_real_dose.hpp"

namespace {

using hode::fail;

size_t al256(size_t x) { return (x + 255) / 256 * 256; }
int hidden_tiles(const hode_real_dose_desc* d) { return (d->hidden_dim + 15) / 16; }
size_t n_waves(const hode_real_dose_desc* d) { return ((size_t)d->batch + 15) / 16; }

// what every entry checks first: the descriptor itself, the two sizes, the method and the flags
int check_domain(const hode_real_dose_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_real_dose_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_real_dose_desc));
  if (d->latent_dim < hode::kRealDoseMinLatent || d->latent_dim > hode::kRealDoseMaxLatent)
    return fail(HODE_E_UNSUPPORTED, "real dose: latent_dim %d has no compiled kernel (have " HODE_REAL_DOSE_TEXT ")", d->latent_dim);
  if (d->hidden_dim < 1 || d->hidden_dim > hode::kRealDoseMaxHidden)
    return fail(HODE_E_UNSUPPORTED, "real dose: hidden_dim %d has no compiled kernel (have " HODE_REAL_DOSE_TEXT ")", d->hidden_dim);
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "real dose: unknown fixed-grid method %d (have " HODE_REAL_DOSE_TEXT ")", d->method);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "real dose: flags %d have no meaning for this solve", d->flags);
  if (d->batch <= 0 || d->n_times <= 0 || d->n_action_times <= 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d n_action_times=%d (each must be >= 1)", d->batch, d->n_times,
                d->n_action_times);
  return 0;
}

struct Layout {
  size_t grads, partials, dose, total;
};
// [ per-wave weight-gradient blocks | per-wave rows of the three scalars | dose table ]
Layout layout(const hode_real_dose_desc* d) {
  Layout L{0, 0, 0, 0};
  size_t off = 0;
  L.grads = off; off = al256(off + n_waves(d) * hode::real_dose_partial_floats(hidden_tiles(d)) * sizeof(float));
  L.partials = off; off = al256(off + n_waves(d) * 3 * sizeof(float));
  L.dose = off; off = al256(off + (size_t)2 * ((size_t)d->n_action_times + 1) * (size_t)d->batch * sizeof(float));
  L.total = off;
  return L;
}

int check(const hode_real_dose_desc* d) {
  if (int e = check_domain(d)) return e;
  if (!d->t || !d->h || !d->act || !d->theta || !d->wflat || !d->grad_h)
    return fail(HODE_E_NULL, "t / h / act (dose table) / theta / wflat (flat weights) / grad_h must be non-NULL");
  if (!d->grad_y0 || !d->grad_act || !d->grad_wflat || !d->grad_theta)
    return fail(HODE_E_NULL, "grad_y0 / grad_act / grad_wflat / grad_theta required");
  const Layout L = layout(d);
  if (!d->workspace || d->workspace_bytes < L.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, L.total);
  if ((uintptr_t)d->workspace & 15) return fail(HODE_E_ALIGN, "workspace must be 16-byte aligned");
  return 0;
}

}  // namespace

extern "C" int hode_real_dose_version(void) { return HODE_REAL_DOSE_ABI_VERSION; }

extern "C" const char* hode_real_dose_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_real_dose_workspace_bytes(const hode_real_dose_desc* d) {
  if (check_domain(d)) return 0;
  return layout(d).total;
}

extern "C" int hode_real_dose_bwd(const hode_real_dose_desc* d, void* stream) {
  if (int e = check(d)) return e;
  hipStream_t s = (hipStream_t)stream;
  const Layout L = layout(d);
  char* ws = (char*)d->workspace;
  hode::RealArgs a{};
  a.t = d->t; a.y0 = d->h; a.act = d->act; a.theta = d->theta; a.wflat = d->wflat; a.h = const_cast<float*>(d->h);
  a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.tape = (float*)(ws + L.grads);
  a.partials = (float*)(ws + L.partials);
  a.dose_tab = (float*)(ws + L.dose);
  a.B = d->batch; a.T = d->n_times; a.Ta = d->n_action_times; a.H = d->hidden_dim; a.perturb = d->perturb ? 1 : 0;
  const int M = d->latent_dim - 4;
  int e;
  switch (hidden_tiles(d)) {
#define HODE_REAL_DOSE_CASE(n) case n: e = hode::real_dose_launch_ht##n(d->method, a, M, d->grad_act, d->grad_wflat, s); break;
    HODE_REAL_DOSE_HTS(HODE_REAL_DOSE_CASE)
#undef HODE_REAL_DOSE_CASE
    default: return check_domain(d);
  }
  if (e) return e;
  return hode::launch_fold_partials(a.partials, (int)n_waves(d), 3, 0, 0, nullptr, nullptr, d->grad_theta, 1, s);
}
