// C-ABI entry points of libhode_real_dims.so (include/hode_real_dims.h): the real-data hybrid rhs (HODE_RHS_ROCHE_REAL) on
// the matrix cores at the latent sizes 5 .. 20 -- the domain check with this library's refusals, the workspace layout and
// the dispatch on the hidden-tile count.  The kernels (hode_real_dims_ht.hip) take M = latent_dim - 4 at run time; size 20
// is accepted so that it can be held against libhode.so's M = 16 kernels, which stay the ones the bindings use there.
// This library exists because libhode.so's set of kernel symbols is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_host.hpp"
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "../hode_real_args.hpp"
#include "hode_real_dims.hpp"

namespace {

using hode::fail;

size_t al256(size_t x) { return (x + 255) / 256 * 256; }
int hidden_tiles(const hode_solve_desc* d) { return (d->hidden_dim + 15) / 16; }
size_t n_waves(const hode_solve_desc* d) { return ((size_t)d->batch + 15) / 16; }

// what every entry checks first: the descriptor itself, the rhs kind, the two sizes and lanes_per_patient
int check_domain(const hode_solve_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE_REAL)
    return fail(HODE_E_UNSUPPORTED, "real dims: rhs_kind %d is not served here (have HODE_RHS_ROCHE_REAL = %d at " HODE_REAL_DIMS_TEXT ")",
                d->rhs_kind, HODE_RHS_ROCHE_REAL);
  if (d->latent_dim < hode::kRealDimsMinLatent || d->latent_dim > hode::kRealDimsMaxLatent)
    return fail(HODE_E_UNSUPPORTED, "real dims: latent_dim %d has no compiled kernel (have " HODE_REAL_DIMS_TEXT "; " HODE_REAL_DIMS_LIBHODE_TEXT ")",
                d->latent_dim);
  if (d->hidden_dim < 1 || d->hidden_dim > hode::kRealDimsMaxHidden)
    return fail(HODE_E_UNSUPPORTED, "real dims: hidden_dim %d has no compiled kernel (have " HODE_REAL_DIMS_TEXT "; " HODE_REAL_DIMS_LIBHODE_TEXT " at any hidden_dim, one patient per lane)",
                d->hidden_dim);
  if (d->lanes_per_patient != 0 && d->lanes_per_patient != 16)
    return fail(HODE_E_UNSUPPORTED, "real dims: lanes_per_patient %d (have 0 and 16 at " HODE_REAL_DIMS_TEXT ": the matrix-core layout only; " HODE_REAL_DIMS_LIBHODE_TEXT " one patient per lane)",
                d->lanes_per_patient);
  return 0;
}

struct Layout {
  size_t grads, partials, dose, total;
};
// [ per-wave weight-gradient blocks (bwd) | per-wave rows of the three scalars (bwd) | dose table (both) ]
Layout layout(const hode_solve_desc* d, bool bwd) {
  Layout L{0, 0, 0, 0};
  size_t off = 0;
  if (bwd) {
    L.grads = off; off = al256(off + n_waves(d) * hode::real_dims_partial_floats(hidden_tiles(d)) * sizeof(float));
    L.partials = off; off = al256(off + n_waves(d) * 3 * sizeof(float));
  }
  L.dose = off; off = al256(off + (size_t)2 * ((size_t)d->n_action_times + 1) * (size_t)d->batch * sizeof(float));
  L.total = off;
  return L;
}

int check(const hode_solve_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "real dims: unknown fixed-grid method %d", d->method);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "real dims: flags %d have no meaning for this solve", d->flags);
  if (d->batch <= 0 || d->n_times <= 0 || d->n_action_times <= 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d n_action_times=%d", d->batch, d->n_times, d->n_action_times);
  if (!d->t || !d->y0 || !d->dosage || !d->theta || !d->w1 || !d->h)
    return fail(HODE_E_NULL, "t / y0 / dosage (dose table) / theta / w1 (flat weights) / h must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0 || !d->grad_theta)) return fail(HODE_E_NULL, "grad_h / grad_y0 / grad_theta required");
  if (bwd && !d->grad_w1)
    return fail(HODE_E_UNSUPPORTED, "real dims: grad_w1 is NULL -- the operand-tape mode is not built here (libhode.so has it at latent_dim 4 and 20), the backward accumulates the flat weight gradient on chip");
  const Layout L = layout(d, bwd);
  if (!d->workspace || d->workspace_bytes < L.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, L.total);
  if ((uintptr_t)d->workspace & 15) return fail(HODE_E_ALIGN, "workspace must be 16-byte aligned");
  return 0;
}

int solve(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (int e = check(d, bwd)) return e;
  const Layout L = layout(d, bwd);
  char* ws = (char*)d->workspace;
  hode::RealArgs a{};
  a.t = d->t; a.y0 = d->y0; a.act = d->dosage; a.theta = d->theta; a.wflat = d->w1; a.h = d->h;
  a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.tape = bwd ? (float*)(ws + L.grads) : nullptr;
  a.partials = bwd ? (float*)(ws + L.partials) : nullptr;
  a.dose_tab = (float*)(ws + L.dose);
  a.B = d->batch; a.T = d->n_times; a.Ta = d->n_action_times; a.H = d->hidden_dim; a.perturb = d->perturb;
  const int M = d->latent_dim - 4;
  int e;
  switch (hidden_tiles(d)) {
#define HODE_REAL_DIMS_CASE(n) case n: e = hode::real_dims_launch_ht##n(d->method, bwd, a, M, d->grad_w1, s); break;
    HODE_REAL_DIMS_HTS(HODE_REAL_DIMS_CASE)
#undef HODE_REAL_DIMS_CASE
    default: return check_domain(d);
  }
  if (e || !bwd) return e;
  return hode::launch_fold_partials(a.partials, (int)n_waves(d), 3, 0, 0, nullptr, nullptr, d->grad_theta, 1, s);
}

}  // namespace

extern "C" int hode_real_dims_version(void) { return HODE_REAL_DIMS_ABI_VERSION; }

extern "C" const char* hode_real_dims_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_real_dims_workspace_bytes(const hode_solve_desc* d, int which) {
  if (check_domain(d)) return 0;
  if (which != HODE_WS_RK_FWD && which != HODE_WS_RK_BWD) return 0;
  if (d->batch <= 0 || d->n_action_times <= 0) return 0;
  return layout(d, which == HODE_WS_RK_BWD).total;
}

extern "C" int hode_real_dims_rk_fwd(const hode_solve_desc* d, void* stream) { return solve(d, false, (hipStream_t)stream); }

extern "C" int hode_real_dims_rk_bwd(const hode_solve_desc* d, void* stream) { return solve(d, true, (hipStream_t)stream); }
