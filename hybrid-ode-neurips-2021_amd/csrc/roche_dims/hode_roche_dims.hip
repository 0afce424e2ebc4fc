// C-ABI entry points of libhode_roche_dims.so (include/hode_roche_dims.h): the hybrid Roche rhs at the latent sizes 5 .. 16
// that libhode.so does not hold -- the domain check with this library's refusals, the layout rule of the fixed-grid
// kernels and their launches.  The kernels are the templates libhode.so instantiates (hode_roche_dims_rk_dim.hip,
// hode_roche_dims_dp_dim.hip); the host code next to them is shared, not copied: ../hode_rk_host.hpp for the fixed grid,
// ../hode_dopri5.hip (compiled a second time, with -DHODE_ROCHE_DIMS_UNIT) for dopri5.  This library exists because
// libhode.so's set of sizes and kernel symbols is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_host.hpp"
#include "../hode_rk_host.hpp"      // grid shape, partial fold, arguments, checks of the lane kernels: defined here, once
#include "hode_roche_dims.hpp"

namespace hode {

int roche_dims_check_domain(const hode_solve_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE && d->rhs_kind != HODE_RHS_ROCHE_ABLATE)
    return fail(HODE_E_UNSUPPORTED, "roche dims: rhs_kind %d is not served here (have HODE_RHS_ROCHE = %d, HODE_RHS_ROCHE_ABLATE = %d at latent_dim " HODE_ROCHE_DIMS_TEXT ")",
                d->rhs_kind, HODE_RHS_ROCHE, HODE_RHS_ROCHE_ABLATE);
  switch (d->latent_dim) {
#define HODE_ROCHE_DIMS_CASE(n) case n:
    HODE_ROCHE_DIMS(HODE_ROCHE_DIMS_CASE)
#undef HODE_ROCHE_DIMS_CASE
    break;
    default:
      return fail(HODE_E_UNSUPPORTED, "roche dims: latent_dim %d has no compiled kernel (have " HODE_ROCHE_DIMS_TEXT "; libhode.so has 4, 6, 8, 12, 20, dopri5 4, 6, 8, 12)",
                  d->latent_dim);
  }
  if (d->lanes_per_patient != 0 && d->lanes_per_patient != 1 && d->lanes_per_patient != 4)
    return fail(HODE_E_UNSUPPORTED, "roche dims: lanes_per_patient %d (have 0, 1 and 4 at latent_dim " HODE_ROCHE_DIMS_TEXT ": there is no MFMA or split layout here)",
                d->lanes_per_patient);
  return 0;
}

}  // namespace hode

namespace {

using hode::fail;

// Layout of the fixed-grid kernels.  A patient per quad exists at every size here (ragged where (D - 4) % 4 != 0, see
// ../hode_roche.hpp).  The default per size is the layout whose rk4 forward + adjoint measured faster at 10 000 patients,
// T = 100 (profiles/roche_dims_probe.txt): the quad layout at every size but 5 -- there the single learned
// row leaves three lanes of a quad with padding only, the forwards tie (63 us) and the adjoint is 184 us against 168 us
// per lane; at 7 the quad is ahead by 7 %, at 9 .. 11 by 3 .. 30 %, and from 13 on the per-lane adjoint spills (2.2 .. 7.1 ms
// against 0.43 .. 0.50 ms).  The probe was not run at large batches: libhode.so's switch to one patient per lane at
// 131 072 patients (hode::choose_lpp) applies unchanged.
bool quad_by_default(int latent_dim) { return latent_dim != 5; }
int rk_lpp(const hode_solve_desc* d) {
  if (d->lanes_per_patient == 1) return 1;
  if (d->lanes_per_patient == 4) return 4;
  if (!quad_by_default(d->latent_dim)) return 1;
  return d->batch >= 131072 ? 1 : 4;
}

int rk_dispatch(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  hode::RkLaunch L;
  L.method = d->method;
  L.lpp = rk_lpp(d);
  L.ablate = d->rhs_kind == HODE_RHS_ROCHE_ABLATE;
  L.bwd = bwd;
  L.need_th = d->need_theta_grad != 0;
  const hode::RkArgs a = hode::rk_make_args(d, L.lpp);
  switch (d->latent_dim) {
#define HODE_ROCHE_DIMS_CASE(n) case n: return hode::roche_dims_rk_dispatch_d##n(L, a, s);
    HODE_ROCHE_DIMS(HODE_ROCHE_DIMS_CASE)
#undef HODE_ROCHE_DIMS_CASE
  }
  return hode::roche_dims_check_domain(d);
}

size_t rk_bwd_bytes(const hode_solve_desc* d) {
  return (size_t)hode::n_waves_for(d->batch, rk_lpp(d)) * hode::n_partials(d) * sizeof(float);
}

int check(const hode_solve_desc* d, bool bwd) {
  if (int e = hode::roche_dims_check_domain(d)) return e;
  if (int e = hode::check_rk(d, bwd)) return e;
  const int known = bwd ? (HODE_FLAG_OVERWRITE_GRADS | HODE_FLAG_SKIP_FOLD) : 0;
  if (d->flags & ~known)
    return fail(HODE_E_UNSUPPORTED, "roche dims: flags %d (the fixed-grid %s honours %d only: no layout here keeps a stage tape)", d->flags,
                bwd ? "backward" : "forward", known);
  return 0;
}

}  // namespace

extern "C" int hode_roche_dims_version(void) { return HODE_ROCHE_DIMS_ABI_VERSION; }

extern "C" const char* hode_roche_dims_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_roche_dims_workspace_bytes(const hode_solve_desc* d, int which) {
  if (hode::roche_dims_check_domain(d)) return 0;
  switch (which) {
    case HODE_WS_RK_BWD: return rk_bwd_bytes(d);
    case HODE_WS_DOPRI5_FWD:
    case HODE_WS_DOPRI5_BWD: return hode::roche_dims_dopri5_workspace_bytes(d);
    default: return 0;  // HODE_WS_RK_FWD: no layout here keeps a stage tape
  }
}

extern "C" int hode_roche_dims_rk_fwd(const hode_solve_desc* d, void* stream) {
  if (int e = check(d, false)) return e;
  return rk_dispatch(d, false, (hipStream_t)stream);
}

extern "C" int hode_roche_dims_rk_bwd(const hode_solve_desc* d, void* stream) {
  if (int e = check(d, true)) return e;
  const size_t need = rk_bwd_bytes(d);
  if (!d->workspace || d->workspace_bytes < need)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  if (d->flags & HODE_FLAG_OVERWRITE_GRADS)
    if (int e = hode::rk_clear_grads(d, s)) return e;
  if (int e = rk_dispatch(d, true, s)) return e;
  if (d->flags & HODE_FLAG_SKIP_FOLD) return 0;
  return hode::rk_fold(d, rk_lpp(d), s);
}
