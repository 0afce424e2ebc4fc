// C-ABI entry points of libhode.so (declared in include/hode.h): argument checks, variant selection, launches.
#include <stdlib.h>

#include "hode_error_state.hpp"  // hode::fail / hip_fail and the message behind hode_last_error_string: defined here, once
#include "hode_host.hpp"
#include "hode_rk_host.hpp"  // the lane kernels' host code (grid, layout rule, fold, checks): defined here, once
#include "hode_roche.hpp"

namespace {

using hode::choose_lpp;
using hode::n_partials;
using hode::n_waves_for;

using hode::check_rk;
using hode::RkArgs;
using hode::RkLaunch;

RkArgs make_args(const hode_solve_desc* d) { return hode::rk_make_args(d, choose_lpp(d)); }

// lanes_per_patient == 16 selects the MFMA layout (hode_rk_mf.hip) where it exists for the dimension
bool use_mf(const hode_solve_desc* d) {
  if (!hode::mf_supported(d)) return false;
  if (d->lanes_per_patient == 16) return true;
  if (d->lanes_per_patient != 0) return false;
  // measured at 10 000 patients (T=100, D=12, rk4): MFMA layout fwd 118 us / bwd 313 us vs quad layout 104 / 339 -- a
  // wash (the 3 dependent 16x16x4 MFMAs + hazard nops cost as much latency as the 24 fmas they replace), so the quad
  // layout stays the default and the MFMA layout is opt-in
  return false;
}

// lanes_per_patient == 48 selects the wave-specialised split layout (hode_rk_split.hip); it is also the default for the
// dimensions it is built for (lanes_per_patient == 4 forces the quad layout)
bool use_split(const hode_solve_desc* d, bool bwd) {
  if (!hode::split_supported(d)) return false;
  if (bwd && d->n_times < 2) return false;
  if (d->lanes_per_patient == 48) return true;
  if (d->lanes_per_patient != 0) return false;
  // default wherever it exists: measured at 10 000 patients (T=100, D=12, rk4) fwd 70 us / bwd 161 us vs 104 / 339 us
  // for the quad layout; it also issues fewer wave-instructions per patient (4.1 vs 7.3 per rhs), so it keeps winning
  // once every SIMD is busy
  return true;
}

int dispatch_dim(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (use_split(d, bwd)) return bwd ? hode::split_rk_bwd(d, s) : hode::split_rk_fwd(d, s);
  if (use_mf(d)) return hode::mf_rk(d, bwd, s);
  RkLaunch L;
  L.method = d->method;
  L.lpp = choose_lpp(d);
  L.ablate = d->rhs_kind == HODE_RHS_ROCHE_ABLATE;
  L.bwd = bwd;
  L.need_th = d->need_theta_grad != 0;
  const RkArgs a = make_args(d);
  switch (d->latent_dim) {
    case 4: return hode::rk_dispatch_d4(L, a, s);
    case 6: return hode::rk_dispatch_d6(L, a, s);
    case 8: return hode::rk_dispatch_d8(L, a, s);
    case 12: return hode::rk_dispatch_d12(L, a, s);
    case 20: return hode::rk_dispatch_d20(L, a, s);
  }
  return hode::fail(HODE_E_UNSUPPORTED, "latent_dim %d has no compiled kernel (have 4, 6, 8, 12, 20)", d->latent_dim);
}

}  // namespace

extern "C" size_t hode_dopri5_workspace_bytes(const hode_solve_desc* d);  // hode_dopri5.hip

extern "C" int hode_version(void) { return HODE_ABI_VERSION; }

extern "C" const char* hode_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_workspace_bytes(const hode_solve_desc* d, int which) {
  if (!d || d->struct_size != sizeof(hode_solve_desc)) return 0;
  if (d->rhs_kind == HODE_RHS_NEURAL && (which == HODE_WS_RK_FWD || which == HODE_WS_RK_BWD))
    return hode::neural_workspace_bytes(d, which == HODE_WS_RK_BWD);
  if (d->rhs_kind == HODE_RHS_ROCHE_REAL && (which == HODE_WS_RK_FWD || which == HODE_WS_RK_BWD))
    return hode::real_workspace_bytes(d, which == HODE_WS_RK_BWD);
  if ((d->rhs_kind == HODE_RHS_NEURAL_REAL || d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND) &&
      (which == HODE_WS_RK_FWD || which == HODE_WS_RK_BWD))
    return hode::neural_real_workspace_bytes(d, which == HODE_WS_RK_BWD);
  switch (which) {
    case HODE_WS_RK_FWD:  // only the split layout's tape (HODE_FLAG_TAPE): the buffer hode_rk_bwd will be handed again
      return ((d->flags & HODE_FLAG_TAPE) && use_split(d, false) && use_split(d, true)) ? hode::split_workspace_bytes(d) : 0;
    case HODE_WS_RK_BWD:
      if (use_split(d, true)) return hode::split_workspace_bytes(d);
      if (use_mf(d)) return hode::mf_workspace_bytes(d);
      return (size_t)n_waves_for(d->batch, choose_lpp(d)) * n_partials(d) * sizeof(float);
    case HODE_WS_DOPRI5_FWD:
    case HODE_WS_DOPRI5_BWD: return hode_dopri5_workspace_bytes(d);
    default: return 0;
  }
}

extern "C" int hode_rk_fwd(const hode_solve_desc* d, void* stream) {
  if (d && d->struct_size == sizeof(hode_solve_desc) && d->rhs_kind == HODE_RHS_NEURAL)
    return hode::neural_rk(d, false, (hipStream_t)stream);
  if (d && d->struct_size == sizeof(hode_solve_desc) && d->rhs_kind == HODE_RHS_ROCHE_REAL)
    return hode::real_rk(d, false, (hipStream_t)stream);
  if (d && d->struct_size == sizeof(hode_solve_desc) &&
      (d->rhs_kind == HODE_RHS_NEURAL_REAL || d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND))
    return hode::neural_real_rk(d, false, (hipStream_t)stream);
  if (int e = check_rk(d, false)) return e;
  const size_t need = hode_workspace_bytes(d, HODE_WS_RK_FWD);
  if (need && (!d->workspace || d->workspace_bytes < need))
    return hode::fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B (HODE_FLAG_TAPE)", d->workspace_bytes, need);
  return dispatch_dim(d, false, (hipStream_t)stream);
}

extern "C" int hode_rk_bwd(const hode_solve_desc* d, void* stream) {
  if (d && d->struct_size == sizeof(hode_solve_desc) &&
      (d->rhs_kind == HODE_RHS_NEURAL_REAL || d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND))
    return hode::neural_real_rk(d, true, (hipStream_t)stream);
  if (d && d->struct_size == sizeof(hode_solve_desc) &&
      (d->rhs_kind == HODE_RHS_NEURAL || d->rhs_kind == HODE_RHS_ROCHE_REAL)) {
    if (d->flags & HODE_FLAG_OVERWRITE_GRADS)
      return hode::fail(HODE_E_UNSUPPORTED, "HODE_FLAG_OVERWRITE_GRADS is only implemented for the ROCHE rhs kinds");
    return d->rhs_kind == HODE_RHS_NEURAL ? hode::neural_rk(d, true, (hipStream_t)stream)
                                          : hode::real_rk(d, true, (hipStream_t)stream);
  }
  if (int e = check_rk(d, true)) return e;
  const size_t need = hode_workspace_bytes(d, HODE_WS_RK_BWD);
  if (!d->workspace || d->workspace_bytes < need)
    return hode::fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  if ((d->flags & HODE_FLAG_OVERWRITE_GRADS) && !use_split(d, true)) {
    // the split layout's fold stores directly; the other layouts accumulate, so clear the outputs first
    if (int e = hode::rk_clear_grads(d, s)) return e;
  }
  if (int e = dispatch_dim(d, true, s)) return e;
  if (use_split(d, true) || use_mf(d)) return 0;  // these layouts fold their own partials
  if (d->flags & HODE_FLAG_SKIP_FOLD) return 0;
  return hode::rk_fold(d, choose_lpp(d), s);
}
