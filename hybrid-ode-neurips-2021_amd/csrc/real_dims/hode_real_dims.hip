// C-ABI entry points of libhode_real_dims.so (include/hode_real_dims.h): the real-data hybrid rhs (HODE_RHS_ROCHE_REAL) on
// the matrix cores at the latent sizes 5 .. 20 -- this library's refusals on top of the checks, the workspace layout and
// the dispatch of ../hode_real_side_host.hpp.  The kernels (hode_real_dims_ht.hip) take M = latent_dim - 4 at run time; size 20
// is accepted so that it can be held against libhode.so's M = 16 kernels, which stay the ones the bindings use there.
// This library exists because libhode.so's set of kernel symbols is pinned.
#include <hip/hip_runtime.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "hode_real_dims.hpp"

namespace {

using hode::fail;

// where the refusals point to libhode.so for what is not served here
const hode::RealSide kSide{"real dims", HODE_REAL_DIMS_TEXT, hode::kRealDimsMinLatent, hode::kRealDimsMaxLatent, hode::kRealDimsMaxHidden,
                           "; " HODE_REAL_DIMS_LIBHODE_TEXT, "; " HODE_REAL_DIMS_LIBHODE_TEXT " at any hidden_dim, one patient per lane",
                           "; " HODE_REAL_DIMS_LIBHODE_TEXT " one patient per lane"};

#define HODE_REAL_DIMS_LAUNCH(n) hode::real_dims_launch_ht##n,
constexpr decltype(&hode::real_dims_launch_ht1) kLaunch[] = {HODE_REAL_SIDE_HTS(HODE_REAL_DIMS_LAUNCH)};
#undef HODE_REAL_DIMS_LAUNCH

// what every entry checks first: the descriptor itself, the rhs kind, the two sizes and lanes_per_patient
int check_domain(const hode_solve_desc* d) {
  if (int e = hode::real_side_check_domain(kSide, d)) return e;
  return hode::real_side_check_lanes(kSide, d);
}

hode::RealSideLayout layout(const hode_solve_desc* d, bool bwd) { return hode::real_side_layout(d, bwd, hode::real_side_blocks(d->batch)); }

int check(const hode_solve_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (int e = hode::real_side_check_method(kSide, d)) return e;
  if (int e = hode::real_side_check_sizes(kSide, d)) return e;
  if (int e = hode::real_side_check_pointers(d, bwd)) return e;
  if (bwd && !d->grad_w1)
    return fail(HODE_E_UNSUPPORTED, "real dims: grad_w1 is NULL -- the operand-tape mode is not built here (libhode.so has it at latent_dim 4 and 20), the backward accumulates the flat weight gradient on chip");
  return hode::real_side_check_workspace(d, layout(d, bwd).total);
}

int solve(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (int e = check(d, bwd)) return e;
  const hode::RealArgs a = hode::real_side_args(d, d->y0, d->dosage, d->w1, d->h, layout(d, bwd), bwd);
  return hode::real_side_launch(kLaunch, a, hode::real_side_blocks(d->batch), bwd ? d->grad_theta : nullptr, s, d->method, bwd, a,
                                d->latent_dim - 4, d->grad_w1, s);
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
