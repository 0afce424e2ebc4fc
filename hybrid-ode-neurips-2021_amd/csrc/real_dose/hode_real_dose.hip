// C-ABI entry points of libhode_real_dose.so (include/hode_real_dose.h): the adjoint of the chained fixed-grid solve of the
// real-data hybrid rhs with the gradient of the dose table -- this library's refusals on top of the checks, the workspace
// layout (a backward's, as in real_dims/hode_real_dims.hip) and the dispatch of ../hode_real_side_host.hpp.  The kernels
// (hode_real_dose_ht.hip) take M = latent_dim - 4 at run time.
#include <hip/hip_runtime.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "hode_real_dose.hpp"

namespace {

using hode::fail;

const hode::RealSide kSide = [] {
  hode::RealSide side{"real dose", HODE_REAL_DOSE_TEXT, hode::kRealDoseMinLatent, hode::kRealDoseMaxLatent, hode::kRealDoseMaxHidden};
  side.method_note = " (have " HODE_REAL_DOSE_TEXT ")";
  side.sizes_note = " (each must be >= 1)";
  return side;
}();

#define HODE_REAL_DOSE_LAUNCH(n) hode::real_dose_launch_ht##n,
constexpr decltype(&hode::real_dose_launch_ht1) kLaunch[] = {HODE_REAL_SIDE_HTS(HODE_REAL_DOSE_LAUNCH)};
#undef HODE_REAL_DOSE_LAUNCH

// what every entry checks first: the descriptor itself, the two sizes, the method and the flags
int check_domain(const hode_real_dose_desc* d) {
  if (int e = hode::real_side_check_domain(kSide, d)) return e;
  if (int e = hode::real_side_check_method(kSide, d)) return e;
  return hode::real_side_check_sizes(kSide, d);
}

hode::RealSideLayout layout(const hode_real_dose_desc* d) { return hode::real_side_layout(d, true, hode::real_side_blocks(d->batch)); }

int check(const hode_real_dose_desc* d) {
  if (int e = check_domain(d)) return e;
  if (!d->t || !d->h || !d->act || !d->theta || !d->wflat || !d->grad_h)
    return fail(HODE_E_NULL, "t / h / act (dose table) / theta / wflat (flat weights) / grad_h must be non-NULL");
  if (!d->grad_y0 || !d->grad_act || !d->grad_wflat || !d->grad_theta)
    return fail(HODE_E_NULL, "grad_y0 / grad_act / grad_wflat / grad_theta required");
  return hode::real_side_check_workspace(d, layout(d).total);
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
  // h[0] is the start state: the kernels read a.h alone
  const hode::RealArgs a = hode::real_side_args(d, d->h, d->act, d->wflat, const_cast<float*>(d->h), layout(d), true);
  return hode::real_side_launch(kLaunch, a, hode::real_side_blocks(d->batch), d->grad_theta, s, d->method, a, d->latent_dim - 4,
                                d->grad_act, d->grad_wflat, s);
}
