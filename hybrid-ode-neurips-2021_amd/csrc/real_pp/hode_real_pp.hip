// C-ABI entry points of libhode_real_pp.so (include/hode_real_pp.h): dopri5 with per-patient step control for the
// real-data hybrid rhs -- this library's refusals on top of the checks, the workspace layout (a backward's with the four
// tapes as its `extra` block) and the dispatch of ../hode_real_side_host.hpp.  The kernels (hode_real_pp_ht.hip) take
// M = latent_dim - 4 at run time.
#include <hip/hip_runtime.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "hode_real_pp.hpp"

namespace {

using hode::al256;
using hode::fail;

const hode::RealSide kSide = [] {
  hode::RealSide side{"real per-patient dopri5", HODE_REAL_PP_TEXT, hode::kRealPpMinLatent, hode::kRealPpMaxLatent, hode::kRealPpMaxHidden};
  side.sizes_note = " (each must be >= 1)";
  return side;
}();

#define HODE_REAL_PP_LAUNCH(n) hode::real_pp_launch_ht##n,
constexpr decltype(&hode::real_pp_launch_ht1) kLaunch[] = {HODE_REAL_SIDE_HTS(HODE_REAL_PP_LAUNCH)};
#undef HODE_REAL_PP_LAUNCH

int max_attempts(const hode_real_pp_desc* d) {
  if (d->max_attempts > 0) return d->max_attempts;
  const long long v = 8LL * d->max_steps + 1024;
  return (int)(v > 0x7fffffffLL ? 0x7fffffffLL : v);
}

// what every entry checks first: the descriptor itself, the two sizes, the counts and the flags
int check_domain(const hode_real_pp_desc* d) {
  if (int e = hode::real_side_check_domain(kSide, d)) return e;
  if (int e = hode::real_side_check_sizes(kSide, d)) return e;
  if (d->max_steps <= 0 || d->max_attempts < 0)
    return fail(HODE_E_SIZE, "bad sizes: max_steps=%d (must be >= 1) max_attempts=%d (must be >= 0)", d->max_steps, d->max_attempts);
  if (d->flags & ~HODE_FLAG_NO_TAPE)
    return fail(HODE_E_UNSUPPORTED, "real per-patient dopri5: flags %d (have HODE_FLAG_NO_TAPE)", d->flags);
  return 0;
}

struct Tapes {
  size_t t, dt, j, y, bytes;  // offsets inside the `extra` block, and its size
};
Tapes tapes(const hode_real_pp_desc* d) {
  Tapes T{};
  const size_t cells = (d->flags & HODE_FLAG_NO_TAPE) ? 0 : (size_t)d->max_steps * (size_t)d->batch;
  size_t off = 0;
  T.t = off; off = al256(off + cells * sizeof(double));
  T.dt = off; off = al256(off + cells * sizeof(double));
  T.j = off; off = al256(off + cells * sizeof(int));
  T.y = off; off = al256(off + cells * (size_t)d->latent_dim * sizeof(float));
  T.bytes = off;
  return T;
}

hode::RealSideLayout layout(const hode_real_pp_desc* d) {
  return hode::real_side_layout(d, true, hode::real_side_blocks(d->batch), tapes(d).bytes);
}

int check(const hode_real_pp_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (!(d->rtol > 0) || !(d->atol >= 0)) return fail(HODE_E_SIZE, "rtol must be > 0 and atol >= 0");
  if (!d->t || !d->y0 || !d->act || !d->theta || !d->wflat || !d->h)
    return fail(HODE_E_NULL, "t / y0 / act (dose table) / theta / wflat (flat weights) / h must be non-NULL");
  if (!d->status || !d->n_accepted || !d->n_rejected || !d->patient_status)
    return fail(HODE_E_NULL, "status / n_accepted / n_rejected / patient_status must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0 || !d->grad_wflat || !d->grad_theta))
    return fail(HODE_E_NULL, "grad_h / grad_y0 / grad_wflat / grad_theta required by the backward");
  if (bwd && (d->flags & HODE_FLAG_NO_TAPE))
    return fail(HODE_E_UNSUPPORTED, "the forward ran with HODE_FLAG_NO_TAPE: there is no tape to sweep");
  return hode::real_side_check_workspace(d, layout(d).total);
}

hode::RealPpArgs make_args(const hode_real_pp_desc* d) {
  const hode::RealSideLayout L = layout(d);
  const Tapes T = tapes(d);
  char* ws = (char*)d->workspace;
  hode::RealPpArgs a{};
  a.r.t = d->t; a.r.y0 = d->y0; a.r.act = d->act; a.r.theta = d->theta; a.r.wflat = d->wflat; a.r.h = d->h;
  a.r.grad_h = d->grad_h; a.r.grad_y0 = d->grad_y0;
  a.r.tape = (float*)(ws + L.grads);
  a.r.partials = (float*)(ws + L.partials);
  a.r.dose_tab = (float*)(ws + L.dose);
  a.r.B = d->batch; a.r.T = d->n_times; a.r.Ta = d->n_action_times; a.r.H = d->hidden_dim; a.r.perturb = 0;
  a.status = d->status; a.n_acc = d->n_accepted; a.n_rej = d->n_rejected; a.pstatus = d->patient_status;
  a.tape_t = (double*)(ws + L.extra + T.t);
  a.tape_dt = (double*)(ws + L.extra + T.dt);
  a.tape_j = (int*)(ws + L.extra + T.j);
  a.tape_y = (float*)(ws + L.extra + T.y);
  a.max_steps = d->max_steps;
  a.max_attempts = max_attempts(d);
  a.no_tape = (d->flags & HODE_FLAG_NO_TAPE) ? 1 : 0;
  a.rtol = (float)d->rtol; a.atol = (float)d->atol;
  return a;
}

}  // namespace

extern "C" int hode_real_pp_version(void) { return HODE_REAL_PP_ABI_VERSION; }

extern "C" const char* hode_real_pp_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_real_pp_workspace_bytes(const hode_real_pp_desc* d) {
  if (check_domain(d)) return 0;
  return layout(d).total;
}

extern "C" int hode_real_pp_fwd(const hode_real_pp_desc* d, void* stream) {
  if (int e = check(d, false)) return e;
  hipStream_t s = (hipStream_t)stream;
  const hode::RealPpArgs a = make_args(d);
  return hode::real_side_launch(kLaunch, a.r, hode::real_side_blocks(d->batch), nullptr, s, false, a, d->latent_dim - 4, nullptr, s);
}

extern "C" int hode_real_pp_bwd(const hode_real_pp_desc* d, void* stream) {
  if (int e = check(d, true)) return e;
  hipStream_t s = (hipStream_t)stream;
  const hode::RealPpArgs a = make_args(d);
  return hode::real_side_launch(kLaunch, a.r, hode::real_side_blocks(d->batch), d->grad_theta, s, true, a, d->latent_dim - 4,
                                d->grad_wflat, s);
}

extern "C" int hode_real_pp_tape_offsets(const hode_real_pp_desc* d, size_t* out4) {
  if (!out4) return fail(HODE_E_NULL, "out4 is NULL");
  if (int e = check_domain(d)) return e;
  const hode::RealSideLayout L = layout(d);
  const Tapes T = tapes(d);
  out4[0] = L.extra + T.t; out4[1] = L.extra + T.dt; out4[2] = L.extra + T.j; out4[3] = L.extra + T.y;
  return 0;
}
