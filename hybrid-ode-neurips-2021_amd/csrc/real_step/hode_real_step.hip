// C-ABI entry points of libhode_real_step.so (include/hode_real_step.h): the one-step-ahead solve of the real-data hybrid
// rhs (HODE_RHS_ROCHE_REAL) on the matrix cores at the latent sizes 5 .. 20 -- this library's refusals on top of the checks
// of ../hode_real_side_host.hpp, the rule that cuts the intervals into runs, the sub-step region of the shared workspace
// layout, the dose-table prelude and the shared dispatch.  The kernels (hode_real_step_ht.hip) take M = latent_dim - 4 at
// run time.
#include <hip/hip_runtime.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "hode_real_step.hpp"

namespace hode {

// The dose table of every patient, written exactly once per launch sequence: one lane per patient, the recurrence of
// real_dose_table over the Ta action rows.  The solve kernels that follow on the stream only read it.
__global__ __launch_bounds__(64) void real_step_dose_kernel(RealArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p < a.B) real_dose_table(a, p, a.theta[1]);
}

}  // namespace hode

namespace {

using hode::fail;

const hode::RealSide kSide = [] {
  hode::RealSide side{"real step", HODE_REAL_STEP_TEXT, hode::kRealStepMinLatent, hode::kRealStepMaxLatent, hode::kRealStepMaxHidden};
  side.n_times_note = " (intervals)";
  return side;
}();

#define HODE_REAL_STEP_LAUNCH(n) hode::real_step_launch_ht##n,
constexpr decltype(&hode::real_step_launch_ht1) kLaunch[] = {HODE_REAL_SIDE_HTS(HODE_REAL_STEP_LAUNCH)};
#undef HODE_REAL_STEP_LAUNCH

// what every entry checks first: the descriptor itself, the rhs kind, the sizes and lanes_per_patient
int check_domain(const hode_solve_desc* d) {
  if (int e = hode::real_side_check_domain(kSide, d)) return e;
  if (d->n_dose < 1 || d->n_dose > hode::kRealStepMaxSub)
    return fail(HODE_E_UNSUPPORTED, "real step: %d solver steps per interval (n_dose) are not served (have " HODE_REAL_STEP_TEXT ")", d->n_dose);
  return hode::real_side_check_lanes(kSide, d);
}

int check_sizes(const hode_solve_desc* d) {
  if (int e = hode::real_side_check_sizes(kSide, d)) return e;
  if (d->max_steps < 0) return fail(HODE_E_SIZE, "bad sizes: max_steps=%d (intervals per wave; 0 = the library chooses)", d->max_steps);
  return 0;
}

// C: forced by the caller, or the run length with the least work per SIMD.  The kernels run one wave per SIMD
// (amdgpu_waves_per_eu(1, 1)), so a grid of W waves takes ceil(W / 1 024) rounds, and a round costs C intervals plus a wave's
// fixed cost (weights in, partial block out), measured at about two intervals' worth.  Ties go to the
// shorter run; a problem that fits one round gets C = 1.
int intervals_per_wave(const hode_solve_desc* d) {
  const long N = d->n_times;
  if (d->max_steps > 0) return (int)(d->max_steps < N ? d->max_steps : N);
  const long blocks = (long)hode::real_side_blocks(d->batch);
  long best = 1, best_cost = -1;
  for (long c = 1; c <= N; ++c) {
    const long waves = blocks * ((N + c - 1) / c);
    const long cost = ((waves + hode::kRealStepSimds - 1) / hode::kRealStepSimds) * (c + hode::kRealStepWaveCost);
    if (best_cost < 0 || cost < best_cost) { best = c; best_cost = cost; }
  }
  return (int)best;
}

size_t n_waves(const hode_solve_desc* d) {
  const size_t c = (size_t)intervals_per_wave(d);
  return hode::real_side_blocks(d->batch) * (((size_t)d->n_times + c - 1) / c);
}

// the shared layout with the sub-step states [N][S - 1][B][D] of a backward as its extra region
hode::RealSideLayout layout(const hode_solve_desc* d, bool bwd) {
  return hode::real_side_layout(d, bwd, n_waves(d),
                                (size_t)d->n_times * (size_t)(d->n_dose - 1) * (size_t)d->batch * (size_t)d->latent_dim * sizeof(float));
}

int check(const hode_solve_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (int e = hode::real_side_check_method(kSide, d)) return e;
  if (int e = check_sizes(d)) return e;
  if (int e = hode::real_side_check_pointers(d, bwd)) return e;
  if (bwd && !d->grad_w1)
    return fail(HODE_E_UNSUPPORTED, "real step: grad_w1 is NULL -- there is no operand-tape mode here, the backward accumulates the flat weight gradient on chip");
  return hode::real_side_check_workspace(d, layout(d, bwd).total);
}

int solve(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (int e = check(d, bwd)) return e;
  const hode::RealSideLayout L = layout(d, bwd);
  hode::RealArgs a = hode::real_side_args(d, d->y0, d->dosage, d->w1, d->h, L, bwd);
  a.T = d->n_times + 1;  // rows of h: the padding row and one per interval
  const hode::RealStepGeom geo{d->n_times, d->n_dose, intervals_per_wave(d), (float*)((char*)d->workspace + (bwd ? L.extra : L.dose))};
  hipLaunchKernelGGL(hode::real_step_dose_kernel, dim3((d->batch + 63) / 64), dim3(64), 0, s, a);
  if (int e = hode::hip_fail(hipGetLastError(), "real step dose-table launch")) return e;
  return hode::real_side_launch(kLaunch, a, n_waves(d), bwd ? d->grad_theta : nullptr, s, d->method, bwd, a, geo, d->latent_dim - 4,
                                d->grad_w1, s);
}

}  // namespace

extern "C" int hode_real_step_version(void) { return HODE_REAL_STEP_ABI_VERSION; }

extern "C" const char* hode_real_step_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_real_step_workspace_bytes(const hode_solve_desc* d, int which) {
  if (check_domain(d)) return 0;
  if (which != HODE_WS_RK_FWD && which != HODE_WS_RK_BWD) return 0;
  if (check_sizes(d)) return 0;
  return layout(d, which == HODE_WS_RK_BWD).total;
}

extern "C" int hode_real_step_intervals_per_wave(const hode_solve_desc* d) {
  if (check_domain(d) || check_sizes(d)) return 0;
  return intervals_per_wave(d);
}

extern "C" int hode_real_step_rk_fwd(const hode_solve_desc* d, void* stream) { return solve(d, false, (hipStream_t)stream); }

extern "C" int hode_real_step_rk_bwd(const hode_solve_desc* d, void* stream) { return solve(d, true, (hipStream_t)stream); }
