// C-ABI entry points of libhode_real_step.so (include/hode_real_step.h): the one-step-ahead solve of the real-data hybrid
// rhs (HODE_RHS_ROCHE_REAL) on the matrix cores at the latent sizes 5 .. 20 -- the domain check with this library's
// refusals, the rule that cuts the intervals into runs, the workspace layout, the dose-table prelude and the dispatch on
// the hidden-tile count.  The kernels (hode_real_step_ht.hip) take M = latent_dim - 4 at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_host.hpp"
#include "../hode_rk_host.hpp"      // launch_fold_partials (the three scalars' per-wave rows): defined here, once
#include "../hode_real_args.hpp"
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

size_t al256(size_t x) { return (x + 255) / 256 * 256; }
int hidden_tiles(const hode_solve_desc* d) { return (d->hidden_dim + 15) / 16; }
size_t n_blocks(const hode_solve_desc* d) { return ((size_t)d->batch + 15) / 16; }

// what every entry checks first: the descriptor itself, the rhs kind, the sizes and lanes_per_patient
int check_domain(const hode_solve_desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->rhs_kind != HODE_RHS_ROCHE_REAL)
    return fail(HODE_E_UNSUPPORTED, "real step: rhs_kind %d is not served here (have HODE_RHS_ROCHE_REAL = %d at " HODE_REAL_STEP_TEXT ")",
                d->rhs_kind, HODE_RHS_ROCHE_REAL);
  if (d->latent_dim < hode::kRealStepMinLatent || d->latent_dim > hode::kRealStepMaxLatent)
    return fail(HODE_E_UNSUPPORTED, "real step: latent_dim %d has no compiled kernel (have " HODE_REAL_STEP_TEXT ")", d->latent_dim);
  if (d->hidden_dim < 1 || d->hidden_dim > hode::kRealStepMaxHidden)
    return fail(HODE_E_UNSUPPORTED, "real step: hidden_dim %d has no compiled kernel (have " HODE_REAL_STEP_TEXT ")", d->hidden_dim);
  if (d->n_dose < 1 || d->n_dose > hode::kRealStepMaxSub)
    return fail(HODE_E_UNSUPPORTED, "real step: %d solver steps per interval (n_dose) are not served (have " HODE_REAL_STEP_TEXT ")", d->n_dose);
  if (d->lanes_per_patient != 0 && d->lanes_per_patient != 16)
    return fail(HODE_E_UNSUPPORTED, "real step: lanes_per_patient %d (have 0 and 16 at " HODE_REAL_STEP_TEXT ": the matrix-core layout only)",
                d->lanes_per_patient);
  return 0;
}

int check_sizes(const hode_solve_desc* d) {
  if (d->batch <= 0 || d->n_times <= 0 || d->n_action_times <= 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d (intervals) n_action_times=%d", d->batch, d->n_times, d->n_action_times);
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
  const long blocks = (long)n_blocks(d);
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
  return n_blocks(d) * (((size_t)d->n_times + c - 1) / c);
}

struct Layout {
  size_t grads, partials, sub, dose, total;
};
// [ per-wave weight-gradient blocks (bwd) | per-wave rows of the three scalars (bwd) | sub-step states (bwd) | dose table ]
Layout layout(const hode_solve_desc* d, bool bwd) {
  Layout L{0, 0, 0, 0, 0};
  size_t off = 0;
  if (bwd) {
    L.grads = off; off = al256(off + n_waves(d) * hode::real_step_partial_floats(hidden_tiles(d)) * sizeof(float));
    L.partials = off; off = al256(off + n_waves(d) * 3 * sizeof(float));
    L.sub = off;
    off = al256(off + (size_t)d->n_times * (size_t)(d->n_dose - 1) * (size_t)d->batch * (size_t)d->latent_dim * sizeof(float));
  }
  L.dose = off; off = al256(off + (size_t)2 * ((size_t)d->n_action_times + 1) * (size_t)d->batch * sizeof(float));
  L.total = off;
  return L;
}

int check(const hode_solve_desc* d, bool bwd) {
  if (int e = check_domain(d)) return e;
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "real step: unknown fixed-grid method %d", d->method);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "real step: flags %d have no meaning for this solve", d->flags);
  if (int e = check_sizes(d)) return e;
  if (!d->t || !d->y0 || !d->dosage || !d->theta || !d->w1 || !d->h)
    return fail(HODE_E_NULL, "t / y0 / dosage (dose table) / theta / w1 (flat weights) / h must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0 || !d->grad_theta)) return fail(HODE_E_NULL, "grad_h / grad_y0 / grad_theta required");
  if (bwd && !d->grad_w1)
    return fail(HODE_E_UNSUPPORTED, "real step: grad_w1 is NULL -- there is no operand-tape mode here, the backward accumulates the flat weight gradient on chip");
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
  a.B = d->batch; a.T = d->n_times + 1; a.Ta = d->n_action_times; a.H = d->hidden_dim; a.perturb = d->perturb;
  const hode::RealStepGeom geo{d->n_times, d->n_dose, intervals_per_wave(d), (float*)(ws + (bwd ? L.sub : L.dose))};
  hipLaunchKernelGGL(hode::real_step_dose_kernel, dim3((d->batch + 63) / 64), dim3(64), 0, s, a);
  if (int e = hode::hip_fail(hipGetLastError(), "real step dose-table launch")) return e;
  const int M = d->latent_dim - 4;
  int e;
  switch (hidden_tiles(d)) {
#define HODE_REAL_STEP_CASE(n) case n: e = hode::real_step_launch_ht##n(d->method, bwd, a, geo, M, d->grad_w1, s); break;
    HODE_REAL_STEP_HTS(HODE_REAL_STEP_CASE)
#undef HODE_REAL_STEP_CASE
    default: return check_domain(d);
  }
  if (e || !bwd) return e;
  return hode::launch_fold_partials(a.partials, (int)n_waves(d), 3, 0, 0, nullptr, nullptr, d->grad_theta, 1, s);
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
