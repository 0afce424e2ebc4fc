// C-ABI entry points hode_dopri5_fwd / hode_dopri5_bwd (include/hode.h): checks, the Roche kernels' arguments and launches.
// The workspace carving, the chunk policy and the attempt loop are hode_adaptive_host.hpp's, shared with the NeuralODE.
//
// This unit is compiled twice, so that the checks, the layout, the arguments and the attempt loop below exist once: as it
// is for libhode.so, and with -DHODE_ROCHE_DIMS_UNIT for libhode_roche_dims.so (include/hode_roche_dims.h), where the
// entries are hode_roche_dims_dopri5_*, the table of sizes is that library's, its refusals come first and there is no
// NeuralODE to hand over to.  (A header would serve as well, but tests/test_kernel_variant_coverage.py reads the Hill
// read-back out of this file.)
#include <stdlib.h>
#include <string.h>

#include "hode_adaptive_host.hpp"
#include "hode_dopri5_kernels.hpp"

#ifdef HODE_ROCHE_DIMS_UNIT
#include "roche_dims/hode_roche_dims.hpp"
#define HODE_DP_ENTRY(name) hode_roche_dims_##name
#define HODE_DP_DOMAIN(d) if (int e_ = hode::roche_dims_check_domain(d)) return e_;
constexpr bool kHasNeural = false;
#else
#define HODE_DP_ENTRY(name) hode_##name
#define HODE_DP_DOMAIN(d)
constexpr bool kHasNeural = true;
#endif

namespace {

using hode::DpArgs;
using hode::DpCtrl;
using hode::DpLaunch;

// attempts between two reads of the controller record (hode_adaptive_host.hpp): first / min / max
constexpr hode::ChunkPolicy kChunks = {64, 32, 2048};
constexpr int kAttemptWavesPerBlock = 1;

// Patients per wave of the dopri5 kernels: full waves.  The fixed-grid kernels spread a small batch over ~one wave per
// SIMD (hode::patients_per_wave) because they stream h every step; an attempt launch has no such stream, its cost per
// wave does not depend on the number of live lanes, and every extra wave is one more workgroup to dispatch and one more
// error-norm partial for every wave of the next launch to read: 6.0-6.1 us per attempt with 16 patients per wave against
// 6.3 with 10 at 10 000 patients (A/B, same call); the backward is indifferent.
int dp_patients_per_wave(const hode_solve_desc* d) { return 64 / hode::choose_lpp(d); }
int dp_n_waves(const hode_solve_desc* d) {
  const int ppw = dp_patients_per_wave(d);
  return (d->batch + ppw - 1) / ppw;
}

using hode::AdaptiveLayout;
using hode::kInitOffset;

AdaptiveLayout dp_layout(const hode_solve_desc* d) {
  const int nw = dp_n_waves(d);
  return hode::adaptive_layout(nw, (size_t)d->batch * d->latent_dim, d->max_steps, d->flags & HODE_FLAG_NO_TAPE,
                               (size_t)2 * nw * sizeof(unsigned long long), hode::n_partials(d));
}

DpArgs dp_args(const hode_solve_desc* d, const AdaptiveLayout& L) {
  DpArgs a{};
  char* ws = (char*)d->workspace;
  a.t = d->t; a.y0 = d->y0; a.dosage = d->dosage; a.dose_times = d->dose_times; a.theta = d->theta;
  a.w1 = d->w1; a.b1 = d->b1; a.h = d->h;
  a.ctrl = (DpCtrl*)(ws + L.ctrl);
  a.init = (hode::DpInit*)(ws + L.ctrl + kInitOffset);
  a.partials = (float*)(ws + L.partials);
  a.slots = (unsigned long long*)(ws + L.slots);
  a.kbuf = (float*)(ws + L.kbuf);
  a.tape_t = (double*)(ws + L.tape_t);
  a.tape_dt = (double*)(ws + L.tape_dt);
  a.tape_j = (int*)(ws + L.tape_j);
  a.tape_y = (float*)(ws + L.tape_y);
  a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.hill2 = -1;
  a.grad_partials = (float*)(ws + L.grad_partials);
  a.B = d->batch; a.T = d->n_times; a.K = d->n_dose;
  a.n_waves = dp_n_waves(d);
  a.ppw = dp_patients_per_wave(d);
  a.max_steps = d->max_steps;
  a.ring = (d->flags & HODE_FLAG_NO_TAPE) ? 1 : 0;
  a.rtol = (float)d->rtol; a.atol = (float)d->atol;
  return a;
}

int dp_dispatch_dim(const hode_solve_desc* d, const DpLaunch& L, const DpArgs& a, hipStream_t s) {
#ifdef HODE_ROCHE_DIMS_UNIT
  switch (d->latent_dim) {
#define HODE_ROCHE_DIMS_CASE(n) case n: return hode::roche_dims_dp_dispatch_d##n(L, a, s);
    HODE_ROCHE_DIMS(HODE_ROCHE_DIMS_CASE)
#undef HODE_ROCHE_DIMS_CASE
  }
  return hode::roche_dims_check_domain(d);  // names the sizes
#else
  switch (d->latent_dim) {
    case 4: return hode::dp_dispatch_d4(L, a, s);
    case 6: return hode::dp_dispatch_d6(L, a, s);
    case 8: return hode::dp_dispatch_d8(L, a, s);
    case 12: return hode::dp_dispatch_d12(L, a, s);
  }
  return hode::fail(HODE_E_UNSUPPORTED, "dopri5: latent_dim %d has no compiled kernel (have 4, 6, 8, 12)", d->latent_dim);
#endif
}

bool is_neural(const hode_solve_desc* d) { return kHasNeural && d && d->struct_size == sizeof(hode_solve_desc) && d->rhs_kind == HODE_RHS_NEURAL; }

// argument checks shared by both rhs families
int check_common(const hode_solve_desc* d, bool bwd) {
  if (!d) return hode::fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return hode::fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->batch <= 0 || d->n_times <= 0 || d->latent_dim < 4 || d->n_dose < 0 || d->max_steps <= 0)
    return hode::fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d latent_dim=%d n_dose=%d max_steps=%d", d->batch,
                      d->n_times, d->latent_dim, d->n_dose, d->max_steps);
  if (!(d->rtol > 0) || !(d->atol >= 0)) return hode::fail(HODE_E_SIZE, "rtol must be > 0 and atol >= 0");
  if (!d->t || !d->y0 || !d->dosage || !d->h || (d->n_dose > 0 && !d->dose_times))
    return hode::fail(HODE_E_NULL, "t / y0 / dosage / dose_times / h must be non-NULL");
  if (!d->host_n_accepted) return hode::fail(HODE_E_NULL, "host_n_accepted is required (fwd: out, bwd: in)");
  if (bwd && (!d->grad_h || !d->grad_y0)) return hode::fail(HODE_E_NULL, "grad_h / grad_y0 required by the backward");
  if (bwd && (d->flags & HODE_FLAG_OVERWRITE_GRADS))
    return hode::fail(HODE_E_UNSUPPORTED, "HODE_FLAG_OVERWRITE_GRADS is only implemented by hode_rk_bwd");
  if (bwd && (d->flags & HODE_FLAG_NO_TAPE))
    return hode::fail(HODE_E_UNSUPPORTED, "the forward ran with HODE_FLAG_NO_TAPE: there is no tape to sweep");
  uintptr_t m = (uintptr_t)d->y0 | (uintptr_t)d->h | (uintptr_t)d->workspace;
  if (bwd) m |= (uintptr_t)d->grad_h | (uintptr_t)d->grad_y0;
  if (m & 15) return hode::fail(HODE_E_ALIGN, "y0 / h / grad_h / grad_y0 / workspace must be 16-byte aligned");
  return 0;
}

int check_dp(const hode_solve_desc* d, bool bwd) {
  if (int e = check_common(d, bwd)) return e;
  if (d->rhs_kind != HODE_RHS_ROCHE && d->rhs_kind != HODE_RHS_ROCHE_ABLATE)
    return hode::fail(HODE_E_UNSUPPORTED, "rhs_kind %d has no dopri5 kernels (have ROCHE, ROCHE_ABLATE, NEURAL)", d->rhs_kind);
  if (!d->theta) return hode::fail(HODE_E_NULL, "theta must be non-NULL");
  if (d->latent_dim > 4 && (!d->w1 || !d->b1)) return hode::fail(HODE_E_NULL, "w1 / b1 required when latent_dim > 4");
  const AdaptiveLayout L = dp_layout(d);
  if (!d->workspace || d->workspace_bytes < L.total)
    return hode::fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, L.total);
  return 0;
}

}  // namespace

#ifdef HODE_ROCHE_DIMS_UNIT
size_t hode::roche_dims_dopri5_workspace_bytes(const hode_solve_desc* d) { return dp_layout(d).total; }
#else
extern "C" size_t hode_dopri5_workspace_bytes(const hode_solve_desc* d) {
  return is_neural(d) ? hode::neural_dopri5_workspace_bytes(d) : dp_layout(d).total;
}
#endif

extern "C" int HODE_DP_ENTRY(dopri5_fwd)(const hode_solve_desc* d, void* stream) {
  HODE_DP_DOMAIN(d)
  if constexpr (kHasNeural) {
    if (is_neural(d)) {
      if (int e = check_common(d, false)) return e;
      return hode::neural_dopri5(d, false, (hipStream_t)stream);
    }
  }
  if (int e = check_dp(d, false)) return e;
  hipStream_t s = (hipStream_t)stream;
  const AdaptiveLayout lay = dp_layout(d);
  DpArgs a = dp_args(d, lay);
  DpLaunch L;
  L.lpp = hode::choose_lpp(d);
  L.ablate = d->rhs_kind == HODE_RHS_ROCHE_ABLATE;
  L.need_th = false;
  L.phase = 0;
  if (int e = dp_dispatch_dim(d, L, a, s)) return e;
  L.phase = 1;
  if (int e = dp_dispatch_dim(d, L, a, s)) return e;
  L.phase = 2;
  L.waves_per_block = kAttemptWavesPerBlock;
#ifdef HODE_DP_EXPERIMENTS   // diagnostic builds only: a stray environment variable must not change the shipped launch structure
  if (const char* env = getenv("HODE_DP_WPB")) {  // tuning
    const int v = atoi(env);
    if (v >= 1 && v <= 4) L.waves_per_block = v;
  }
#endif
  {
    // which rhs specialisation the attempts run (both Hill exponents == 2 is the shipped configuration) is a property of
    // the parameters: read the two exponents back once, under the init kernels, instead of on the device in every launch
    float hill[2] = {0.f, 0.f};
    if (int e = hode::hip_fail(hipMemcpyAsync(hill, d->theta, sizeof(hill), hipMemcpyDeviceToHost, s), "theta read-back")) return e;
    if (int e = hode::hip_fail(hipStreamSynchronize(s), "theta read-back sync")) return e;
    a.hill2 = (hill[0] == 2.0f && hill[1] == 2.0f) ? 1 : 0;
  }
  DpCtrl host{};
  const long long max_attempts = hode::adaptive_max_attempts(d);
  // Experiment builds only (-DHODE_DP_EXPERIMENTS, then HODE_DP_PERSIST=1, quad layout): the whole attempt loop in one persistent launch (dp_persist_body_own: state in
  // registers, one hop through memory per attempt instead of a kernel boundary).  Correct and bounded, but MEASURED SLOWER on
  // this part -- 7.0 us per attempt against 5.7 (tools/dp_persist_probe.py): a fence-free, atomics-free all-to-all exchange
  // across 8 XCDs still costs ~5 us, more than the ~3.8 us the kernel boundary costs.  Kept as the
  // reproducible form of that measurement; a launch that cannot assemble its waves falls back to the loop below.
  bool persist = false;
#ifdef HODE_DP_EXPERIMENTS
  if (const char* env = getenv("HODE_DP_PERSIST")) persist = atoi(env) != 0 && L.lpp == 4 && a.n_waves <= hode::kDpMaxPersistWaves;
#endif
  if (persist) {
    if (int e = hode::hip_fail(hipMemsetAsync(a.slots, 0, (size_t)2 * a.n_waves * sizeof(unsigned long long), s), "slot clear")) return e;
    L.phase = 6;
    a.max_iters = (int)(max_attempts > 0x3fffffff ? 0x3fffffff : max_attempts);
    if (int e = dp_dispatch_dim(d, L, a, s)) return e;
    if (int e = hode::hip_fail(hipMemcpyAsync(&host, a.ctrl, sizeof(DpCtrl), hipMemcpyDeviceToHost, s), "controller read-back")) return e;
    if (int e = hode::hip_fail(hipStreamSynchronize(s), "controller read-back sync")) return e;
    if (!(host.status & hode::kDpStatusBarrierTimeout)) {
      if (!host.done) host.status |= HODE_STATUS_MAX_STEPS;
    } else {
      // the grid could not assemble (another kernel held the CUs): start over, one launch per attempt
      persist = false;
      L.phase = 0;
      if (int e = dp_dispatch_dim(d, L, a, s)) return e;
      L.phase = 1;
      if (int e = dp_dispatch_dim(d, L, a, s)) return e;
      host = DpCtrl{};
    }
  }
  L.phase = 2;
  if (!persist) {
    const auto enqueue = [&](int i) {
      a.attempt = i;
      return dp_dispatch_dim(d, L, a, s);  // checks its own launch
    };
    if (int e = hode::adaptive_attempts(d, a.ctrl, kChunks, "dopri5 attempt launch", s, enqueue, &host)) return e;
  }
  return hode::adaptive_report(d, host, s);
}

extern "C" int HODE_DP_ENTRY(dopri5_bwd)(const hode_solve_desc* d, void* stream) {
  HODE_DP_DOMAIN(d)
  if constexpr (kHasNeural) {
    if (is_neural(d)) {
      if (int e = check_common(d, true)) return e;
      return hode::neural_dopri5(d, true, (hipStream_t)stream);
    }
  }
  if (int e = check_dp(d, true)) return e;
  hipStream_t s = (hipStream_t)stream;
  const AdaptiveLayout lay = dp_layout(d);
  DpArgs a = dp_args(d, lay);
  a.n_acc = *d->host_n_accepted;
  if (a.n_acc < 0 || a.n_acc > d->max_steps) return hode::fail(HODE_E_SIZE, "n_accepted %d outside the tape", a.n_acc);
  DpLaunch L;
  L.lpp = hode::choose_lpp(d);
  L.ablate = d->rhs_kind == HODE_RHS_ROCHE_ABLATE;
  L.need_th = d->need_theta_grad != 0;
  L.phase = 3;
  if (int e = dp_dispatch_dim(d, L, a, s)) return e;
  const int M = d->latent_dim - 4;
  if (int e = hode::launch_fold_partials(a.grad_partials, a.n_waves, hode::n_partials(d), M * d->latent_dim, M, d->grad_w1,
                                         d->grad_b1, d->grad_theta, d->need_theta_grad, s))
    return e;
  if (a.n_acc == 0 || (d->flags & HODE_FLAG_DETACH_FIRST_STEP)) return 0;
  // the reference's graph differentiates dt_0 (kernels: "backward of the initial step size"); the partial array is free
  // again once the fold above has read it (same stream)
  L.phase = 4;
  if (int e = dp_dispatch_dim(d, L, a, s)) return e;
  L.phase = 5;
  if (int e = dp_dispatch_dim(d, L, a, s)) return e;
  return hode::launch_fold_partials(a.grad_partials, a.n_waves, hode::n_partials(d), M * d->latent_dim, M, d->grad_w1,
                                    d->grad_b1, d->grad_theta, d->need_theta_grad, s);
}

extern "C" int HODE_DP_ENTRY(dopri5_tape_offsets)(const hode_solve_desc* d, size_t* out5) {
  if (!d || !out5) return hode::fail(HODE_E_NULL, "descriptor / out5 is NULL");
  if (d->struct_size != sizeof(hode_solve_desc)) return hode::fail(HODE_E_SIZE, "struct_size mismatch");
  HODE_DP_DOMAIN(d)
  if constexpr (kHasNeural) {
    if (is_neural(d)) return hode::neural_dopri5_tape_offsets(d, out5);
  }
  hode::adaptive_tape_offsets(dp_layout(d), out5);
  return 0;
}
