// Dormand-Prince 5(4) with PER-PATIENT step control for the hybrid Roche rhs, gfx950 (C ABI: include/hode_dopri5_pp.h).
//
// hode_dopri5_kernels.hpp restates torchdiffeq's batch-global controller: one RMS error norm over B*D elements, one dt for
// everybody, hence a grid-wide reduction and a kernel boundary per attempt.  Here a patient controls its own steps (its norm
// runs over its own D components), so nothing is exchanged between lanes: a lane (LaneMap<1>) runs its patient's WHOLE solve
// -- Hairer's first step, attempts, accept / reject, dense output, tape -- in registers, in one launch, and a second launch
// sweeps the per-patient tapes backwards.  The arithmetic is dp_init1_body / dp_init2_body / dp_attempt_body / dp_bwd_body
// with the count B*D replaced by D; the rhs, its VJP, the stages, the tableau, the step factor and the partial rows are
// those headers' own code, compiled here.
//
// Divergence.  Lanes of a wave take different numbers of attempts, so the attempt loop and the sweep run under a divergent
// exec mask.  Nothing inside them crosses lanes: the LPP = 1 bodies of roche_rhs / roche_vjp / gather_rows / pick_own are
// plain per-lane arithmetic (their DPP moves exist for LPP = 4 only), dp_stages and dp_step_factor likewise.  The
// reductions (wave_sum in store_grad_partials) and the status atomicOr come after the loops, where the wave has
// reconverged.  Every loop is bounded by max_attempts / max_steps / T, none by data.
//
// All step sizes are constants in the backward, dt_0 included (the semantics of HODE_FLAG_DETACH_FIRST_STEP); the sigma /
// dp_initbwd_* machinery of the batch-global path has no counterpart here.
#pragma once
#include "../../../include/hode_dopri5_pp.h"
#include "../hode_dopri5_kernels.hpp"

namespace hode {

struct PpArgs {
  const float* __restrict__ t;
  const float* __restrict__ y0;
  const float* __restrict__ dosage;
  const float* __restrict__ dose_times;
  const float* __restrict__ theta;
  const float* __restrict__ w1;
  const float* __restrict__ b1;
  float* __restrict__ h;
  int* status;               // [1] OR of all patients
  int* __restrict__ n_acc;   // [B]
  int* __restrict__ n_rej;   // [B]
  int* __restrict__ pstatus; // [B]
  double* tape_t;            // [max_steps][B]
  double* tape_dt;           // [max_steps][B]
  int2* tape_j;              // [max_steps][B]: first / one-past-last output index interpolated inside the step
  float* tape_y;             // [max_steps][B][D]: the state at the START of the step
  const float* __restrict__ grad_h;
  float* __restrict__ grad_y0;
  float* __restrict__ grad_partials;  // [n_waves][P]
  int B, T, K, max_steps, max_attempts, no_tape;
  float rtol, atol;
};

struct PpLaunch {
  bool ablate, bwd, need_th;
};

constexpr int kPpLanes = 64;  // patients per wave: lane per patient, full waves

// ------------------------------------------------------------------------------------------------------- forward
template <int D, bool ABLATE, bool HILL2, bool K1>
HODE_DEV void pp_fwd_body(const PpArgs& a) {
  using Ml = MlSlice<D, 1>;
  constexpr int MR = Ml::MR;
  const LaneMap<1> lm(a.B, kPpLanes);
  const int p = lm.p;  // idle lanes shadow the last patient and never store
  const RocheTheta th = load_theta(a.theta, ABLATE);
  Ml ml;
  ml.load(a.w1, a.b1, 0);
  const DoseSched<K1> ds = load_dose<K1>(a.dosage, a.dose_times, a.K, p);
  const size_t Bs = (size_t)a.B;
  const size_t row = Bs * D;
  const size_t poff = (size_t)p * D;
  const float cnt = (float)D;

  // ---- f0 and Hairer's initial step from this patient's own norms (dp_init1_body / dp_init2_body / attempt 0)
  float y[D], f0[D], own[MR];
  load_vec<D>(a.y0 + poff, y);
  const float tf0 = a.t[0];
  roche_rhs<D, 1, ABLATE, HILL2>(th, ml, ds.at(tf0, th.kel).v, y, f0, own);
  store_vec<D, 1>(a.h + poff, y, 0, lm.live);
  double dt;
  {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const float scale = a.atol + __builtin_fabsf(y[c]) * a.rtol;
      const float u = div_f32(y[c], scale), v = div_f32(f0[c], scale);
      s0 = __builtin_fmaf(u, u, s0);
      s1 = __builtin_fmaf(v, v, s1);
    }
    const float d0 = __builtin_sqrtf(s0 / cnt);
    const float d1 = __builtin_sqrtf(s1 / cnt);
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : div_f32(0.01f * d0, d1);
    float y1[D], f1[D];
#pragma unroll
    for (int c = 0; c < D; ++c) y1[c] = __builtin_fmaf(h0, f0[c], y[c]);
    roche_rhs<D, 1, ABLATE, HILL2>(th, ml, ds.at(add_rn(tf0, h0), th.kel).v, y1, f1, own);
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const float scale = a.atol + __builtin_fabsf(y[c]) * a.rtol;
      const float u = div_f32(f1[c] - f0[c], scale);
      s2 = __builtin_fmaf(u, u, s2);
    }
    const float d2 = div_f32(__builtin_sqrtf(s2 / cnt), h0);
    float h1;
    if (d1 <= 1e-15f && d2 <= 1e-15f) h1 = fmaxf(1e-6f, h0 * 1e-3f);
    else h1 = powf(div_f32(0.01f, fmaxf(d1, d2)), 0.2f);
    dt = (double)fminf(100.0f * h0, h1);
  }

  // ---- the attempt loop: fp64 clock, fp32 stage times (dp_attempt_body, its decision taken in the same iteration)
  double t0 = (double)tf0;
  int n_acc = 0, n_rej = 0, j_next = 1, status = 0;
  bool run = lm.live && a.T > 1;
  for (int it = 0; run; ++it) {
    if (j_next >= a.T) break;
    // torchdiffeq asserts on the state before a step; here ahead of the dt check, so that a NaN state is reported as one
    // (the NaN step size it produces would otherwise read as an underflow)
    bool bad = false;
#pragma unroll
    for (int i = 0; i < D; ++i) bad |= !__builtin_isfinite(y[i]);
    if (bad) { status |= HODE_STATUS_NONFINITE; break; }
    if (!(t0 + dt > t0)) { status |= HODE_STATUS_DT_UNDERFLOW; break; }
    if (n_acc >= a.max_steps || it >= a.max_attempts) { status |= HODE_STATUS_MAX_STEPS; break; }
    const double t1 = t0 + dt;
    const float t0f = (float)t0, dtf = (float)dt, t1f = (float)t1;
    float k[7][D], Y[7][D], s[7][MR];
    DoseVal dv[7];
#pragma unroll
    for (int i = 0; i < D; ++i) k[0][i] = f0[i];
    dp_stages<D, 1, ABLATE, HILL2, K1>(th, ml, ds, y, t0f, dtf, t1f, k, Y, s, dv);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      float err = 0.f;
#pragma unroll
      for (int m = 0; m < 7; ++m) err = __builtin_fmaf(dtf * kDpErr[m], k[m][i], err);
      const float tol = a.atol + a.rtol * fmaxf(__builtin_fabsf(y[i]), __builtin_fabsf(Y[6][i]));
      const float u = div_f32(err, tol);
      se = __builtin_fmaf(u, u, se);
    }
    const float ratio = __builtin_sqrtf(se / cnt);
    if (ratio <= 1.0f) {
      // emit every output time inside (t0, t1] from the quartic dense output (coefficient forms of dp_attempt_body)
      int j = j_next;
      if ((double)a.t[j] <= t1) {
        float ym[D];
#pragma unroll
        for (int i = 0; i < D; ++i) ym[i] = y[i];
#pragma unroll
        for (int m = 0; m < 7; ++m) {
          const float w = dtf * kDpMid[m];
#pragma unroll
          for (int i = 0; i < D; ++i) ym[i] = __builtin_fmaf(w, k[m][i], ym[i]);
        }
        float ca[D], cb[D], cc_[D], cd[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const float f0i = k[0][i], f1i = k[6][i], y0i = y[i], y1i = Y[6][i], ymi = ym[i];
          ca[i] = 2.0f * dtf * (f1i - f0i) - 8.0f * (y1i + y0i) + 16.0f * ymi;
          cb[i] = dtf * (5.0f * f0i - 3.0f * f1i) + 18.0f * y0i + 14.0f * y1i - 32.0f * ymi;
          cc_[i] = dtf * (f1i - 4.0f * f0i) - 11.0f * y0i - 5.0f * y1i + 16.0f * ymi;
          cd[i] = dtf * f0i;
        }
        for (; j < a.T && (double)a.t[j] <= t1; ++j) {
          const float x = (float)(((double)a.t[j] - t0) / (t1 - t0));
          const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
          float out[D];
#pragma unroll
          for (int i = 0; i < D; ++i) out[i] = (((y[i] + x * cd[i]) + x2 * cc_[i]) + x3 * cb[i]) + x4 * ca[i];
          store_vec<D, 1>(a.h + (size_t)j * row + poff, out, 0, true);
        }
      }
      if (!a.no_tape) {  // n_acc < max_steps: checked above
        const size_t e = (size_t)n_acc * Bs + (size_t)p;
        a.tape_t[e] = t0;
        a.tape_dt[e] = dt;
        a.tape_j[e] = make_int2(j_next, j);
        store_vec<D, 1>(a.tape_y + e * D, y, 0, true);
      }
      j_next = j;
      ++n_acc;
      t0 = t1;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        y[i] = Y[6][i];
        f0[i] = k[6][i];  // FSAL
      }
    } else {
      ++n_rej;  // a NaN ratio lands here, and its NaN factor ends the lane with DT_UNDERFLOW
    }
    dt = dt * dp_step_factor(ratio);
  }
  // the wave has reconverged
  if (lm.live) {
    a.n_acc[p] = n_acc;
    a.n_rej[p] = n_rej;
    a.pstatus[p] = status;
    if (status) atomicOr(a.status, status);
  }
}

template <int D, bool ABLATE>
__global__ __launch_bounds__(64) void pp_fwd_kernel(PpArgs a) {
  const bool hill2 = ABLATE || (a.theta[0] == 2.0f && a.theta[1] == 2.0f);
  if (hill2 && a.K == 1) pp_fwd_body<D, ABLATE, true, true>(a);
  else if (hill2) pp_fwd_body<D, ABLATE, true, false>(a);
  else pp_fwd_body<D, ABLATE, false, false>(a);
}

// ------------------------------------------------------------------------------------------------------ backward
// dp_bwd_body with per-lane tape reads and without the dt_0 terms: each lane sweeps its own accepted steps
// n = n_accepted[p]-1 .. 0, recomputes the stages from tape_y and accumulates lam_y, lam_f and the GradAcc terms.
template <int D, bool ABLATE, bool HILL2, bool NEED_TH, bool K1>
HODE_DEV void pp_bwd_body(const PpArgs& a) {
  using Ml = MlSlice<D, 1>;
  constexpr int MR = Ml::MR;
  constexpr int M = D - 4;
  const LaneMap<1> lm(a.B, kPpLanes);
  const int p = lm.p;
  const RocheTheta th = load_theta(a.theta, ABLATE);
  Ml ml;
  ml.load(a.w1, a.b1, 0);
  MlColSlice<D, 1> mc;
  mc.load(a.w1, 0);
  const float ln_ec50 = log_f32(th.ec50);
  const DoseSched<K1> ds = load_dose<K1>(a.dosage, a.dose_times, a.K, p);
  GradAcc<D, 1> acc;
  acc.zero();
  const size_t Bs = (size_t)a.B;
  const size_t row = Bs * D;
  const size_t poff = (size_t)p * D;

  float lam_y[D], lam_f[D];
#pragma unroll
  for (int i = 0; i < D; ++i) lam_y[i] = lam_f[i] = 0.f;

  const int n_mine = lm.live ? min(max(a.n_acc[p], 0), a.max_steps) : 0;  // idle lanes sweep nothing and add zeros
  for (int n = n_mine - 1; n >= 0; --n) {
    const size_t e = (size_t)n * Bs + (size_t)p;
    const double t0 = a.tape_t[e], dt = a.tape_dt[e];
    const double t1 = t0 + dt;
    const float t0f = (float)t0, dtf = (float)dt, t1f = (float)t1;
    float y0[D];
    load_vec<D>(a.tape_y + e * D, y0);
    float k[7][D], Y[7][D], s[7][MR];
    DoseVal dv[7];
    const float tk1 = (n == 0) ? a.t[0] : nextafter_down(t0f);
    dv[0] = ds.at(tk1, th.kel);
    roche_rhs<D, 1, ABLATE, HILL2>(th, ml, dv[0].v, y0, k[0], s[0]);
#pragma unroll
    for (int i = 0; i < D; ++i) Y[0][i] = y0[i];
    dp_stages<D, 1, ABLATE, HILL2, K1>(th, ml, ds, y0, t0f, dtf, t1f, k, Y, s, dv);

    float g[7][D], lam_y0[D], lam_mid[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      g[6][i] = lam_f[i];
      lam_y0[i] = 0.f;
      lam_mid[i] = 0.f;
#pragma unroll
      for (int m = 0; m < 6; ++m) g[m][i] = 0.f;
    }
    // cotangents of the outputs interpolated inside this step (the indices are the forward's own; clamped all the same)
    const int2 jj = a.tape_j[e];
    const int jlo = max(jj.x, 1), jhi = min(jj.y, a.T);
    for (int j = jlo; j < jhi; ++j) {
      const float x = (float)(((double)a.t[j] - t0) / (t1 - t0));
      const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
      const float P0 = 1.0f - 11.0f * x2 + 18.0f * x3 - 8.0f * x4;
      const float P1 = -5.0f * x2 + 14.0f * x3 - 8.0f * x4;
      const float Pm = 16.0f * x2 - 32.0f * x3 + 16.0f * x4;
      const float Q0 = dtf * (x - 4.0f * x2 + 5.0f * x3 - 2.0f * x4);
      const float Q1 = dtf * (x2 - 3.0f * x3 + 2.0f * x4);
      float G[D];
      load_vec<D>(a.grad_h + (size_t)j * row + poff, G);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        lam_y0[i] = __builtin_fmaf(P0, G[i], lam_y0[i]);
        lam_y[i] = __builtin_fmaf(P1, G[i], lam_y[i]);
        lam_mid[i] = __builtin_fmaf(Pm, G[i], lam_mid[i]);
        g[0][i] = __builtin_fmaf(Q0, G[i], g[0][i]);
        g[6][i] = __builtin_fmaf(Q1, G[i], g[6][i]);
      }
    }
    // y_mid = y0 + dt sum cmid_m k_m
#pragma unroll
    for (int i = 0; i < D; ++i) {
      lam_y0[i] += lam_mid[i];
#pragma unroll
      for (int m = 0; m < 7; ++m) g[m][i] = __builtin_fmaf(dtf * kDpMid[m], lam_mid[i], g[m][i]);
    }
    // stage 7: k7 = f(t1-, y1)
    float a_[D];
    roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, dv[6], Y[6], s[6], g[6], 0, a_, acc);
#pragma unroll
    for (int i = 0; i < D; ++i) lam_y[i] += a_[i];
    // y1 = y0 + dt sum_{m<=6} beta_6m k_m
#pragma unroll
    for (int i = 0; i < D; ++i) {
      lam_y0[i] += lam_y[i];
#pragma unroll
      for (int m = 0; m < 6; ++m) g[m][i] = __builtin_fmaf(kDpBeta[5][m] * dtf, lam_y[i], g[m][i]);
    }
    // stages 6 .. 2
#pragma unroll
    for (int st = 6; st >= 2; --st) {
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, dv[st - 1], Y[st - 1], s[st - 1], g[st - 1], 0, a_, acc);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        lam_y0[i] += a_[i];
#pragma unroll
        for (int m = 0; m < st - 1; ++m) g[m][i] = __builtin_fmaf(kDpBeta[st - 2][m] * dtf, a_[i], g[m][i]);
      }
    }
    // g1 is handed to step n-1 as lam_f (k1 of step n IS k7 of step n-1); at n = 0 it goes through J1 instead
    if (n == 0) {
      roche_vjp<D, 1, ABLATE, HILL2, NEED_TH>(th, ml, mc, ln_ec50, dv[0], Y[0], s[0], g[0], 0, a_, acc);
#pragma unroll
      for (int i = 0; i < D; ++i) lam_y0[i] += a_[i];
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      lam_y[i] = lam_y0[i];
      lam_f[i] = g[0][i];
    }
  }
  // the wave has reconverged.  Output 0 is y0 itself
  {
    float G[D];
    load_vec<D>(a.grad_h + poff, G);
#pragma unroll
    for (int i = 0; i < D; ++i) lam_y[i] += G[i];
  }
  store_vec<D, 1>(a.grad_y0 + poff, lam_y, 0, lm.live);

  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  constexpr int P = M * D + M + kNTheta;
  store_grad_partials<D, 1, NEED_TH>(acc, a.grad_partials + (size_t)wave * P);
}

template <int D, bool ABLATE, bool NEED_TH>
__global__ __launch_bounds__(64) void pp_bwd_kernel(PpArgs a) {
  const bool hill2 = ABLATE || (a.theta[0] == 2.0f && a.theta[1] == 2.0f);
  if (hill2 && a.K == 1) pp_bwd_body<D, ABLATE, true, NEED_TH, true>(a);
  else if (hill2) pp_bwd_body<D, ABLATE, true, NEED_TH, false>(a);
  else pp_bwd_body<D, ABLATE, false, NEED_TH, false>(a);
}

// one launch of the forward or of the sweep for latent size D; the caller turns the hipError_t into the library's message
template <int D>
hipError_t pp_launch(const PpLaunch& L, const PpArgs& a, hipStream_t s) {
  const dim3 grid((a.B + kPpLanes - 1) / kPpLanes), block(64);
  if (!L.bwd) {
    if (L.ablate) hipLaunchKernelGGL((pp_fwd_kernel<D, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((pp_fwd_kernel<D, false>), grid, block, 0, s, a);
  } else if (L.ablate) {
    if (L.need_th) hipLaunchKernelGGL((pp_bwd_kernel<D, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((pp_bwd_kernel<D, true, false>), grid, block, 0, s, a);
  } else {
    if (L.need_th) hipLaunchKernelGGL((pp_bwd_kernel<D, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((pp_bwd_kernel<D, false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

// one entry per compiled latent size (hode_dopri5_pp_dim.hip, -DHODE_DIM=<D>)
hipError_t pp_launch_d4(const PpLaunch&, const PpArgs&, hipStream_t);
hipError_t pp_launch_d6(const PpLaunch&, const PpArgs&, hipStream_t);
hipError_t pp_launch_d8(const PpLaunch&, const PpArgs&, hipStream_t);
hipError_t pp_launch_d12(const PpLaunch&, const PpArgs&, hipStream_t);

}  // namespace hode
