// Kernel templates of the adaptive NeuralODE solve (hode_neural_dopri5.hip has the description): the attempt kernels, the
// backward sweep, the backward of the initial step size, and the host templates that launch them, nd_fwd and nd_bwd, on the
// workspace carving, chunk policy and attempt loop of hode_adaptive_host.hpp.  Instantiated by hode_neural_dopri5.hip for
// libhode.so (even latent dimensions) and by neural_odd/hode_neural_odd_dim.hip for libhode_neural_odd.so (odd ones);
// nothing here is instantiated by inclusion.
#pragma once
#include <hip/hip_runtime.h>

#include "hode_adaptive_host.hpp"
#include "hode_dopri5_kernels.hpp"
#include "hode_neural_mf.hpp"

namespace hode {

struct NdpArgs {
  NeuralArgs nn;  // t, y0, dosage, dose_times, w1, b1, b2, w2, h, grad_h, grad_y0, B, T, K
  DpCtrl* ctrl;
  DpInit* init;
  float* partials;       // [4 * n_waves], as DpArgs::partials: the odd slots of the second half carry init1's non-finite flags
  float* kbuf;           // [7][B][D]
  double* tape_t;
  double* tape_dt;
  int* tape_j;
  float* tape_y;
  float* grad_partials;  // [n_waves][NP]
  float* grad_w1;
  float* grad_b1;
  float* grad_w2;
  float* grad_b2;
  int n_waves, max_steps, attempt, n_acc, ring;
  float rtol, atol;
};

HODE_DEV size_t ndp_tape_row(const NdpArgs& a, int n) { return (size_t)(a.ring ? (n & 1) : n); }
// per-lane context: which patient / rows this lane holds
template <int D>
struct NdpLane {
  int g, n, p, wave, lane;
  bool live;
  float lv, dosage;
  v4 valid;  // 1 for rows < D
  HODE_DEV NdpLane(const NdpArgs& a) {
    lane = threadIdx.x;
    g = lane >> 4;
    n = lane & 15;
    wave = blockIdx.x;
    const int pr = wave * 16 + n;
    live = pr < a.nn.B;
    p = live ? pr : a.nn.B - 1;
    lv = live ? 1.0f : 0.0f;
    dosage = a.nn.dosage[p];
#pragma unroll
    for (int r = 0; r < 4; ++r) valid[r] = (4 * g + r) < D ? 1.0f : 0.0f;
  }
};

// sum over the wave of (u / s)^2 on the valid rows of live patients
template <int D>
HODE_DEV float ndp_sq_ratio(const NdpLane<D>& L, const v4& u, const v4& s) {
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float q = L.valid[r] != 0.0f ? div_f32(u[r], s[r]) : 0.0f;
    acc = __builtin_fmaf(q, q, acc);
  }
  return acc * L.lv;
}

template <int D>
HODE_DEV v4 ndp_scale(const NdpArgs& a, const v4& y) {
  v4 s;
#pragma unroll
  for (int r = 0; r < 4; ++r) s[r] = a.atol + __builtin_fabsf(y[r]) * a.rtol;
  return s;
}

// ------------------------------------------------------------------------------------------------ forward kernels
template <int D, int PHASE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ndp_fwd_kernel(NdpArgs a) {
  constexpr int HT = NeuralMf<D>::HT;
  const NdpLane<D> L(a);
  const int g = L.g;
  const size_t row = (size_t)a.nn.B * D;
  const size_t poff = (size_t)L.p * D;
  const float cnt = (float)a.nn.B * (float)D;
  const int gid = blockIdx.x * 64 + threadIdx.x;
  v4 a1[HT];

  if constexpr (PHASE == 0) {
    // init1: f0 = f(t[0], y0); h[0] = tape_y[0] = y0; kbuf[0] = f0; partials of (y0/scale)^2, (f0/scale)^2
    NeuralMf<D> nn;
    nn.load(a.nn, L.lane);
    const v4 y = mf_load_rows<D>(a.nn.y0 + poff, g);
    const v4 f0 = nn.rhs(mf_with_dose<D>(y, neural_dose(a.nn, L.p, L.dosage, a.nn.t[0]), g), a1);
    mf_store_rows<D>(a.nn.h + poff, g, y, L.live);
    mf_store_rows<D>(a.tape_y + poff, g, y, L.live);
    mf_store_rows<D>(a.kbuf + poff, g, f0, L.live);
    const v4 sc = ndp_scale<D>(a, y);
    const float s0 = wave_sum(ndp_sq_ratio<D>(L, y, sc)), s1 = wave_sum(ndp_sq_ratio<D>(L, f0, sc));
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) bad |= L.valid[r] != 0.0f && !__builtin_isfinite(y[r]);
    const bool wave_bad = __builtin_amdgcn_ballot_w64(bad && L.live) != 0;
    if (L.lane == 0) {
      a.partials[2 * L.wave] = s0;
      a.partials[2 * L.wave + 1] = s1;
      // a non-finite start state (dp_init1_body): the wave's flag, in the slot no other launch uses
      a.partials[2 * a.n_waves + 2 * L.wave + 1] = wave_bad ? 1.0f : 0.0f;
    }
  } else if constexpr (PHASE == 1) {
    // init2: h0 from (d0, d1); f1 = f(t0 + h0, y0 + h0 f0); partial of ((f1 - f0)/scale)^2; lane 0 seeds the controller
    NeuralMf<D> nn;
    nn.load(a.nn, L.lane);
    const float d0 = __builtin_sqrtf(fold_waves(a.partials, a.n_waves, 2, 0) / cnt);
    const float d1 = __builtin_sqrtf(fold_waves(a.partials, a.n_waves, 2, 1) / cnt);
    const float bad0 = fold_waves(a.partials + (size_t)2 * a.n_waves, a.n_waves, 2, 1);  // init1's non-finite flags
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : div_f32(0.01f * d0, d1);
    const v4 y = mf_load_rows<D>(a.nn.y0 + poff, g);
    const v4 f0 = mf_load_rows<D>(a.kbuf + poff, g);
    const float t0f = a.nn.t[0];
    const v4 f1 = nn.rhs(mf_with_dose<D>(vfma4(h0, f0, y), neural_dose(a.nn, L.p, L.dosage, add_rn(t0f, h0)), g), a1);
    const float s2 = wave_sum(ndp_sq_ratio<D>(L, f1 - f0, ndp_scale<D>(a, y)));
    float* pout = a.partials + (size_t)2 * a.n_waves;
    if (L.lane == 0) pout[2 * L.wave] = s2;
    if (gid == 0) {
      DpCtrl c;
      c.t0 = (double)t0f;
      c.dt = 0.0;
      c.h0 = h0;
      c.d1 = d1;
      c.n_acc = 0; c.n_rej = 0; c.j_next = 1; c.done = (a.nn.T <= 1) ? 1 : 0; c.attempt = 0;
      c.status = bad0 != 0.0f ? HODE_STATUS_NONFINITE : 0;  // attempt 0 stops on it before it looks at dt_0
      a.ctrl[0] = c;
      a.ctrl[1] = c;
      DpInit in{};
      in.h0 = h0; in.d0 = d0; in.d1 = d1;
      *a.init = in;
    }
  } else {
    // one attempt (see dp_attempt_body_own: same record handling, same dense output, same termination checks)
    const int par = a.attempt & 1;
    DpCtrl* cout = a.ctrl + (par ^ 1);
    const float* pin = a.partials + (size_t)(par ^ 1) * 2 * a.n_waves;
    float* pout = a.partials + (size_t)par * 2 * a.n_waves;
    const FoldHead head = fold_issue(pin, a.n_waves, 2, 0);
    const DpCtrl cin = a.ctrl[par];
    if (cin.done) {
      if (gid == 0) *cout = cin;
      return;
    }
    NeuralMf<D> nn;
    nn.load(a.nn, L.lane);
    const v4 y_old = mf_load_rows<D>(a.tape_y + ndp_tape_row(a, cin.n_acc) * row + poff, g);
    const v4 k_first = mf_load_rows<D>(a.kbuf + poff, g);
    const v4 y_new = mf_load_rows<D>(a.tape_y + ndp_tape_row(a, cin.n_acc + 1) * row + poff, g);
    const v4 k_last = mf_load_rows<D>(a.kbuf + 6 * row + poff, g);
    const float t_next = a.nn.t[min(cin.j_next, a.nn.T - 1)];

    DpCtrl c = cin;
    v4 y, f0;
    if (cin.attempt == 0) {
      const float d2 = div_f32(__builtin_sqrtf(fold_finish(head, pin, a.n_waves, 2, 0) / cnt), cin.h0);
      float h1;
      if (cin.d1 <= 1e-15f && d2 <= 1e-15f) h1 = fmaxf(1e-6f, cin.h0 * 1e-3f);
      else h1 = powf(div_f32(0.01f, fmaxf(cin.d1, d2)), 0.2f);
      c.dt = (double)fminf(100.0f * cin.h0, h1);
      if (gid == 0) { a.init->d2 = d2; a.init->h1 = h1; }
      y = y_old;
      f0 = k_first;
    } else {
      const float ratio = __builtin_sqrtf(fold_finish(head, pin, a.n_waves, 2, 0) / cnt);
      const double t1 = cin.t0 + cin.dt;
      if (cin.attempt == 1 && gid == 0) a.init->first_accepted = ratio <= 1.0f ? 1 : 0;
      if (ratio <= 1.0f) {
        y = y_new;
        f0 = k_last;
        int j = cin.j_next;
        if (j < a.nn.T && (double)t_next <= t1) {
          const float dtf = (float)cin.dt;
          v4 ym = y_old;
          for (int m = 0; m < 7; ++m) ym = vfma4(dtf * kDpMid[m], mf_load_rows<D>(a.kbuf + (size_t)m * row + poff, g), ym);
          const v4 f0i = k_first, f1i = f0, y0i = y_old, y1i = y;
          const v4 ca = 2.0f * dtf * (f1i - f0i) - 8.0f * (y1i + y0i) + 16.0f * ym;
          const v4 cb = dtf * (5.0f * f0i - 3.0f * f1i) + 18.0f * y0i + 14.0f * y1i - 32.0f * ym;
          const v4 cc = dtf * (f1i - 4.0f * f0i) - 11.0f * y0i - 5.0f * y1i + 16.0f * ym;
          const v4 cd = dtf * f0i;
          for (; j < a.nn.T && (double)a.nn.t[j] <= t1; ++j) {
            const float x = (float)(((double)a.nn.t[j] - cin.t0) / (t1 - cin.t0));
            const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
            const v4 out = (((y0i + x * cd) + x2 * cc) + x3 * cb) + x4 * ca;
            mf_store_rows<D>(a.nn.h + (size_t)j * row + poff, g, out, L.live);
          }
        }
        if (gid == 0) {
          a.tape_t[cin.n_acc] = cin.t0;
          a.tape_dt[cin.n_acc] = cin.dt;
          a.tape_j[2 * cin.n_acc] = cin.j_next;
          a.tape_j[2 * cin.n_acc + 1] = j;
        }
        c.j_next = j;
        c.n_acc = cin.n_acc + 1;
        c.t0 = t1;
      } else {
        c.n_rej = cin.n_rej + 1;
        y = y_old;
        f0 = k_first;
      }
      c.dt = cin.dt * dp_step_factor(ratio);
    }
    c.attempt = cin.attempt + 1;

    bool stop = false;
    if (c.status) { c.done = 1; stop = true; }
    if (!stop && c.j_next >= a.nn.T) { c.done = 1; stop = true; }
    if (!stop && !(c.t0 + c.dt > c.t0)) { c.status |= HODE_STATUS_DT_UNDERFLOW; c.done = 1; stop = true; }
    if (!stop && c.n_acc >= a.max_steps) { c.status |= HODE_STATUS_MAX_STEPS; c.done = 1; stop = true; }
    if (stop) {
      if (gid == 0) *cout = c;
      return;
    }

    const float t0f = (float)c.t0, dtf = (float)c.dt, t1f = (float)(c.t0 + c.dt);
    v4 k[7], Y = y;
    k[0] = f0;
#pragma unroll
    for (int i = 2; i <= 7; ++i) {
      const float ti = dp_stage_time(i, t0f, dtf, t1f);
      Y = y;
#pragma unroll
      for (int m = 0; m < i - 1; ++m) Y = vfma4(kDpBeta[i - 2][m] * dtf, k[m], Y);
      k[i - 1] = nn.rhs(mf_with_dose<D>(Y, neural_dose(a.nn, L.p, L.dosage, ti), g), a1);
    }
    // Y is y1 (FSAL row)
    v4 err = splat4(0.f), tol;
    bool bad = false;
#pragma unroll
    for (int m = 0; m < 7; ++m) err = vfma4(dtf * kDpErr[m], k[m], err);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tol[r] = a.atol + a.rtol * fmaxf(__builtin_fabsf(y[r]), __builtin_fabsf(Y[r]));
      bad |= !__builtin_isfinite(y[r]);
    }
    const float se = wave_sum(ndp_sq_ratio<D>(L, err, tol));
    if (L.lane == 0) pout[2 * L.wave] = se;
    mf_store_rows<D>(a.tape_y + ndp_tape_row(a, c.n_acc + 1) * row + poff, g, Y, L.live);
    mf_store_rows<D>(a.kbuf + poff, g, k[0], L.live);
    mf_store_rows<D>(a.kbuf + 6 * row + poff, g, k[6], L.live);
    if ((double)(c.j_next == cin.j_next ? t_next : a.nn.t[c.j_next]) <= c.t0 + c.dt) {
#pragma unroll
      for (int m = 1; m < 6; ++m) mf_store_rows<D>(a.kbuf + (size_t)m * row + poff, g, k[m], L.live);
    }
    if (bad && L.live) atomicOr(&cout->status, HODE_STATUS_NONFINITE);
    if (gid == 0) {
      cout->t0 = c.t0; cout->dt = c.dt; cout->h0 = c.h0; cout->d1 = c.d1;
      cout->n_acc = c.n_acc; cout->n_rej = c.n_rej; cout->j_next = c.j_next; cout->done = c.done; cout->attempt = c.attempt;
      if (c.status) atomicOr(&cout->status, c.status);
    }
  }
}

// stage VJP with the hidden activations recomputed from the stage state; accumulates the weight gradients
template <int D>
HODE_DEV v4 ndp_vjp(const NeuralMf<D>& nn, NeuralGradAcc<D>& acc, const v4& e, const v4& k, const v4& gk, int g, int n) {
  constexpr int HT = NeuralMf<D>::HT;
  v4 a1[HT], u1[HT], u2;
  nn.hidden(e, a1);
  v4 av = nn.vjp(a1, k, gk, u2, u1);
  acc.add(u1, e, u2, a1, g, n);
  if (g == NeuralMf<D>::GD) av[NeuralMf<D>::RD] = 0.f;  // the Dose input is not a state
  return av;
}

// ------------------------------------------------------------------------------------------------ backward sweep
template <int D>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ndp_bwd_kernel(NdpArgs a) {
  constexpr int HT = NeuralMf<D>::HT;
  __shared__ __attribute__((aligned(16))) float lds[NeuralGradAcc<D>::kLdsFloats];
  const NdpLane<D> L(a);
  const int g = L.g;
  NeuralMf<D> nn;
  nn.load(a.nn, L.lane);
  NeuralGradAcc<D> acc;
  acc.init(lds);
  const size_t row = (size_t)a.nn.B * D;
  const size_t poff = (size_t)L.p * D;
  v4 lam_y = splat4(0.f), lam_f = splat4(0.f);
  float sig_d = 0.f;
  v4 a1[HT];

  for (int n = a.n_acc - 1; n >= 0; --n) {
    const double t0 = a.tape_t[n], dt = a.tape_dt[n];
    const double t1 = t0 + dt;
    const float t0f = (float)t0, dtf = (float)dt, t1f = (float)t1;
    const bool first = n == 0;
    const float rdt = div_f32(1.0f, dtf);
    float sd = 0.f;
    v4 k[7], Ys[7];
    float dose[7];
    Ys[0] = mf_load_rows<D>(a.tape_y + (size_t)n * row + poff, g);
    dose[0] = neural_dose(a.nn, L.p, L.dosage, first ? a.nn.t[0] : nextafter_down(t0f));
    k[0] = nn.rhs(mf_with_dose<D>(Ys[0], dose[0], g), a1);
#pragma unroll
    for (int i = 2; i <= 7; ++i) {
      v4 Y = Ys[0];
#pragma unroll
      for (int m = 0; m < i - 1; ++m) Y = vfma4(kDpBeta[i - 2][m] * dtf, k[m], Y);
      Ys[i - 1] = Y;
      dose[i - 1] = neural_dose(a.nn, L.p, L.dosage, dp_stage_time(i, t0f, dtf, t1f));
      k[i - 1] = nn.rhs(mf_with_dose<D>(Y, dose[i - 1], g), a1);
    }

    v4 gk[7], lam_y0 = splat4(0.f), lam_mid = splat4(0.f);
#pragma unroll
    for (int m = 0; m < 6; ++m) gk[m] = splat4(0.f);
    gk[6] = lam_f;
    const int jlo = a.tape_j[2 * n], jhi = a.tape_j[2 * n + 1];
    if (jlo < jhi) {
      // p'(x) / dt from the stage derivatives (the y0 terms of the quartic's coefficients cancel exactly), see dp_bwd_body
      v4 s1 = splat4(0.f), sm = splat4(0.f);
#pragma unroll
      for (int m = 0; m < 6; ++m) s1 = vfma4(kDpBeta[5][m], k[m], s1);
#pragma unroll
      for (int m = 0; m < 7; ++m) sm = vfma4(kDpMid[m], k[m], sm);
      const v4 ca = 4.0f * (2.0f * (k[6] - k[0]) - 8.0f * s1 + 16.0f * sm);
      const v4 cb = 3.0f * ((5.0f * k[0] - 3.0f * k[6]) + 14.0f * s1 - 32.0f * sm);
      const v4 cc = 2.0f * ((k[6] - 4.0f * k[0]) - 5.0f * s1 + 16.0f * sm);
      for (int j = jlo; j < jhi; ++j) {
        const float x = (float)(((double)a.nn.t[j] - t0) / (t1 - t0));
        const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
        const float P0 = 1.0f - 11.0f * x2 + 18.0f * x3 - 8.0f * x4;
        const float P1 = -5.0f * x2 + 14.0f * x3 - 8.0f * x4;
        const float Pm = 16.0f * x2 - 32.0f * x3 + 16.0f * x4;
        const float Q0 = dtf * (x - 4.0f * x2 + 5.0f * x3 - 2.0f * x4);
        const float Q1 = dtf * (x2 - 3.0f * x3 + 2.0f * x4);
        const v4 G = L.lv * mf_load_rows<D>(a.nn.grad_h + (size_t)j * row + poff, g);
        lam_y0 = vfma4(P0, G, lam_y0);
        lam_y = vfma4(P1, G, lam_y);
        lam_mid = vfma4(Pm, G, lam_mid);
        gk[0] = vfma4(Q0, G, gk[0]);
        gk[6] = vfma4(Q1, G, gk[6]);
        const v4 dp = ((k[0] + x * cc) + x2 * cb) + x3 * ca;
        sig_d = __builtin_fmaf(first ? -x : -1.0f, hsum4(G * dp), sig_d);
      }
      if (first) {
        sd += hsum4(gk[0] * k[0]) + hsum4((gk[6] - lam_f) * k[6]);
        sig_d += hsum4(lam_mid * sm);
      }
    }
    lam_y0 = lam_y0 + lam_mid;
#pragma unroll
    for (int m = 0; m < 7; ++m) gk[m] = vfma4(dtf * kDpMid[m], lam_mid, gk[m]);
    // stage 7: k7 = f(t1-, y1)
    v4 av = ndp_vjp<D>(nn, acc, mf_with_dose<D>(Ys[6], dose[6], g), k[6], gk[6], g, L.n);
    lam_y = lam_y + av;
    lam_y0 = lam_y0 + lam_y;
    if (first) sd += hsum4(lam_y * (Ys[6] - Ys[0]));
#pragma unroll
    for (int m = 0; m < 6; ++m) gk[m] = vfma4(kDpBeta[5][m] * dtf, lam_y, gk[m]);
#pragma unroll
    for (int st = 6; st >= 2; --st) {
      av = ndp_vjp<D>(nn, acc, mf_with_dose<D>(Ys[st - 1], dose[st - 1], g), k[st - 1], gk[st - 1], g, L.n);
      lam_y0 = lam_y0 + av;
      if (first) sd += hsum4(av * (Ys[st - 1] - Ys[0]));
#pragma unroll
      for (int m = 0; m < st - 1; ++m) gk[m] = vfma4(kDpBeta[st - 2][m] * dtf, av, gk[m]);
    }
    if (first) {
      av = ndp_vjp<D>(nn, acc, mf_with_dose<D>(Ys[0], dose[0], g), k[0], gk[0], g, L.n);
      lam_y0 = lam_y0 + av;
    }
    lam_y = lam_y0;
    lam_f = gk[0];
    sig_d = __builtin_fmaf(sd, rdt, sig_d);
  }
  lam_y = lam_y + L.lv * mf_load_rows<D>(a.nn.grad_h + poff, g);
  mf_store_rows<D>(a.nn.grad_y0 + poff, g, lam_y, L.live);
  const float sig = wave_sum(sig_d);  // rows >= D and dead patients carry zero cotangents
  if (L.lane == 0) a.partials[L.wave] = sig;
  acc.store(a.grad_partials + (size_t)L.wave * NeuralGradAcc<D>::NP, L.lane);
}

// ------------------------------------------------------------------------------- backward of the initial step size
// dp_initbwd_body for this rhs (no stage-time term).  PASS 1: the batch-global part of the cotangent of h0;
// PASS 2: everything into grad_y0 and a second block of weight-gradient partials.
template <int D, int PASS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ndp_initbwd_kernel(NdpArgs a) {
  constexpr int HT = NeuralMf<D>::HT;
  __shared__ __attribute__((aligned(16))) float lds[NeuralGradAcc<D>::kLdsFloats];
  const NdpLane<D> L(a);
  const int g = L.g;
  const DpInit in = *a.init;
  const float sigma = fold_waves(a.partials, a.n_waves, 1, 0);
  float* gout = a.grad_partials + (size_t)L.wave * NeuralGradAcc<D>::NP;
  if (!in.first_accepted || sigma == 0.0f) {
    if constexpr (PASS == 1) {
      if (L.lane == 0) a.partials[a.n_waves + L.wave] = 0.f;
    } else {
      NeuralGradAcc<D>::store_zero(gout, L.lane);
      if (L.wave == 0 && L.lane == 0) a.init->sigma = in.first_accepted ? sigma : 0.f;
    }
    return;
  }
  NeuralMf<D> nn;
  nn.load(a.nn, L.lane);
  NeuralGradAcc<D> acc;
  acc.init(lds);
  const size_t poff = (size_t)L.p * D;
  const float NN = (float)a.nn.B * (float)D;
  const float h0 = in.h0, d0 = in.d0, d1 = in.d1, d2 = in.d2, h1 = in.h1;
  const bool deg0 = d0 < 1e-5f || d1 < 1e-5f;
  const bool deg1 = d1 <= 1e-15f && d2 <= 1e-15f;
  const bool use_d2 = d2 > d1;
  const bool branch_a = 100.0f * h0 <= h1;
  float h0b = branch_a ? 100.0f * sigma : 0.0f;
  const float h1b = branch_a ? 0.0f : sigma;
  float d1b = 0.f, d2b = 0.f;
  if (deg1) {
    if (h0 * 1e-3f > 1e-6f) h0b = __builtin_fmaf(1e-3f, h1b, h0b);
  } else {
    const float mb = -0.2f * div_f32(h1, use_d2 ? d2 : d1) * h1b;
    if (use_d2) d2b = mb; else d1b = mb;
  }
  const float r2 = d2 * h0;
  float r2b = 0.f;
  if (d2b != 0.0f && r2 > 0.0f) {
    r2b = div_f32(d2b, h0);
    h0b -= div_f32(d2b * d2, h0);
  }
  v4 a1[HT];
  const v4 y = mf_load_rows<D>(a.nn.y0 + poff, g);
  const float t0f = a.nn.t[0];
  const v4 e0 = mf_with_dose<D>(y, neural_dose(a.nn, L.p, L.dosage, t0f), g);
  const v4 f0 = nn.rhs(e0, a1);
  const v4 e1 = mf_with_dose<D>(vfma4(h0, f0, y), neural_dose(a.nn, L.p, L.dosage, add_rn(t0f, h0)), g);
  const v4 f1 = nn.rhs(e1, a1);
  const v4 scale = ndp_scale<D>(a, y);
  const float cw = r2b != 0.0f ? div_f32(r2b, NN * r2) * L.lv : 0.0f;
  v4 w, wb, f1b;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    w[r] = L.valid[r] != 0.0f ? div_f32(f1[r] - f0[r], scale[r]) : 0.0f;
    wb[r] = cw * w[r];
    f1b[r] = div_f32(wb[r], scale[r]);
  }
  const v4 y1b = ndp_vjp<D>(nn, acc, e1, f1, f1b, g, L.n);
  if constexpr (PASS == 1) {
    const float sp = wave_sum(hsum4(y1b * f0));
    if (L.lane == 0) a.partials[a.n_waves + L.wave] = sp;
  } else {
    h0b += fold_waves(a.partials + a.n_waves, a.n_waves, 1, 0);
    float d0b = 0.f;
    if (!deg0) {
      d0b = div_f32(0.01f, d1) * h0b;
      d1b -= div_f32(h0, d1) * h0b;
    }
    const float cv = d1 > 0.0f ? div_f32(d1b, NN * d1) * L.lv : 0.0f;
    const float cu = d0 > 0.0f ? div_f32(d0b, NN * d0) * L.lv : 0.0f;
    v4 f0b, yb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rs = div_f32(1.0f, scale[r]);
      const float v = f0[r] * rs * L.valid[r], u = y[r] * rs * L.valid[r];
      const float vb = cv * v, ub = cu * u;
      f0b[r] = __builtin_fmaf(h0, y1b[r], (vb - wb[r]) * rs);
      const float sb = -(wb[r] * w[r] + vb * v + ub * u) * rs;
      const float sgn = y[r] > 0.0f ? 1.0f : (y[r] < 0.0f ? -1.0f : 0.0f);
      yb[r] = y1b[r] + ub * rs + sb * a.rtol * sgn;
    }
    const v4 a0 = ndp_vjp<D>(nn, acc, e0, f0, f0b, g, L.n);
    const v4 gy = mf_load_rows<D>(a.nn.grad_y0 + poff, g) + yb + a0;
    mf_store_rows<D>(a.nn.grad_y0 + poff, g, gy, L.live);
    acc.store(gout, L.lane);
    if (L.wave == 0 && L.lane == 0) a.init->sigma = sigma;
  }
}
// ------------------------------------------------------------------------------------------------ host side
// the workspace of hode_adaptive_host.hpp without the Roche kernels' slots; one NeuralGradAcc block per wave
template <int D>
AdaptiveLayout nd_layout(const hode_solve_desc* d) {
  return adaptive_layout((d->batch + 15) / 16, (size_t)d->batch * D, d->max_steps, d->flags & HODE_FLAG_NO_TAPE, 0,
                         NeuralGradAcc<D>::NP);
}

template <int D>
NdpArgs nd_args(const hode_solve_desc* d, const AdaptiveLayout& L) {
  NdpArgs a{};
  char* ws = (char*)d->workspace;
  a.nn.t = d->t; a.nn.y0 = d->y0; a.nn.dosage = d->dosage; a.nn.dose_times = d->dose_times;
  a.nn.w1 = d->w1; a.nn.b1 = d->b1; a.nn.w2 = d->w2; a.nn.b2 = d->b2; a.nn.w2t = nullptr;
  a.nn.h = d->h; a.nn.grad_h = d->grad_h; a.nn.grad_y0 = d->grad_y0;
  a.nn.B = d->batch; a.nn.T = d->n_times; a.nn.K = d->n_dose; a.nn.perturb = 0;
  a.ctrl = (DpCtrl*)(ws + L.ctrl);
  a.init = (DpInit*)(ws + L.ctrl + kInitOffset);
  a.partials = (float*)(ws + L.partials);
  a.kbuf = (float*)(ws + L.kbuf);
  a.tape_t = (double*)(ws + L.tape_t);
  a.tape_dt = (double*)(ws + L.tape_dt);
  a.tape_j = (int*)(ws + L.tape_j);
  a.tape_y = (float*)(ws + L.tape_y);
  a.grad_partials = (float*)(ws + L.grad_partials);
  a.grad_w1 = d->grad_w1; a.grad_b1 = d->grad_b1; a.grad_w2 = d->grad_w2; a.grad_b2 = d->grad_b2;
  a.n_waves = (d->batch + 15) / 16;
  a.max_steps = d->max_steps;
  a.ring = (d->flags & HODE_FLAG_NO_TAPE) ? 1 : 0;
  a.rtol = (float)d->rtol; a.atol = (float)d->atol;
  return a;
}

// attempts between two reads of the controller record (hode_adaptive_host.hpp): first / min / max
constexpr ChunkPolicy kNdChunks = {32, 16, 1024};

template <int D>
int nd_fwd(const hode_solve_desc* d, hipStream_t s) {
  const AdaptiveLayout lay = nd_layout<D>(d);
  if (!d->workspace || d->workspace_bytes < lay.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, lay.total);
  NdpArgs a = nd_args<D>(d, lay);
  const dim3 grid(a.n_waves), block(64);
  hipLaunchKernelGGL((ndp_fwd_kernel<D, 0>), grid, block, 0, s, a);
  hipLaunchKernelGGL((ndp_fwd_kernel<D, 1>), grid, block, 0, s, a);
  if (int e = hip_fail(hipGetLastError(), "neural dopri5 init launch")) return e;
  DpCtrl host{};
  const auto enqueue = [&](int i) {
    a.attempt = i;
    hipLaunchKernelGGL((ndp_fwd_kernel<D, 2>), grid, block, 0, s, a);
    return 0;  // the loop looks at hipGetLastError once per chunk
  };
  if (int e = adaptive_attempts(d, a.ctrl, kNdChunks, "neural dopri5 attempt launch", s, enqueue, &host)) return e;
  return adaptive_report(d, host, s);
}

// the backward's launch sequence: the sweep over the tape and its fold, then (unless the first step is detached) the two
// passes of the initial step size's backward and their fold.  (Internal linkage, like the helpers of hode_adaptive_host.hpp;
// nd_fwd keeps the external linkage under which its instantiations are among the names both libraries have always held.)
template <int D>
static int nd_bwd(const hode_solve_desc* d, hipStream_t s) {
  const AdaptiveLayout lay = nd_layout<D>(d);
  if (!d->workspace || d->workspace_bytes < lay.total)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, lay.total);
  NdpArgs a = nd_args<D>(d, lay);
  a.n_acc = *d->host_n_accepted;
  if (a.n_acc < 0 || a.n_acc > d->max_steps) return fail(HODE_E_SIZE, "n_accepted %d outside the tape", a.n_acc);
  const dim3 grid(a.n_waves), block(64);
  const dim3 fgrid(NeuralGradAcc<D>::NP);
  hipLaunchKernelGGL((ndp_bwd_kernel<D>), grid, block, 0, s, a);
  hipLaunchKernelGGL((neural_grad_fold_kernel<D>), fgrid, block, 0, s, a.grad_partials, a.n_waves, a.grad_w1, a.grad_b1, a.grad_w2, a.grad_b2);
  if (a.n_acc > 0 && !(d->flags & HODE_FLAG_DETACH_FIRST_STEP)) {
    hipLaunchKernelGGL((ndp_initbwd_kernel<D, 1>), grid, block, 0, s, a);
    hipLaunchKernelGGL((ndp_initbwd_kernel<D, 2>), grid, block, 0, s, a);
    hipLaunchKernelGGL((neural_grad_fold_kernel<D>), fgrid, block, 0, s, a.grad_partials, a.n_waves, a.grad_w1, a.grad_b1, a.grad_w2, a.grad_b2);
  }
  return hip_fail(hipGetLastError(), "neural dopri5 backward launch");
}

}  // namespace hode
