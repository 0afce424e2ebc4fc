// The kernels of libhode_real_pp.so at one hidden-tile count HT = HODE_REAL_PP_HT (hidden_dim <= 16 HT): Dormand-Prince
// 5(4) with PER-PATIENT step control for the real-data hybrid rhs, and its discrete adjoint.
//
// Layout: that of ../hode_real_mf.hpp with the ragged tile -- a wave carries 16 patients, patient n of the tile is column n
// of the MFMA operands and lives in the four lanes n, n + 16, n + 32, n + 48 (lane group g holds rows 4g .. 4g + 3 of the
// GRU tile; g == 0 also the four expert states).  The rhs reads the time only through its column's own dose lookup, so the
// 16 patients of a tile ATTEMPT TOGETHER, each with its own t0, dt and accept flag in its lanes: no divergence around the
// MFMAs, exec stays full.  A patient that is done, or whose attempt was rejected, keeps its state by a select.  The one
// thing the controller needs across lanes is the sum of a patient's error terms over its four lanes (col_sum: the same
// bits in all four, so they take the same decision).  The loops end on wave-uniform votes and are bounded by
// max_attempts / max_steps / T.
//
// Compiled from the shared headers, not restated: the rhs and its VJP, the weight-gradient accumulator and its fold, the
// dose table and the state I/O (../hode_real_mf.hpp, ../hode_real_args.hpp); the tableau, the stage times and the step
// factor (../hode_dopri5_kernels.hpp).  What is here is the controller with its step clipping, the tape and the sweep.
//
// Registers: a stage's activations (Net::Stage, 28 + 8 HT floats) are never kept across a step.  The forward keeps the
// seven stage derivatives; the sweep recomputes them from the taped state, then recomputes each stage's activations from
// them immediately before that stage's VJP.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../hode_dopri5_kernels.hpp"
#include "../hode_real_mf.hpp"
#include "hode_real_pp.hpp"

#ifndef HODE_REAL_PP_HT
#error "compile with -DHODE_REAL_PP_HT=<1 .. 4>"
#endif

namespace hode {

constexpr int kHT = HODE_REAL_PP_HT;
static_assert(kHT >= 1 && kHT <= 4, "hidden tiles");
static_assert(RealGradAcc<kHT>::NP == real_side_partial_floats(kHT), "partial block size");

// sum over the four lanes n, n + 16, n + 32, n + 48 of a column: the two additions commute, so all four lanes hold the
// same bits and may branch on the value
HODE_DEV float col_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

HODE_DEV v4 fma4(float c, const v4& k, const v4& y) { return __builtin_elementwise_fma(v4{c, c, c, c}, k, y); }
HODE_DEV v4 div4(const v4& a, const v4& b) { return v4{div_f32(a[0], b[0]), div_f32(a[1], b[1]), div_f32(a[2], b[2]), div_f32(a[3], b[3])}; }
HODE_DEV v4 abs4(const v4& a) { return __builtin_elementwise_abs(a); }
HODE_DEV v4 sel4(bool c, const v4& a, const v4& b) { return c ? a : b; }

// which of a lane's eight values are components of its patient's state
struct PpMask {
  bool x;     // the four expert states: lanes g == 0
  bool h[4];  // GRU rows 4g + r < M
  float cnt;  // D
  HODE_DEV PpMask(int g, int M) : x(g == 0), cnt((float)(M + 4)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = 4 * g + r < M;
  }
  // RMS over the patient's D components of (uX, uH); values outside the mask are not read (they may be 0 / 0)
  HODE_DEV float rms(const v4& uX, const v4& uH) const {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float u = x ? uX[r] : 0.f;
      s = __builtin_fmaf(u, u, s);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float u = h[r] ? uH[r] : 0.f;
      s = __builtin_fmaf(u, u, s);
    }
    return __builtin_sqrtf(col_sum(s) / cnt);
  }
  HODE_DEV bool nonfinite(const v4& X, const v4& Hs) const {
    float nf = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((x && !__builtin_isfinite(X[r])) || (h[r] && !__builtin_isfinite(Hs[r]))) nf = 1.0f;
    return col_sum(nf) != 0.0f;
  }
};

// state and time of stage Q + 1 (Q = 1 .. 6: the index of its derivative) from the step's start state and the derivatives
// before it: dp_stages' combination and dp_stage_time
template <int Q>
HODE_DEV void pp_stage_in(const v4& X, const v4& Hs, const v4 (&kX)[7], const v4 (&kH)[7], float t0f, float dtf, float t1f, v4& YX,
                          v4& YH, float& ti) {
  ti = dp_stage_time(Q + 1, t0f, dtf, t1f);
  // the increment is summed first and added to the state once (torchdiffeq's y0 + k.matmul(beta dt)): one rounding at the
  // size of the state instead of Q.  At rtol 1e-7 the tolerance IS that rounding, and the controller would otherwise chase it
  v4 iX = v4{0.f, 0.f, 0.f, 0.f}, iH = iX;
#pragma unroll
  for (int m = 0; m < Q; ++m) {
    const float c = kDpBeta[Q - 1][m] * dtf;
    iX = fma4(c, kX[m], iX);
    iH = fma4(c, kH[m], iH);
  }
  YX = X + iX;
  YH = Hs + iH;
}
// The cotangent of derivative k_{Q+1}, pulled from the cotangents c[Q'] of the stage states Q' + 1 > Q + 1 it was combined
// into (c[6]: the step's end state), in the order Q' = 6 .. Q + 1.  Pulled when stage Q + 1 is reached, not pushed when
// c[Q'] is formed: the sweep then holds Q derivatives and 6 - Q cotangents at stage Q + 1, six vectors instead of eleven.
template <int Q>
HODE_DEV void pp_pull(const v4 (&cX)[7], const v4 (&cH)[7], float dtf, v4& gX, v4& gH) {
  gX = gH = v4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qq = 6; qq > Q; --qq) {
    const float c = kDpBeta[qq - 1][Q] * dtf;
    gX = fma4(c, cX[qq], gX);
    gH = fma4(c, cH[qq], gH);
  }
}

// ------------------------------------------------------------------------------------------------------- forward
template <int HT>
HODE_DEV void real_pp_fwd_body(const RealPpArgs& a, const RealTileRagged tile) {
  typedef RealMf<HT, RealTileRagged> Net;
  typedef typename Net::Stage Stage;
  const RealArgs& ra = a.r;
  const int M = tile.m(), D = M + 4;
  const int lane = threadIdx.x;
  Net nn;
  nn.load(ra, tile, lane);
  const int g = nn.g;
  const bool g0 = g == 0;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < ra.B;
  const int p = live ? pr : ra.B - 1;  // idle columns shadow the last patient and never store
  const size_t B = ra.B;
  const size_t row = B * D;
  const size_t poff = (size_t)p * D;
  const PpMask mask(g, M);
  if (g0) real_dose_table(ra, p, nn.kel);  // each lane reads back only its own column

  Stage s;
  auto eval = [&](const v4& YX, const v4& YH, float t, v4& kX, v4& kH) __attribute__((always_inline)) {
    s.X = YX;
    s.Hs = YH;
    real_set_dose(ra, p, nn.kel, g0, s, t);
    nn.rhs(s, kH);
    kX = s.KX;
  };

  // ---- k1 and Hairer's initial step from this patient's own norms (pp_fwd_body's arithmetic on the tile's registers)
  v4 X, Hs, k1X, k1H;
  real_load_state(tile, g, ra.y0 + poff, X, Hs);
  if (live) real_store_state(tile, g, ra.h + poff, X, Hs);
  const float tf0 = ra.t[0];
  eval(X, Hs, tf0, k1X, k1H);
  double dt;
  {
    const v4 scX = a.atol + abs4(X) * a.rtol, scH = a.atol + abs4(Hs) * a.rtol;
    const float d0 = mask.rms(div4(X, scX), div4(Hs, scH));
    const float d1 = mask.rms(div4(k1X, scX), div4(k1H, scH));
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : div_f32(0.01f * d0, d1);
    v4 fX, fH;
    eval(fma4(h0, k1X, X), fma4(h0, k1H, Hs), add_rn(tf0, h0), fX, fH);
    const float d2 = div_f32(mask.rms(div4(fX - k1X, scX), div4(fH - k1H, scH)), h0);
    float h1;
    if (d1 <= 1e-15f && d2 <= 1e-15f) h1 = fmaxf(1e-6f, h0 * 1e-3f);
    else h1 = powf(div_f32(0.01f, fmaxf(d1, d2)), 0.2f);
    dt = (double)fminf(100.0f * h0, h1);
  }

  // ---- the attempt loop: fp64 clock per patient, fp32 stage times, the tile in step
  double t0 = (double)tf0;
  int n_acc = 0, n_rej = 0, j_next = 1, status = 0;
  bool run = live && ra.T > 1;
  for (int it = 0;; ++it) {
    const bool bad = mask.nonfinite(X, Hs);  // cross-lane: outside the per-patient branches
    if (run) {
      if (j_next >= ra.T) run = false;
      else if (bad) { status |= HODE_STATUS_NONFINITE; run = false; }
      else if (!(t0 + dt > t0)) { status |= HODE_STATUS_DT_UNDERFLOW; run = false; }
      else if (n_acc >= a.max_steps || it >= a.max_attempts) { status |= HODE_STATUS_MAX_STEPS; run = false; }
    }
    if (__builtin_amdgcn_ballot_w64(run) == 0) break;  // the whole tile is done; it <= max_attempts
    // no step crosses an output time
    const double tj = (double)ra.t[min(j_next, ra.T - 1)];
    const double rem = tj - t0;
    const bool clip = !(dt < rem);
    const double dtu = run ? (clip ? rem : dt) : 0.0;  // a patient that is done attempts a step of length 0 and discards it
    const double t1 = run ? (clip ? tj : t0 + dtu) : t0;
    const float t0f = (float)t0, dtf = (float)dtu, t1f = (float)t1;
    v4 kX[7], kH[7], YX, YH;
    kX[0] = k1X;
    kH[0] = k1H;
    float ti;
    pp_stage_in<1>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[1], kH[1]);
    pp_stage_in<2>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[2], kH[2]);
    pp_stage_in<3>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[3], kH[3]);
    pp_stage_in<4>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[4], kH[4]);
    pp_stage_in<5>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[5], kH[5]);
    pp_stage_in<6>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti); eval(YX, YH, ti, kX[6], kH[6]);
    // (YX, YH) is y1: the last row of the tableau is the solution's weights
    v4 eX = v4{0.f, 0.f, 0.f, 0.f}, eH = eX;
#pragma unroll
    for (int m = 0; m < 7; ++m) {
      eX = fma4(dtf * kDpErr[m], kX[m], eX);
      eH = fma4(dtf * kDpErr[m], kH[m], eH);
    }
    const v4 tolX = a.atol + a.rtol * __builtin_elementwise_max(abs4(X), abs4(YX));
    const v4 tolH = a.atol + a.rtol * __builtin_elementwise_max(abs4(Hs), abs4(YH));
    const float ratio = mask.rms(div4(eX, tolX), div4(eH, tolH));
    const bool accept = run && ratio <= 1.0f;  // a NaN ratio is a rejection, and its NaN factor ends the patient with DT_UNDERFLOW
    if (accept) {  // run implies live; n_acc < max_steps was checked above
      const size_t e = (size_t)n_acc * B + (size_t)p;
      if (!a.no_tape) {
        if (g0) {
          a.tape_t[e] = t0;
          a.tape_dt[e] = dtu;
          a.tape_j[e] = clip ? j_next : -1;
        }
        real_store_state(tile, g, a.tape_y + e * D, X, Hs);
      }
      if (clip) real_store_state(tile, g, ra.h + (size_t)j_next * row + poff, YX, YH);
    }
    if (run) {
      if (accept) {
        ++n_acc;
        t0 = t1;
        if (clip) ++j_next;
      } else {
        ++n_rej;
      }
      dt = dtu * dp_step_factor(ratio);
    }
    X = sel4(accept, YX, X);
    Hs = sel4(accept, YH, Hs);
    k1X = sel4(accept, kX[6], k1X);  // FSAL
    k1H = sel4(accept, kH[6], k1H);
  }
  if (live && g0) {
    a.n_acc[p] = n_acc;
    a.n_rej[p] = n_rej;
    a.pstatus[p] = status;
    if (status) atomicOr(a.status, status);
  }
}

template <int HT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_pp_fwd_kernel(RealPpArgs a, int M) {
  real_pp_fwd_body<HT>(a, RealTileRagged{M});
}

// ------------------------------------------------------------------------------------------------------ backward
// The discrete adjoint of the accepted steps, every step size a constant (pp_bwd_body's chain without the dense output).
// The sweep is wave-uniform: n runs from the tile's largest n_acc down to 0, and a patient with n >= n_acc[p] has not
// started -- it recomputes a step of length 0 from the zero state with zero cotangents, so what it adds to every sum is
// exactly zero and its lam stays zero.  All patients reach n == 0 together, where g1 goes through the VJP of k1.
template <int HT>
HODE_DEV void real_pp_bwd_body(const RealPpArgs& a, const RealTileRagged tile, float* lds) {
  typedef RealMf<HT, RealTileRagged> Net;
  typedef typename Net::Stage Stage;
  constexpr int NT2 = 2 * HT;
  const RealArgs& ra = a.r;
  const int M = tile.m(), D = M + 4;
  const int lane = threadIdx.x;
  Net nn;
  nn.load(ra, tile, lane);
  const int g = nn.g;
  const bool g0 = g == 0;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < ra.B;
  const int p = live ? pr : ra.B - 1;
  const size_t B = ra.B;
  const size_t row = B * D;
  const size_t poff = (size_t)p * D;
  RealGradAcc<HT> acc;
  acc.init(lds);
  if (g0) real_dose_table(ra, p, nn.kel);

  const int n_mine = live ? min(max(a.n_acc[p], 0), a.max_steps) : 0;  // idle columns sweep nothing and add zeros
  int n_max = n_mine;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) n_max = max(n_max, __shfl_xor(n_max, m, 64));
  n_max = __builtin_amdgcn_readfirstlane(n_max);

  const v4 zero = v4{0.f, 0.f, 0.f, 0.f};
  float dth[3] = {0.f, 0.f, 0.f};
  v4 lamX = zero, lamH = zero, lfX = zero, lfH = zero;  // cotangents of the state and of k1 of the step after
  Stage s;
  const float tf0 = ra.t[0];
  for (int n = n_max - 1; n >= 0; --n) {
    const bool on = n < n_mine;
    double t0 = (double)tf0, dtu = 0.0;
    int j = -1;
    v4 X = zero, Hs = zero;
    if (on) {
      const size_t e = (size_t)n * B + (size_t)p;
      t0 = a.tape_t[e];
      dtu = a.tape_dt[e];
      j = a.tape_j[e];
      real_load_state(tile, g, a.tape_y + e * D, X, Hs);
      if (j >= 1 && j < ra.T) {  // the step reached output j: its cotangent first
        v4 ghX, ghH;
        real_load_state(tile, g, ra.grad_h + (size_t)j * row + poff, ghX, ghH);
        lamX = lamX + ghX;
        lamH = lamH + ghH;
      }
    }
    const double t1 = (j >= 1 && j < ra.T) ? (double)ra.t[j] : t0 + dtu;
    const float t0f = (float)t0, dtf = (float)dtu, t1f = (float)t1;
    const float tk1 = n == 0 ? tf0 : nextafter_down(t0f);  // k1 of step n IS k7 of step n - 1

    // the derivatives the stage states are combined from (k1 .. k6; k7 enters no stage state); the activations are not kept
    v4 kX[7], kH[7];
    {
      v4 YX, YH;
      float ti;
      s.X = X; s.Hs = Hs; real_set_dose(ra, p, nn.kel, g0, s, tk1); nn.rhs(s, kH[0]); kX[0] = s.KX;
#define HODE_PP_STAGE(Q)                                                    \
  pp_stage_in<Q>(X, Hs, kX, kH, t0f, dtf, t1f, YX, YH, ti);                  \
  s.X = YX; s.Hs = YH; real_set_dose(ra, p, nn.kel, g0, s, ti); nn.rhs(s, kH[Q]); kX[Q] = s.KX;
      HODE_PP_STAGE(1) HODE_PP_STAGE(2) HODE_PP_STAGE(3) HODE_PP_STAGE(4) HODE_PP_STAGE(5)
      kX[6] = kH[6] = zero;
#undef HODE_PP_STAGE
    }
    // (aX, aH) = J^T (gX, gH) at stage Q + 1, whose activations are recomputed here, immediately before
    auto vjp = [&](auto qc, const v4& gX, const v4& gH, v4& aX, v4& aH) __attribute__((always_inline)) {
      constexpr int Q = decltype(qc)::value;
      float ti = tk1;
      if constexpr (Q == 0) {
        s.X = X;
        s.Hs = Hs;
      } else {
        pp_stage_in<Q>(X, Hs, kX, kH, t0f, dtf, t1f, s.X, s.Hs, ti);
      }
      real_set_dose(ra, p, nn.kel, g0, s, ti);
      v4 kh;
      nn.rhs(s, kh);
      v4 U1[NT2], ur, uz, uh;
      float u12, u22;
      nn.vjp(s, gX, gH, aX, aH, U1, u12, u22, ur, uz, uh, dth);
      acc.add(U1, s.ah, s.X, u12, u22, uh, uz, ur, s.RH, s.Hs, g, nn.n);
    };
    v4 cX[7], cH[7], gX, gH;  // c[Q]: the cotangent of stage state Q + 1 (Q = 1 .. 5), c[6] that of the end state
    cX[0] = cH[0] = zero;
    // stage 7: k7 = f(t1-, y1); y1 is the state AND the last stage's input
    vjp(std::integral_constant<int, 6>{}, lfX, lfH, cX[6], cH[6]);
    cX[6] = lamX = lamX + cX[6];
    cH[6] = lamH = lamH + cH[6];
    // stages 6 .. 2
#define HODE_PP_VJP(Q)                                             \
  pp_pull<Q>(cX, cH, dtf, gX, gH);                                  \
  vjp(std::integral_constant<int, Q>{}, gX, gH, cX[Q], cH[Q]);      \
  lamX = lamX + cX[Q]; lamH = lamH + cH[Q];
    HODE_PP_VJP(5) HODE_PP_VJP(4) HODE_PP_VJP(3) HODE_PP_VJP(2) HODE_PP_VJP(1)
#undef HODE_PP_VJP
    // g1 is handed to step n - 1 (FSAL); at n == 0 (wave-uniform) it goes through the VJP of k1
    pp_pull<0>(cX, cH, dtf, lfX, lfH);
    if (n == 0) {
      v4 aX, aH;
      vjp(std::integral_constant<int, 0>{}, lfX, lfH, aX, aH);
      lamX = lamX + aX;
      lamH = lamH + aH;
    }
  }
  // output 0 is y0 itself
  {
    v4 ghX, ghH;
    real_load_state(tile, g, ra.grad_h + poff, ghX, ghH);
    if (live) real_store_state(tile, g, ra.grad_y0 + poff, lamX + ghX, lamH + ghH);
  }
  // only lanes g == 0 of live patients carry scalar-gradient terms (X and the cotangents are zero elsewhere)
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    const float v = wave_sum(g0 ? dth[jj] : 0.f);
    if (lane == 0) ra.partials[(size_t)blockIdx.x * 3 + jj] = v;
  }
  acc.store(ra.tape + (size_t)blockIdx.x * RealGradAcc<HT>::NP, lane);
}

template <int HT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void real_pp_bwd_kernel(RealPpArgs a, int M) {
  __shared__ __attribute__((aligned(16))) float lds[RealGradAcc<HT>::kLdsFloats];
  real_pp_bwd_body<HT>(a, RealTileRagged{M}, lds);
}

// the three M x M blocks are written with M as row stride; padded rows and columns of the tiles are never written
template <int HT>
__global__ __launch_bounds__(64) void real_pp_fold_kernel(const float* __restrict__ partials, int n_waves, int H, int M,
                                                          float* __restrict__ gw) {
  real_grad_fold<HT>(partials, n_waves, H, M, gw);
}

int HODE_CAT(real_pp_launch_ht, HODE_REAL_PP_HT)(bool bwd, const RealPpArgs& a, int M, float* grad_w, hipStream_t s) {
  const dim3 grid((a.r.B + 15) / 16);
  if (!bwd) {
    hipLaunchKernelGGL((real_pp_fwd_kernel<kHT>), grid, dim3(64), 0, s, a, M);
    return hip_fail(hipGetLastError(), "real per-patient dopri5 forward launch");
  }
  hipLaunchKernelGGL((real_pp_bwd_kernel<kHT>), grid, dim3(64), 0, s, a, M);
  hipLaunchKernelGGL((real_pp_fold_kernel<kHT>), dim3(RealGradAcc<kHT>::NP), dim3(64), 0, s, a.r.tape, (int)grid.x, a.r.H, M, grad_w);
  return hip_fail(hipGetLastError(), "real per-patient dopri5 sweep launch");
}

}  // namespace hode
