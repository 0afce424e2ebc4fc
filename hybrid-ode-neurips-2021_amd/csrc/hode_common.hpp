// Device-side helpers shared by the hode kernels (gfx950 only: wave64, DPP, v_exp/v_rcp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HODE_DEV __device__ __forceinline__

namespace hode {

constexpr int kWave = 64;

// ---------------------------------------------------------------------------------------------------------
// transcendental helpers.  Every "bound" below is enforced pointwise, against float64 on about 2.7 million inputs per
// helper, by tests/test_hip_helpers.py through the test-only probe library (csrc/probe): it is the derived bound of
// tests/helper_cases.py (first order in the measured errors of v_exp_f32 / v_log_f32 / v_rcp_f32, each <= 1 ulp, and half an
// ulp per fp32 rounding).  "measured" is the largest error one run on an MI355X found: a record for
// orientation, which no test holds.  The hardware primitives flush: v_exp_f32 returns 0 for a result below 2^-126,
// v_log_f32 and v_rcp_f32 read a subnormal operand as 0, and v_rcp_f32 returns 0 for a result below 2^-126.
// ---------------------------------------------------------------------------------------------------------

// exp(x): hardware exp2 of the rounded product x*log2(e), corrected by the product's rounding residual (exact via fma);
// 5 instructions.  The fp32 log2(e) is off by 1.3e-8 relative and the residual does not correct that, so the relative
// error grows with |x|: bound (3 + 0.224 |x|) 2^-24 relative, i.e. 3.2 ulp at |x| = 1, 5 ulp at 8, 21 ulp at 80, 23 ulp at
// 88; measured 1.26 ulp below 1, 2.76 ulp below 8, 20.9 ulp up to 88.72.  A result below 2^-126 (x < -87.33) is
// flushed to 0.
// DOMAIN: finite x with |x * log2(e)| < 128 (x below the overflow threshold 88.72; below -87.33 the result is 0).  Outside
// it the correction term is 0 * inf or inf - inf: exp_f32(-inf) = exp_f32(+inf) = NaN, |x| > 2.3e38 (x*log2(e) overflows)
// = NaN, and past 88.72 the result is +inf when the residual is positive and NaN otherwise.  Mending this inside the
// helper costs the flagship step 3 % even with the select off the dependent chain, so the call
// sites are split instead.  exp_f32 is for arguments that are finite and <= 0 by construction:
//   hode_roche.hpp DoseSched::at    kel*(tau - t) under the `t >= tau` select: tau - t <= 0, and the elimination rate kel >= 0
//                                   (a negative or non-finite kel is outside the model)
//   hode_real_args.hpp real_dose    kel*(n - t) with n = min(Ta, floor(t)) <= t; real_dose_table: -kel
//   hode_readout_mlp.hip            the ELU's z <= 0 branch under the `z > 0 ?` select
// Arguments of either sign that nothing bounds (0.5*log_var, y, z - 5 in hode_mckl.hip and flow/hode_flow.hip) go through
// exp_full_f32.
HODE_DEV float exp_f32(float x) {
  const float l2e = 1.4426950408889634f;
  const float t = x * l2e;
  const float lo = __builtin_fmaf(x, l2e, -t);
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, lo * 0.6931471805599453f, e);
}

// exp(x) on the whole line, bit for bit exp_f32 inside its domain: for |t| >= 128 (also +-inf) exp2 returns 0 or +inf, which
// is the limit itself, and the correction factor is replaced by 1 so that the fma keeps it.  exp_full_f32(-inf) = 0,
// exp_full_f32(+inf) = +inf, +inf past 88.72, 0 below -103.97 and where x*log2(e) overflows; NaN propagates.
HODE_DEV float exp_full_f32(float x) {
  const float l2e = 1.4426950408889634f;
  const float t = x * l2e;
  const float lo = __builtin_fmaf(x, l2e, -t);
  const float e = __builtin_amdgcn_exp2f(t);
  const float c = __builtin_fabsf(t) < 128.0f ? lo * 0.6931471805599453f : 1.0f;
  return __builtin_fmaf(e, c, e);
}

// natural log through the hardware log2 (only used by the Hill-exponent gradients): bound 2.6 ulp, measured 1.92 ulp for
// normal x > 0.  log_f32(1) = 0, log_f32(+-0) = -inf, and a subnormal x also gives -inf (v_log_f32 reads it as 0).
HODE_DEV float log_f32(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }

// tanh(x) = 1 - 2 / (exp(2x) + 1): v_mul, v_exp, v_add, v_rcp, v_fma.  ABSOLUTE error: bound 4.2e-7 over the whole
// line (largest for x < 0, where 1 - tanh is near 2), measured 2.1e-7; the relative error grows for |x| << 1 (the result
// for |x| < 3e-8 is 0), which does not matter here because tanh feeds an additive rate dy/dt.  NaN propagates,
// +-inf -> +-1, and tanh_f32(-0) = +0.
HODE_DEV float tanh_f32(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);  // exp(2x)
  return __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), -2.0f, 1.0f);
}

// tanh with RELATIVE accuracy (odd polynomial below 0.625, exp form above): bound 3.1 ulp (just above the branch point),
// measured 1.51 ulp; odd, so the sign of zero is kept; +-inf -> +-1.  Kept for the encoder gates.
HODE_DEV float tanh_precise_f32(float x) {
  float ax = __builtin_fabsf(x);
  float u = x * x;
  float p = -0.005508354399353266f;
  p = __builtin_fmaf(p, u, 0.020461998879909515f);
  p = __builtin_fmaf(p, u, -0.05368518456816673f);
  p = __builtin_fmaf(p, u, 0.13330785930156708f);
  p = __builtin_fmaf(p, u, -0.3333325684070587f);
  float small = __builtin_fmaf(ax * u, p, ax);
  float e = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);
  float big = __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), -2.0f, 1.0f);
  float r = ax < 0.625f ? small : big;
  return __builtin_copysignf(r, x);
}

// logistic sigmoid via tanh: sigma(x) = 0.5 + 0.5 tanh(x/2).  ABSOLUTE error: bound 2.1e-7, measured 1.0e-7; below
// x = -17 the result is 0 or 2^-25-spaced, not the tiny true value.
HODE_DEV float sigmoid_f32(float x) { return __builtin_fmaf(tanh_f32(0.5f * x), 0.5f, 0.5f); }

// ---------------------------------------------------------------------------------------------------------
// packed fp32: v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 retire TWO fp32 operations in the issue slot of one
// (tools/micro/issue_rates.hip: 2.28 ns per wave-instruction for v_fma_f32 and for v_pk_fma_f32 alike, dependent or
// not) -- the solver kernels are bound by issue slots, so the paired algebra is written with this type explicitly
// (the SLP vectoriser's automatic pairing costs more v_mov than it saves and is switched off for these files).
// ---------------------------------------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));
HODE_DEV f2 splat2(float x) { f2 r = {x, x}; return r; }
HODE_DEV f2 pair2(float a, float b) { f2 r = {a, b}; return r; }
HODE_DEV float vfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
HODE_DEV f2 vfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
HODE_DEV f2 vfma(float a, f2 b, f2 c) { return __builtin_elementwise_fma(splat2(a), b, c); }
HODE_DEV f2 vfma(f2 a, float b, f2 c) { return __builtin_elementwise_fma(a, splat2(b), c); }
template <class V> HODE_DEV V vsplat(float x);
template <> HODE_DEV float vsplat<float>(float x) { return x; }
template <> HODE_DEV f2 vsplat<f2>(float x) { return splat2(x); }
HODE_DEV float hsum(f2 v) { return v.x + v.y; }
// bit for bit the scalar tanh_f32
HODE_DEV f2 tanh_f32(f2 x) {  // the two transcendentals stay scalar, the three arithmetic steps are packed
  const f2 t = x * splat2(2.885390081777927f);
  const f2 e = pair2(__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)) + splat2(1.0f);
  return vfma(pair2(__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)), splat2(-2.0f), splat2(1.0f));
}
// the scaled form of tanh: tanh(z) = 1 - 2 / (exp2(z') + 1) for an argument z' = 2 log2(e) z whose factor the caller folded
// into its weights (v_exp, add, v_rcp, fma per value, the add and the fma on packed pairs).  Accuracy as tanh_f32 without the
// argument's rounding; every copy (these and NeuralMf::tanh_scaled) is bit for bit tanh_f32 at the same scaled argument.
HODE_DEV float tanh_scaled(float z) {
  return __builtin_fmaf(__builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(z) + 1.0f), -2.0f, 1.0f);
}
HODE_DEV f2 tanh_scaled(f2 z) {
  const f2 e = pair2(__builtin_amdgcn_exp2f(z.x), __builtin_amdgcn_exp2f(z.y)) + splat2(1.0f);
  return vfma(pair2(__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)), splat2(-2.0f), splat2(1.0f));
}
typedef float v4 __attribute__((ext_vector_type(4)));
HODE_DEV v4 tanh_scaled4(const v4& z) {
  const f2 e0 = pair2(__builtin_amdgcn_exp2f(z[0]), __builtin_amdgcn_exp2f(z[1])) + splat2(1.0f);
  const f2 e1 = pair2(__builtin_amdgcn_exp2f(z[2]), __builtin_amdgcn_exp2f(z[3])) + splat2(1.0f);
  const f2 t0 = __builtin_elementwise_fma(pair2(__builtin_amdgcn_rcpf(e0.x), __builtin_amdgcn_rcpf(e0.y)), splat2(-2.0f), splat2(1.0f));
  const f2 t1 = __builtin_elementwise_fma(pair2(__builtin_amdgcn_rcpf(e1.x), __builtin_amdgcn_rcpf(e1.y)), splat2(-2.0f), splat2(1.0f));
  return v4{t0.x, t0.y, t1.x, t1.y};
}
// halves and packed activations of a four-vector (the recurrent decoders, hode_seqdec.hip)
HODE_DEV f2 lo2(const v4& v) { return pair2(v[0], v[1]); }
HODE_DEV f2 hi2(const v4& v) { return pair2(v[2], v[3]); }
HODE_DEV v4 cat4(f2 a, f2 b) { return v4{a.x, a.y, b.x, b.y}; }
HODE_DEV f2 sigmoid2(f2 x) { return vfma(tanh_f32(x * splat2(0.5f)), splat2(0.5f), splat2(0.5f)); }  // 0.5 + 0.5 tanh(x/2)
HODE_DEV v4 sigmoid4(const v4& x) { return cat4(sigmoid2(lo2(x)), sigmoid2(hi2(x))); }
HODE_DEV v4 tanh4(const v4& x) { return cat4(tanh_f32(lo2(x)), tanh_f32(hi2(x))); }
HODE_DEV bool vfinite(float v) { return __builtin_isfinite(v); }
HODE_DEV bool vfinite(f2 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y); }

// division by v_rcp + one Newton step: the first-order errors cancel, bound 0.5 ulp + 9 * 2^-48 relative, measured
// 0.500 ulp, for a, b, 1/b and a/b normal (|a| >= 2^-100, 2^-125 <= |b| <= 2^125, 2^-125 <= |a/b| < 2^127).
// DOMAIN: b finite, nonzero and normal, a finite, a / b below 2^127.  Outside it the Newton step forms 0 * inf or
// inf - inf and the result is NaN where IEEE division gives +-inf or +-0 (b = +-0, +-inf or subnormal, a = +-inf, an
// overflowing quotient); |b| > 2^126 (1/b flushed) gives 0.  Returning q = a * rcp(b) there was measured and not taken: q
// sits on the expert wave's dependent chain and cost the flagship step 3.9 %.  Every call site stays inside the domain
// whenever its own operands are finite (DESIGN.md section 10 lists the 46 sites with their guards):
//   * divisor atol + rtol |y| (scale, tol): the host refuses rtol <= 0 and atol < 0 (check_common, hode_dopri5.hip), so it
//     is positive and finite; it is 0 only for atol = 0 at a zero component, where IEEE division is not finite either;
//   * divisor d1, d0, max(d1, d2), h0, r2, NN r2, NN d1, NN d0: under the selects `d0 < 1e-5f || d1 < 1e-5f`, `!deg0`,
//     `!deg1` (max(d1, d2) > 1e-15), `r2 > 0.0f`, `r2b != 0.0f`, `d1 > 0.0f`, `d0 > 0.0f`, `valid != 0.0f`;
//     h0 is 1e-6 or 0.01 d0 / d1 with d0 >= 1e-5;
//   * divisor dt of an accepted step read from the tape: min(100 h0, h1) times factors in [0.2, 10], positive;
//   * the Hill term irp emax / (ecp + irp): the quotient is at most emax; the divisor is infinite only together with the
//     dividend, and 0 only for ec50 = 0 and ImmuneReact = 0 together -- both NaN under IEEE division too; it is
//     subnormal only for ec50 and ImmuneReact both below 1e-19, outside the parameter's domain (ec50 is a concentration
//     of order 1).
HODE_DEV float div_f32(float a, float b) {
  float r = __builtin_amdgcn_rcpf(b);
  float q = a * r;
  float e = __builtin_fmaf(-b, q, a);
  return __builtin_fmaf(e, r, q);
}

// ---------------------------------------------------------------------------------------------------------
// cross-lane helpers for the "4 lanes per patient" layout: a patient occupies one DPP quad.
// ---------------------------------------------------------------------------------------------------------

// broadcast the value held by lane SRC (0..3) of each quad to all four lanes of the quad (one v_mov_dpp)
template <int SRC>
HODE_DEV float quad_bcast(float v) {
  constexpr int ctrl = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);  // quad_perm:[SRC,SRC,SRC,SRC]
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true));
}

// sum over the four lanes of each quad, result in all four lanes (two DPP adds)
HODE_DEV float quad_sum(float v) {
  // quad_perm:[1,0,3,2] = 0xB1, quad_perm:[2,3,0,1] = 0x4E
  float a = v + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
  return a + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0x4E, 0xf, 0xf, true));
}

// DPP row rotations (a "row" = 16 lanes): plain VALU adds with a DPP operand, no LDS crossbar round trip like __shfl_xor
template <int CTRL>
HODE_DEV float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 4 lanes of a row that share (lane & 3), in every lane of the row   (row_ror:4, row_ror:8).  Each lane adds
// in its own rotated order, so lanes agree only to rounding, not bit for bit: no caller may branch on the value.
HODE_DEV float row_sum_stride4(float v) {
  v += dpp_f32<0x124>(v);
  v += dpp_f32<0x128>(v);
  return v;
}
// sum over the 16 lanes of a row, in every lane of the row   (row_ror:1, 2, 4, 8); as above the lanes agree only to rounding
HODE_DEV float row_sum(float v) {
  v += dpp_f32<0x121>(v);
  v += dpp_f32<0x122>(v);
  v += dpp_f32<0x124>(v);
  v += dpp_f32<0x128>(v);
  return v;
}

// sum across the lanes of a wave that hold the same quad position (xor over lane bits 2..5), result everywhere
HODE_DEV float wave_sum_stride4(float v) {
#pragma unroll
  for (int m = 4; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// full wave sum, the SAME bits in every lane: four DPP row rotations, then the four row sums through SGPRs.  (Six __shfl_xor
// steps are six dependent LDS-crossbar round trips; a dopri5 attempt does two such sums on its critical path,
// DESIGN.md section 5.)
HODE_DEV float wave_sum(float v) {
  v = row_sum(v);
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

HODE_DEV float nextafter_up(float x) {
  // nextafter(x, +inf) for finite x, signed zeros and subnormals included (torchdiffeq Perturb.NEXT,
  // oracle/solvers.py::_nextafter); +inf gives a NaN
  if (x == 0.0f) return __builtin_bit_cast(float, 1u);
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  return __builtin_bit_cast(float, x > 0.0f ? u + 1u : u - 1u);
}
HODE_DEV float nextafter_down(float x) {
  if (x == 0.0f) return __builtin_bit_cast(float, 0x80000001u);
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  return __builtin_bit_cast(float, x > 0.0f ? u - 1u : u + 1u);
}

// fp32 ops that must NOT be contracted into an fma (stage times are compared against dose times with >= / ==,
// so they have to round exactly like the reference's separate mul and add).  HIP's __fmul_rn / __fadd_rn are plain `*` and
// `+`, which the default -ffp-contract=fast fuses after inlining: the contraction is switched off in the bodies instead.
HODE_DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
HODE_DEV float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

}  // namespace hode
