/* C ABI of libhode_probe.so: a TEST-ONLY library that runs the shared device helpers of csrc/hode_common.hpp and
 * csrc/hode_lanes.hpp (and the few helpers of other headers built on them) on their own, one helper per op id, so that the
 * tests can compare each against float64 (tests/test_hip_helpers.py through tests/device_probe.py).  Nothing under hode/
 * loads it.  It is compiled with the flags of the product units, so the helpers see the same -ffp-contract default.
 *
 * Every entry point takes `op id, device pointers, n, stream`, launches one kernel and returns 0, <0 for an argument error
 * (HODE_PROBE_E_*, nothing is launched) or >0 a hipError_t; the message is in hode_probe_last_error_string().
 *
 *   hode_probe_map      y[i] = op(a[i] [, b[i] [, c[i]]]) for i < n.  One element per lane; n must be a multiple of 64 so that
 *                       all 64 lanes of every wave are live.  Pointers an op does not read may be NULL.
 *   hode_probe_wave     y[i] = op(x)[i]: the cross-lane helpers, lane i & 63 of wave i / 64; n a multiple of `block`,
 *                       block 64 or 256.
 *   hode_probe_lanemap  out[3 * thread + {0, 1, 2}] = LaneMap<lpp>(B, ppw).{p, q, live} for every thread of a grid of
 *                       n_blocks blocks of `block` threads.
 *   hode_probe_roundtrip  every thread builds LaneMap<lpp>(B, ppw), load_vec<D>(src + p * D) and
 *                       store_vec<D, lpp>(dst + p * D, ., q, live); the grid is the smallest that covers B patients.
 *                       A lane that must not store (not live; q != 0 when D % 4 != 0) holds poisoned values, so a store
 *                       it should not make shows in dst.
 *                       src and dst are [B][D]; D in {4, 6, 8, 12, 20}. */
#ifndef HODE_PROBE_H_
#define HODE_PROBE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_PROBE_ABI_VERSION 1

#define HODE_PROBE_E_NULL -1         /* a required pointer is NULL */
#define HODE_PROBE_E_SIZE -2         /* n, block, B, ppw or D outside the domain */
#define HODE_PROBE_E_UNSUPPORTED -3  /* unknown op id */

/* hode_probe_map: unary (a) */
#define HODE_PROBE_OP_PRIM_EXP2 0        /* __builtin_amdgcn_exp2f */
#define HODE_PROBE_OP_PRIM_LOG2 1        /* __builtin_amdgcn_logf */
#define HODE_PROBE_OP_PRIM_RCP 2         /* __builtin_amdgcn_rcpf */
#define HODE_PROBE_OP_PRIM_SQRT 3        /* __builtin_sqrtf */
#define HODE_PROBE_OP_EXP 4              /* exp_f32 */
#define HODE_PROBE_OP_LOG 5              /* log_f32 */
#define HODE_PROBE_OP_TANH 6             /* tanh_f32(float) */
#define HODE_PROBE_OP_TANH_PK0 7         /* tanh_f32(f2{a, 0.5 a}).x */
#define HODE_PROBE_OP_TANH_PK1 8         /* tanh_f32(f2{0.5 a, a}).y */
#define HODE_PROBE_OP_TANH_PRECISE 9     /* tanh_precise_f32 */
#define HODE_PROBE_OP_SIGMOID 10         /* sigmoid_f32 */
#define HODE_PROBE_OP_SIGMOID_GATE 11    /* sigmoid_gate (hode_lstm_kernels.hpp) */
#define HODE_PROBE_OP_TANH_SCALED0 12    /* NeuralMf<8>::tanh_scaled, a in slot 0 (the other slots hold 0.5 a) */
#define HODE_PROBE_OP_TANH_SCALED1 13
#define HODE_PROBE_OP_TANH_SCALED2 14
#define HODE_PROBE_OP_TANH_SCALED3 15
#define HODE_PROBE_OP_NEXTAFTER_UP 16
#define HODE_PROBE_OP_NEXTAFTER_DOWN 17
#define HODE_PROBE_OP_TANH_SCALED_F 18   /* tanh_scaled(float) */
#define HODE_PROBE_OP_TANH_SCALED_PK0 19 /* tanh_scaled(f2{a, 0.5 a}).x */
#define HODE_PROBE_OP_TANH_SCALED_PK1 20 /* tanh_scaled(f2{0.5 a, a}).y */
#define HODE_PROBE_OP_TANH_SCALED4_0 21  /* tanh_scaled4, a in slot 0 (the other slots hold 0.5 a) */
#define HODE_PROBE_OP_TANH_SCALED4_1 22
#define HODE_PROBE_OP_TANH_SCALED4_2 23
#define HODE_PROBE_OP_TANH_SCALED4_3 24
#define HODE_PROBE_OP_SIGMOID2_0 25      /* sigmoid2(f2{a, 0.5 a}).x */
#define HODE_PROBE_OP_SIGMOID2_1 26      /* sigmoid2(f2{0.5 a, a}).y */
#define HODE_PROBE_OP_SIGMOID4_0 27      /* sigmoid4, a in slot 0 */
#define HODE_PROBE_OP_SIGMOID4_3 28      /* sigmoid4, a in slot 3 */
#define HODE_PROBE_OP_TANH4_1 29         /* tanh4, a in slot 1 */
#define HODE_PROBE_OP_TANH4_2 30         /* tanh4, a in slot 2 */
#define HODE_PROBE_OP_EXP_FULL 31        /* exp_full_f32 */
/* hode_probe_map: binary (a, b) and ternary (a, b, c) */
#define HODE_PROBE_OP_DIV 32             /* div_f32(a, b) */
#define HODE_PROBE_OP_MUL_ADD_RN 33      /* add_rn(mul_rn(a, b), c) */
#define HODE_PROBE_OP_DPOW_DP 34         /* dpow_dp(a, b, c) (hode_roche.hpp) */
/* hode_probe_wave */
#define HODE_PROBE_OP_QUAD_BCAST0 64
#define HODE_PROBE_OP_QUAD_BCAST1 65
#define HODE_PROBE_OP_QUAD_BCAST2 66
#define HODE_PROBE_OP_QUAD_BCAST3 67
#define HODE_PROBE_OP_QUAD_SUM 68
#define HODE_PROBE_OP_ROW_SUM_STRIDE4 69
#define HODE_PROBE_OP_ROW_SUM 70
#define HODE_PROBE_OP_WAVE_SUM_STRIDE4 71
#define HODE_PROBE_OP_WAVE_SUM 72
#define HODE_PROBE_OP_WAVE_SUM_PATIENTS1 73
#define HODE_PROBE_OP_WAVE_SUM_PATIENTS4 74

int hode_probe_version(void);
const char* hode_probe_last_error_string(void);
int hode_probe_map(int32_t op, const float* a, const float* b, const float* c, float* y, int64_t n, void* hip_stream);
int hode_probe_wave(int32_t op, const float* x, float* y, int64_t n, int32_t block, void* hip_stream);
int hode_probe_lanemap(int32_t lpp, int32_t B, int32_t ppw, int32_t block, int32_t n_blocks, int32_t* out, void* hip_stream);
int hode_probe_roundtrip(int32_t D, int32_t lpp, int32_t B, int32_t ppw, int32_t block, const float* src, float* dst,
                         void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_PROBE_H_ */
