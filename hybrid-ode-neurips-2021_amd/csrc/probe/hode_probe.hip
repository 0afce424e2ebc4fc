// TEST-ONLY probe of the shared device helpers (C ABI include/hode_probe.h, libhode_probe.so): one kernel per group, one
// helper per op id, each called exactly as the product kernels call it.  Nothing here restates a helper: a copy would test
// nothing.  Built with the product flags (build_hip.py TEST_LIBRARIES), loaded only by tests/device_probe.py.
#include <hip/hip_runtime.h>

#include "../../../include/hode_probe.h"
#include "../hode_lanes.hpp"
#include "../hode_lstm_kernels.hpp"
#include "../hode_neural_mf.hpp"
#include "../hode_roche.hpp"
#include "../hode_side_error.hpp"

namespace hode_probe {
namespace {

using namespace hode;

template <int SLOT>
HODE_DEV float tanh_scaled_slot(float v) {
  const float o = 0.5f * v;
  v4 z = {o, o, o, o};
  z[SLOT] = v;
  return NeuralMf<8>::tanh_scaled(z)[SLOT];
}

template <int SLOT, int FN>  // FN 0: tanh_scaled4, 1: sigmoid4, 2: tanh4
HODE_DEV float four_slot(float v) {
  const float o = 0.5f * v;
  v4 z = {o, o, o, o};
  z[SLOT] = v;
  if constexpr (FN == 0) return tanh_scaled4(z)[SLOT];
  else if constexpr (FN == 1) return sigmoid4(z)[SLOT];
  else return tanh4(z)[SLOT];
}

HODE_DEV float map_op(int op, float a, float b, float c) {
  switch (op) {
    case HODE_PROBE_OP_PRIM_EXP2: return __builtin_amdgcn_exp2f(a);
    case HODE_PROBE_OP_PRIM_LOG2: return __builtin_amdgcn_logf(a);
    case HODE_PROBE_OP_PRIM_RCP: return __builtin_amdgcn_rcpf(a);
    case HODE_PROBE_OP_PRIM_SQRT: return __builtin_sqrtf(a);
    case HODE_PROBE_OP_EXP: return exp_f32(a);
    case HODE_PROBE_OP_LOG: return log_f32(a);
    case HODE_PROBE_OP_TANH: return tanh_f32(a);
    case HODE_PROBE_OP_TANH_PK0: return tanh_f32(pair2(a, 0.5f * a)).x;
    case HODE_PROBE_OP_TANH_PK1: return tanh_f32(pair2(0.5f * a, a)).y;
    case HODE_PROBE_OP_TANH_PRECISE: return tanh_precise_f32(a);
    case HODE_PROBE_OP_SIGMOID: return sigmoid_f32(a);
    case HODE_PROBE_OP_SIGMOID_GATE: return sigmoid_gate(a);
    case HODE_PROBE_OP_TANH_SCALED0: return tanh_scaled_slot<0>(a);
    case HODE_PROBE_OP_TANH_SCALED1: return tanh_scaled_slot<1>(a);
    case HODE_PROBE_OP_TANH_SCALED2: return tanh_scaled_slot<2>(a);
    case HODE_PROBE_OP_TANH_SCALED3: return tanh_scaled_slot<3>(a);
    case HODE_PROBE_OP_NEXTAFTER_UP: return nextafter_up(a);
    case HODE_PROBE_OP_NEXTAFTER_DOWN: return nextafter_down(a);
    case HODE_PROBE_OP_TANH_SCALED_F: return tanh_scaled(a);
    case HODE_PROBE_OP_TANH_SCALED_PK0: return tanh_scaled(pair2(a, 0.5f * a)).x;
    case HODE_PROBE_OP_TANH_SCALED_PK1: return tanh_scaled(pair2(0.5f * a, a)).y;
    case HODE_PROBE_OP_TANH_SCALED4_0: return four_slot<0, 0>(a);
    case HODE_PROBE_OP_TANH_SCALED4_1: return four_slot<1, 0>(a);
    case HODE_PROBE_OP_TANH_SCALED4_2: return four_slot<2, 0>(a);
    case HODE_PROBE_OP_TANH_SCALED4_3: return four_slot<3, 0>(a);
    case HODE_PROBE_OP_SIGMOID2_0: return sigmoid2(pair2(a, 0.5f * a)).x;
    case HODE_PROBE_OP_SIGMOID2_1: return sigmoid2(pair2(0.5f * a, a)).y;
    case HODE_PROBE_OP_SIGMOID4_0: return four_slot<0, 1>(a);
    case HODE_PROBE_OP_SIGMOID4_3: return four_slot<3, 1>(a);
    case HODE_PROBE_OP_TANH4_1: return four_slot<1, 2>(a);
    case HODE_PROBE_OP_TANH4_2: return four_slot<2, 2>(a);
    case HODE_PROBE_OP_EXP_FULL: return exp_full_f32(a);
    case HODE_PROBE_OP_DIV: return div_f32(a, b);
    case HODE_PROBE_OP_MUL_ADD_RN: return add_rn(mul_rn(a, b), c);
    default: return dpow_dp(a, b, c);  // HODE_PROBE_OP_DPOW_DP
  }
}

// n is a multiple of 64 and of the block size (the host checks it): every lane is live
__global__ __launch_bounds__(256) void map_kernel(int op, const float* __restrict__ a, const float* __restrict__ b,
                                                  const float* __restrict__ c, float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  y[i] = map_op(op, a[i], b ? b[i] : 0.0f, c ? c[i] : 0.0f);
}

__global__ __launch_bounds__(256) void wave_kernel(int op, const float* __restrict__ x, float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float v = x[i];
  float r;
  switch (op) {  // op is uniform: every lane of the wave takes the same arm
    case HODE_PROBE_OP_QUAD_BCAST0: r = quad_bcast<0>(v); break;
    case HODE_PROBE_OP_QUAD_BCAST1: r = quad_bcast<1>(v); break;
    case HODE_PROBE_OP_QUAD_BCAST2: r = quad_bcast<2>(v); break;
    case HODE_PROBE_OP_QUAD_BCAST3: r = quad_bcast<3>(v); break;
    case HODE_PROBE_OP_QUAD_SUM: r = quad_sum(v); break;
    case HODE_PROBE_OP_ROW_SUM_STRIDE4: r = row_sum_stride4(v); break;
    case HODE_PROBE_OP_ROW_SUM: r = row_sum(v); break;
    case HODE_PROBE_OP_WAVE_SUM_STRIDE4: r = wave_sum_stride4(v); break;
    case HODE_PROBE_OP_WAVE_SUM: r = wave_sum(v); break;
    case HODE_PROBE_OP_WAVE_SUM_PATIENTS1: r = wave_sum_patients<1>(v); break;
    default: r = wave_sum_patients<4>(v); break;  // HODE_PROBE_OP_WAVE_SUM_PATIENTS4
  }
  y[i] = r;
}

template <int LPP>
__global__ __launch_bounds__(256) void lanemap_kernel(int B, int ppw, int* __restrict__ out) {
  const LaneMap<LPP> m(B, ppw);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[3 * i] = m.p;
  out[3 * i + 1] = m.q;
  out[3 * i + 2] = m.live ? 1 : 0;
}

// LaneMap keeps p inside [0, B) for every lane, so both rows are inside [B][D]
template <int D, int LPP>
__global__ __launch_bounds__(256) void roundtrip_kernel(int B, int ppw, const float* __restrict__ src, float* __restrict__ dst) {
  const LaneMap<LPP> m(B, ppw);
  float v[D];
  load_vec<D>(src + (size_t)m.p * D, v);
  // a lane that must not store holds values no source row has: a store from it shows in dst
  if (!m.live || (D % 4 != 0 && m.q != 0)) {
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = -(float)(1000 + (threadIdx.x & 63));
  }
  store_vec<D, LPP>(dst + (size_t)m.p * D, v, m.q, m.live);
}

template <int D>
int launch_roundtrip(int lpp, dim3 grid, dim3 block, hipStream_t s, int B, int ppw, const float* src, float* dst) {
  if (lpp == 1) hipLaunchKernelGGL((roundtrip_kernel<D, 1>), grid, block, 0, s, B, ppw, src, dst);
  else hipLaunchKernelGGL((roundtrip_kernel<D, 4>), grid, block, 0, s, B, ppw, src, dst);
  return hode_side::launch_fail(hipGetLastError(), "hode_probe_roundtrip");
}

bool geometry_ok(int lpp, int B, int ppw, int block) {
  return (lpp == 1 || lpp == 4) && B >= 1 && B <= (1 << 24) && ppw >= 1 && ppw <= 64 / lpp && (block == 64 || block == 256);
}

}  // namespace
}  // namespace hode_probe


extern "C" {

int hode_probe_version(void) { return HODE_PROBE_ABI_VERSION; }
const char* hode_probe_last_error_string(void) { return hode_side::g_err; }

int hode_probe_map(int32_t op, const float* a, const float* b, const float* c, float* y, int64_t n, void* hip_stream) {
  const bool unary = op >= HODE_PROBE_OP_PRIM_EXP2 && op <= HODE_PROBE_OP_EXP_FULL;
  const bool binary = op == HODE_PROBE_OP_DIV, ternary = op == HODE_PROBE_OP_MUL_ADD_RN || op == HODE_PROBE_OP_DPOW_DP;
  if (!unary && !binary && !ternary) return hode_side::fail(HODE_PROBE_E_UNSUPPORTED, "hode_probe_map: unknown op %d", op);
  if (!a || !y || (!unary && !b) || (ternary && !c)) return hode_side::fail(HODE_PROBE_E_NULL, "hode_probe_map: op %d: NULL operand", op);
  if (n < 0 || n % 64 != 0 || n > ((int64_t)1 << 30)) return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_map: n = %lld is not a multiple of 64 in [0, 2^30]", (long long)n);
  if (n == 0) return 0;
  const int block = n % 256 == 0 ? 256 : 64;
  hipLaunchKernelGGL(hode_probe::map_kernel, dim3((unsigned)(n / block)), dim3(block), 0, (hipStream_t)hip_stream, (int)op, a,
                     unary ? nullptr : b, ternary ? c : nullptr, y);
  return hode_side::launch_fail(hipGetLastError(), "hode_probe_map");
}

int hode_probe_wave(int32_t op, const float* x, float* y, int64_t n, int32_t block, void* hip_stream) {
  if (op < HODE_PROBE_OP_QUAD_BCAST0 || op > HODE_PROBE_OP_WAVE_SUM_PATIENTS4) return hode_side::fail(HODE_PROBE_E_UNSUPPORTED, "hode_probe_wave: unknown op %d", op);
  if (!x || !y) return hode_side::fail(HODE_PROBE_E_NULL, "hode_probe_wave: NULL operand");
  if ((block != 64 && block != 256) || n < 0 || n % block != 0 || n > ((int64_t)1 << 30)) return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_wave: n = %lld, block = %d", (long long)n, block);
  if (n == 0) return 0;
  hipLaunchKernelGGL(hode_probe::wave_kernel, dim3((unsigned)(n / block)), dim3(block), 0, (hipStream_t)hip_stream, (int)op, x, y);
  return hode_side::launch_fail(hipGetLastError(), "hode_probe_wave");
}

int hode_probe_lanemap(int32_t lpp, int32_t B, int32_t ppw, int32_t block, int32_t n_blocks, int32_t* out, void* hip_stream) {
  if (!out) return hode_side::fail(HODE_PROBE_E_NULL, "hode_probe_lanemap: NULL out");
  if (!hode_probe::geometry_ok(lpp, B, ppw, block) || n_blocks < 1 || n_blocks > (1 << 20)) return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_lanemap: lpp = %d, B = %d, ppw = %d, block = %d, n_blocks = %d", lpp, B, ppw, block, n_blocks);
  if (lpp == 1) hipLaunchKernelGGL(hode_probe::lanemap_kernel<1>, dim3(n_blocks), dim3(block), 0, (hipStream_t)hip_stream, B, ppw, out);
  else hipLaunchKernelGGL(hode_probe::lanemap_kernel<4>, dim3(n_blocks), dim3(block), 0, (hipStream_t)hip_stream, B, ppw, out);
  return hode_side::launch_fail(hipGetLastError(), "hode_probe_lanemap");
}

int hode_probe_roundtrip(int32_t D, int32_t lpp, int32_t B, int32_t ppw, int32_t block, const float* src, float* dst,
                         void* hip_stream) {
  if (!src || !dst) return hode_side::fail(HODE_PROBE_E_NULL, "hode_probe_roundtrip: NULL operand");
  if (!hode_probe::geometry_ok(lpp, B, ppw, block)) return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_roundtrip: lpp = %d, B = %d, ppw = %d, block = %d", lpp, B, ppw, block);
  if (D % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15)) return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_roundtrip: rows of D = %d need 16-byte aligned buffers", D);
  const int waves = (B + ppw - 1) / ppw, wpb = block / 64;
  const dim3 grid((waves + wpb - 1) / wpb), blk(block);
  hipStream_t s = (hipStream_t)hip_stream;
  switch (D) {
    case 4: return hode_probe::launch_roundtrip<4>(lpp, grid, blk, s, B, ppw, src, dst);
    case 6: return hode_probe::launch_roundtrip<6>(lpp, grid, blk, s, B, ppw, src, dst);
    case 8: return hode_probe::launch_roundtrip<8>(lpp, grid, blk, s, B, ppw, src, dst);
    case 12: return hode_probe::launch_roundtrip<12>(lpp, grid, blk, s, B, ppw, src, dst);
    case 20: return hode_probe::launch_roundtrip<20>(lpp, grid, blk, s, B, ppw, src, dst);
  }
  return hode_side::fail(HODE_PROBE_E_SIZE, "hode_probe_roundtrip: D = %d is not one of 4, 6, 8, 12, 20", D);
}

}  // extern "C"
