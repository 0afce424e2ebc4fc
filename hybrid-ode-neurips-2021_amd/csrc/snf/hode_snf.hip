// The Sylvester-flow posterior (LHM-SNF): K Sylvester flows over S draws per patient from the encoder's raw heads, with
// the exp(z - 5) output layer and the Monte-Carlo KL against the Exponential(100) prior, forward and backward, one launch
// each, gfx950 (libhode_snf.so, C ABI include/hode_snf.h).
//
// Layout: that of csrc/sylvester/hode_sylvester.hip.  A workgroup holds `ppb` patients of L lanes each (L a power of two,
// T <= L <= 64); the L lanes of a patient take the draws s = slot, slot + L, ...  The flows are streamed: per flow a
// prologue forms the patient's A, C, b and the diagonal products once, into LDS, zero-padded to the tile T >= D, straight
// from the raw head rows: r1 = U full_d + diag(tanh diag1), r2 = U full_d^T + diag(tanh diag2) are read off full_d entry
// by entry and never exist in memory.  In Householder mode Q is built in LDS, a lane per row, by H rank-1 updates of the
// identity, and A = Q r2^T, C = Q r1; in triangular mode A and C are rows of r2 and r1 picked by the identity (even flows)
// or the flip (odd flows).  Between flows a draw's state lives in the caller's workspace: slabs z_0 .. z_K (the tape, the
// forward writes it) and one slab for the backward's running cotangent.  A lane only ever re-reads rows it wrote itself.
//
// Sums over the draws of a patient (the KL, the outer products zbar h^T and z abar^T, the base gradients) run in a fixed
// order: a lane walks its draws in order, stages its vectors in LDS, and one owner lane per entry adds the L staged draws
// in lane order.  No float atomics: repeated calls are bit-identical.  The backward epilogue of a flow carries the chain
// rule to the raw heads: g_full_d = U g_r1 + (U g_r2)^T, the diagonals through 1 - tanh^2, and v by a reverse sweep over
// the reflections that needs no tape, because Q_{h-1} = Q_h H_h.
#include <hip/hip_runtime.h>

#include "../../../include/hode_snf.h"
#include "../hode_common.hpp"
#include "../hode_side_error.hpp"

namespace hode_snf {

using hode::exp_full_f32;
using hode::log_f32;
using hode::tanh_precise_f32;
using hode_side::fail;
using hode_side::launch_fail;

constexpr int kBlock = 256;
constexpr int kLdsLimit = 64 * 1024;
constexpr int kStage = 5;  // staged vectors per lane in the backward: zbar | h | z | abar | diagonal term
constexpr int kMaxH = HODE_SNF_MAX_HOUSEHOLDER;
constexpr float kLogSqrt2Pi = 0.9189385332046727f;
constexpr float kLogRate = 4.605170185988092f;  // log 100
constexpr float kRate = 100.0f;

struct SnfArgs {
  const float* __restrict__ mu;
  const float* __restrict__ log_var;
  const float* __restrict__ full_d;
  const float* __restrict__ diag1;
  const float* __restrict__ diag2;
  const float* __restrict__ bias;
  const float* __restrict__ v;
  const float* __restrict__ noise;
  float* z_out;
  float* kl;
  float* ws;  // [K + 2][S][B][D]: z_0 .. z_K, then the backward's running cotangent
  const float* gz;
  const float* gkl;
  float* g_mu;
  float* g_lv;
  float* g_fd;
  float* g_d1;
  float* g_d2;
  float* g_bias;
  float* g_v;
  int B, D, K, S, H, s_kl, L, ppb;
};

// LDS per patient, one flow at a time: [A (T x T) | C (T x T) | b (T) | r1_mm r2_mm (T) | tanh diag1 (T) | tanh diag2 (T)];
// the backward's accumulators [sum z abar^T | sum zbar h^T | sum abar | sum diagonal term | base sums (2 T)] have the same
// shape
template <int T>
constexpr int kPrm = 2 * T * T + 4 * T;
// [mu (T) | sigma (T) | sum_d (-log sigma - log sqrt(2 pi)), padded to 4]
template <int T>
constexpr int kBase = 2 * T + 4;
// Householder mode only: [Q (T x T) | vh (kMaxH x T) | 1 / |v| (kMaxH)]
template <int T>
constexpr int kOrtho = T * T + kMaxH * T + kMaxH;

template <int T>
constexpr int kUnroll = T >= 32 ? 2 : 4;

// tanh(x) and 1 - tanh(x)^2 from one exponential, so that the derivative of a saturated diagonal is tiny, not zero
__device__ __forceinline__ void tanh_sech2(float x, float* t, float* s2) {
  const float e = expf(-2.0f * fabsf(x));
  const float r = 1.0f / (1.0f + e);
  const float m = (1.0f - e) * r;
  *t = x < 0.f ? -m : m;
  *s2 = 4.0f * e * r * r;
}

__device__ __forceinline__ float group_sum(float v, int L) {
  for (int off = L >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// A, C, b and the diagonal products of patient `bb`, flow `k`, zero outside D x D.  Every lane of the workgroup calls
// this (the barriers involve all of them); `active` says whether the lane's patient exists.
template <int T>
__device__ __forceinline__ void flow_setup(const SnfArgs& a, bool active, int bb, int k, int slot, float* prm, float* ort) {
  const int D = a.D, H = a.H, L = a.L;
  const size_t pk = (size_t)(active ? bb : 0) * a.K + k;
  float* t1 = prm + 2 * T * T + 2 * T;
  float* t2 = t1 + T;
  float* Q = ort;
  float* vh = ort + T * T;
  float* vinv = vh + kMaxH * T;
  if (active) {
    for (int m = slot; m < T; m += L) {
      float x1 = 0.f, x2 = 0.f, s;
      if (m < D) {
        tanh_sech2(a.diag1[pk * D + m], &x1, &s);
        tanh_sech2(a.diag2[pk * D + m], &x2, &s);
      }
      t1[m] = x1;
      t2[m] = x2;
      prm[2 * T * T + m] = m < D ? a.bias[pk * D + m] : 0.f;
      prm[2 * T * T + T + m] = x1 * x2;
    }
    // vh = v / |v|, scaled by max|v| first so that neither a tiny nor a huge v leaves float32 when squared
    for (int h = slot; h < H; h += L) {
      const float* vr = a.v + (pk * H + h) * D;
      float big = 0.f;
      for (int d = 0; d < D; ++d) big = fmaxf(big, fabsf(vr[d]));
      const float rb = 1.0f / big;
      float n2 = 0.f;
      for (int d = 0; d < D; ++d) {
        const float w = vr[d] * rb;
        n2 = __builtin_fmaf(w, w, n2);
      }
      const float rn = 1.0f / sqrtf(n2);
      for (int d = 0; d < T; ++d) vh[h * T + d] = d < D ? vr[d] * rb * rn : 0.f;
      vinv[h] = rb * rn;
    }
  }
  __syncthreads();
  if (H) {
    if (active) {
      for (int d = slot; d < D; d += L) {
        float* row = Q + d * T;
        for (int j = 0; j < T; ++j) row[j] = j == d ? 1.0f : 0.f;
        for (int h = 0; h < H; ++h) {
          const float* w = vh + h * T;
          float dot = 0.f;
          for (int j = 0; j < D; ++j) dot = __builtin_fmaf(row[j], w[j], dot);
          dot *= -2.0f;
          for (int j = 0; j < D; ++j) row[j] = __builtin_fmaf(dot, w[j], row[j]);
        }
      }
    }
    __syncthreads();
  }
  if (active) {
    const float* fd = a.full_d + pk * D * D;
    const bool flip = k & 1;
    for (int idx = slot; idx < T * T; idx += L) {
      const int d = idx / T, m = idx % T;
      float av = 0.f, cv = 0.f;
      if (d < D && m < D) {
        if (H) {
          const float* row = Q + d * T;
#pragma unroll 4
          for (int j = 0; j < D; ++j) {
            const float t = row[j] * fd[j * D + m];
            if (j < m) cv += t;  // r1[j][m] = full_d[j][m] above the diagonal
            if (j > m) av += t;  // r2[m][j] = full_d[j][m] above the diagonal
          }
          av = __builtin_fmaf(row[m], t2[m], av);
          cv = __builtin_fmaf(row[m], t1[m], cv);
        } else {
          const int pd = flip ? D - 1 - d : d;
          av = m < pd ? fd[pd * D + m] : m == pd ? t2[m] : 0.f;  // r2[m][p[d]]
          cv = pd < m ? fd[pd * D + m] : m == pd ? t1[m] : 0.f;  // r1[p[d]][m]
        }
      }
      prm[idx] = av;
      prm[T * T + idx] = cv;
    }
  }
  __syncthreads();
}

// mu, sigma and the constant of the base density of patient `bb`
template <int T>
__device__ __forceinline__ void base_setup(const SnfArgs& a, int bb, int slot, float* base) {
  for (int d = slot; d < T; d += a.L) {
    const bool in = d < a.D;
    base[d] = in ? a.mu[(size_t)bb * a.D + d] : 0.f;
    base[T + d] = in ? exp_full_f32(0.5f * a.log_var[(size_t)bb * a.D + d]) : 0.f;
  }
  if (slot == 0) {
    float c = 0.f;
    for (int d = 0; d < a.D; ++d) c -= 0.5f * a.log_var[(size_t)bb * a.D + d] + kLogSqrt2Pi;
    base[2 * T] = c;
  }
}

// h = tanh(z A + b), zero past D; z[d] is read through `zrow` (global or LDS)
template <int T>
__device__ __forceinline__ void flow_act(const SnfArgs& a, const float* prm, const float* zrow, float (&h)[T]) {
#pragma unroll
  for (int m = 0; m < T; ++m) h[m] = prm[2 * T * T + m];
#pragma unroll kUnroll<T>
  for (int d = 0; d < a.D; ++d) {
    const float zd = zrow[d];
#pragma unroll
    for (int m = 0; m < T; ++m) h[m] = __builtin_fmaf(zd, prm[d * T + m], h[m]);
  }
#pragma unroll
  for (int m = 0; m < T; ++m) h[m] = m < a.D ? tanh_precise_f32(h[m]) : 0.f;
}

template <int T>
__global__ __launch_bounds__(kBlock) void snf_fwd_kernel(SnfArgs a) {
  extern __shared__ float lds[];
  const int L = a.L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * a.ppb + pl;
  const bool active = bb < a.B;
  float* prm = lds + (size_t)pl * (kPrm<T> + kBase<T> + (a.H ? kOrtho<T> : 0));
  float* base = prm + kPrm<T>;
  float* ort = base + kBase<T>;
  const size_t sbd = (size_t)a.S * a.B * a.D;
  if (active) base_setup<T>(a, bb, slot, base);
  float kl_sum = 0.f;
  for (int k = 0; k < a.K; ++k) {
    if (k) __syncthreads();  // every lane is done with the previous flow's constants
    flow_setup<T>(a, active, bb, k, slot, prm, ort);
    if (!active) continue;
    float* src = a.ws + (size_t)k * sbd;
    float* dst = src + sbd;
    const bool last = k == a.K - 1;
    for (int s = slot; s < a.S; s += L) {
      const size_t row = ((size_t)s * a.B + bb) * a.D;
      const bool in_kl = s >= a.s_kl;
      if (k == 0) {  // z_0 = eps sigma + mu; log N(z_0; mu, sigma) = const - |eps|^2 / 2
        float q2 = 0.f;
        for (int d = 0; d < a.D; ++d) {
          const float e = a.noise[row + d];
          src[row + d] = __builtin_fmaf(e, base[T + d], base[d]);
          q2 = __builtin_fmaf(e, e, q2);
        }
        if (in_kl) kl_sum += __builtin_fmaf(-0.5f, q2, base[2 * T]);
      }
      float h[T];
      flow_act<T>(a, prm, src + row, h);
      float tail = 0.f;  // the output layer's share of logdet + log p
#pragma unroll kUnroll<T>
      for (int d = 0; d < a.D; ++d) {
        float v = src[row + d];
#pragma unroll
        for (int m = 0; m < T; ++m) v = __builtin_fmaf(h[m], prm[T * T + d * T + m], v);
        dst[row + d] = v;
        if (last) {
          const float y = v - 5.0f;
          const float zo = exp_full_f32(y);
          tail += y + (kLogRate - kRate * zo);
          if (a.z_out) a.z_out[row + d] = zo;
        }
      }
      float ld = 0.f;
#pragma unroll
      for (int m = 0; m < T; ++m)
        if (m < a.D) ld += log_f32(fabsf(__builtin_fmaf(__builtin_fmaf(-h[m], h[m], 1.0f), prm[2 * T * T + T + m], 1.0f)));
      if (in_kl) kl_sum -= ld + tail;
    }
  }
  if (active) {
    kl_sum = group_sum(kl_sum, L);
    if (slot == 0) a.kl[bb] = kl_sum / (float)(a.S - a.s_kl);
  }
}

// the chain rule from the accumulators of patient `bb`, flow `k`, to the raw heads; in Householder mode dL/dQ goes to
// `gq` (T x T) for the sweep.  r1 and r2 are read off full_d and the staged tanh values.
template <int T>
__device__ __forceinline__ void flow_epilogue(const SnfArgs& a, int bb, int k, int slot, const float* prm, const float* acc,
                                              const float* Q, float* gq) {
  const int D = a.D, H = a.H, L = a.L;
  const size_t pk = (size_t)bb * a.K + k;
  const float* fd = a.full_d + pk * D * D;
  const float* t1 = prm + 2 * T * T + 2 * T;
  const float* t2 = t1 + T;
  const float* acc_a = acc;
  const float* acc_c = acc + T * T;
  const float* acc_b = acc + 2 * T * T;
  const float* acc_dd = acc_b + T;
  const bool flip = k & 1;
  float* gfd = a.g_fd + pk * D * D;
  for (int idx = slot; idx < D * D; idx += L) {
    const int i = idx / D, j = idx % D;
    // above the diagonal full_d[i][j] is r1[i][j], whose gradient is (Q^T g_C)[i][j]; below it is r2[j][i], whose
    // gradient is (g_A^T Q)[j][i]; on the diagonal both, for the tanh heads
    float gc = 0.f, ga = 0.f;
    if (H) {
#pragma unroll 4
      for (int d = 0; d < D; ++d) {
        const float qv = Q[d * T + i];
        gc = __builtin_fmaf(qv, acc_c[d * T + j], gc);
        ga = __builtin_fmaf(qv, acc_a[d * T + j], ga);
      }
    } else {
      const int pi = flip ? D - 1 - i : i;
      gc = acc_c[pi * T + j];
      ga = acc_a[pi * T + j];
    }
    if (i == j) {
      float x, s1, s2;
      tanh_sech2(a.diag1[pk * D + i], &x, &s1);
      tanh_sech2(a.diag2[pk * D + i], &x, &s2);
      a.g_d1[pk * D + i] = __builtin_fmaf(acc_dd[i], t2[i], gc) * s1;
      a.g_d2[pk * D + i] = __builtin_fmaf(acc_dd[i], t1[i], ga) * s2;
      gfd[idx] = 0.f;
    } else {
      gfd[idx] = i < j ? gc : ga;
    }
  }
  for (int m = slot; m < D; m += L) a.g_bias[pk * D + m] = acc_b[m];
  if (H) {
    // dL/dQ[d][j] = sum_m g_A[d][m] r2[m][j] + g_C[d][m] r1[j][m]
    for (int idx = slot; idx < D * D; idx += L) {
      const int d = idx / D, j = idx % D;
      float g = __builtin_fmaf(acc_a[d * T + j], t2[j], acc_c[d * T + j] * t1[j]);
#pragma unroll 4
      for (int m = 0; m < D; ++m) {
        const float f = fd[j * D + m];
        if (m < j) g = __builtin_fmaf(acc_a[d * T + m], f, g);
        if (m > j) g = __builtin_fmaf(acc_c[d * T + m], f, g);
      }
      gq[d * T + j] = g;
    }
  }
}

// dL/dv of patient `bb`, flow `k`, from dL/dQ in `gq`, the last reflection first: with P = Q_{h-1} = Q_h H_h,
// dL/dvh = -2 (P^T (G vh) + G^T (P vh)) and dL/dQ_{h-1} = G H_h.  Every lane of the workgroup calls this.  Q is consumed.
template <int T>
__device__ __forceinline__ void householder_sweep(const SnfArgs& a, bool active, int bb, int k, int slot, float* ort, float* gq) {
  const int D = a.D, H = a.H, L = a.L;
  float* Q = ort;
  const float* vh = ort + T * T;
  const float* vinv = vh + kMaxH * T;
  float* pv = gq + T * T;  // P vh
  float* gv = pv + T;      // G vh
  float* gw = gv + T;      // dL/dvh
  for (int h = H - 1; h >= 0; --h) {
    const float* w = vh + h * T;
    if (active) {
      for (int d = slot; d < D; d += L) {
        float* row = Q + d * T;
        const float* grow = gq + d * T;
        float dot = 0.f, c = 0.f;
        for (int j = 0; j < D; ++j) {
          dot = __builtin_fmaf(row[j], w[j], dot);
          c = __builtin_fmaf(grow[j], w[j], c);
        }
        dot *= -2.0f;
        float p = 0.f;
        for (int j = 0; j < D; ++j) {
          row[j] = __builtin_fmaf(dot, w[j], row[j]);
          p = __builtin_fmaf(row[j], w[j], p);
        }
        pv[d] = p;
        gv[d] = c;
      }
    }
    __syncthreads();
    if (active) {
      for (int j = slot; j < D; j += L) {
        float g = 0.f;
        for (int d = 0; d < D; ++d) {
          g = __builtin_fmaf(Q[d * T + j], gv[d], g);
          g = __builtin_fmaf(gq[d * T + j], pv[d], g);
        }
        gw[j] = -2.0f * g;
      }
    }
    __syncthreads();
    if (active) {
      for (int d = slot; d < D; d += L) {
        float* grow = gq + d * T;
        const float c = -2.0f * gv[d];
        for (int j = 0; j < D; ++j) grow[j] = __builtin_fmaf(c, w[j], grow[j]);
      }
      // vh = v / |v|: dL/dv = (dL/dvh - (dL/dvh . vh) vh) / |v|
      float dot = 0.f;
      for (int j = 0; j < D; ++j) dot = __builtin_fmaf(gw[j], w[j], dot);
      float* out = a.g_v + (((size_t)bb * a.K + k) * H + h) * D;
      for (int j = slot; j < D; j += L) out[j] = __builtin_fmaf(-dot, w[j], gw[j]) * vinv[h];
    }
    // the next round's first phase writes only what its own lane reads here (rows of Q and gq, pv[d], gv[d]); gw is
    // rewritten after that round's first barrier
  }
}

template <int T>
__global__ __launch_bounds__(kBlock) void snf_bwd_kernel(SnfArgs a) {
  extern __shared__ float lds[];
  const int L = a.L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * a.ppb + pl;
  const bool active = bb < a.B;
  const int n_ort = a.H ? kOrtho<T> : 0;
  float* prm = lds + (size_t)pl * (2 * kPrm<T> + kBase<T> + n_ort + L * kStage * T);
  float* base = prm + kPrm<T>;
  float* ort = base + kBase<T>;
  float* acc = ort + n_ort;
  float* stg = acc + kPrm<T>;
  float* mine = stg + slot * kStage * T;
  const size_t sbd = (size_t)a.S * a.B * a.D;
  float* zb = a.ws + (size_t)(a.K + 1) * sbd;  // the running cotangent of z
  const int n_it = (a.S + L - 1) / L;  // the same in every lane: the barriers below involve the whole workgroup
  const float n_kl = (float)(a.S - a.s_kl);
  const float ckl = (a.gkl && active) ? a.gkl[bb] / n_kl : 0.f;
  if (active) {
    base_setup<T>(a, bb, slot, base);
    // z_out = exp(z_K - 5): d/dz_K = z_out (G_z + 100 c); logdet's sum_d (z_K - 5): -c
    const float* zk = a.ws + (size_t)a.K * sbd;
    for (int s = slot; s < a.S; s += L) {
      const size_t row = ((size_t)s * a.B + bb) * a.D;
      const float c = s >= a.s_kl ? ckl : 0.f;
      for (int d = 0; d < a.D; ++d) {
        const float gz = a.gz ? a.gz[row + d] : 0.f;
        zb[row + d] = __builtin_fmaf(exp_full_f32(zk[row + d] - 5.0f), __builtin_fmaf(kRate, c, gz), -c);
      }
    }
  }
  for (int k = a.K - 1; k >= 0; --k) {
    __syncthreads();  // the previous flow's epilogue is done with the constants and the accumulators
    if (active)
      for (int i = slot; i < kPrm<T>; i += L) acc[i] = 0.f;
    flow_setup<T>(a, active, bb, k, slot, prm, ort);
    const float* src = a.ws + (size_t)k * sbd;
    for (int it = 0; it < n_it; ++it) {
      const int s = it * L + slot;
      const bool valid = active && s < a.S;
      const size_t row = valid ? ((size_t)s * a.B + bb) * a.D : 0;
      float h[T], hb[T];
      for (int d = 0; d < T; ++d) {
        mine[d] = valid && d < a.D ? zb[row + d] : 0.f;
        mine[2 * T + d] = valid && d < a.D ? src[row + d] : 0.f;
      }
      flow_act<T>(a, prm, mine + 2 * T, h);
#pragma unroll
      for (int m = 0; m < T; ++m) hb[m] = 0.f;
#pragma unroll kUnroll<T>
      for (int d = 0; d < a.D; ++d) {
        const float zbd = mine[d];
#pragma unroll
        for (int m = 0; m < T; ++m) hb[m] = __builtin_fmaf(zbd, prm[T * T + d * T + m], hb[m]);
      }
      const float g = valid && s >= a.s_kl ? -ckl : 0.f;  // d loss / d logdet of this draw
#pragma unroll
      for (int m = 0; m < T; ++m) {
        const bool live = valid && m < a.D;
        const float one_m = __builtin_fmaf(-h[m], h[m], 1.0f);
        const float dd = prm[2 * T * T + T + m];
        const float rg = __builtin_amdgcn_rcpf(__builtin_fmaf(one_m, dd, 1.0f));
        const float hbar = __builtin_fmaf(-2.0f * g * h[m], dd * rg, hb[m]);  // + g d log|1 + (1 - h^2) dd| / dh
        hb[m] = live ? hbar * one_m : 0.f;                                    // abar
        mine[T + m] = h[m];
        mine[3 * T + m] = hb[m];
        mine[4 * T + m] = live ? g * one_m * rg : 0.f;                        // g d log|.| / d dd
      }
#pragma unroll kUnroll<T>
      for (int d = 0; d < a.D; ++d) {
        float v = mine[d];
#pragma unroll
        for (int m = 0; m < T; ++m) v = __builtin_fmaf(prm[d * T + m], hb[m], v);
        if (valid) zb[row + d] = v;
      }
      __syncthreads();
      if (active) {
        for (int idx = slot; idx < T * T; idx += L) {
          const int d = idx / T, m = idx % T;
          if (d < a.D && m < a.D) {
            float sa = 0.f, sc = 0.f;
#pragma unroll 4
            for (int l = 0; l < L; ++l) {
              const float* p = stg + l * kStage * T;
              sc = __builtin_fmaf(p[d], p[T + m], sc);
              sa = __builtin_fmaf(p[2 * T + d], p[3 * T + m], sa);
            }
            acc[idx] += sa;
            acc[T * T + idx] += sc;
          }
        }
        for (int m = slot; m < a.D; m += L) {
          float sb_ = 0.f, sd = 0.f;
#pragma unroll 4
          for (int l = 0; l < L; ++l) {
            const float* p = stg + l * kStage * T;
            sb_ += p[3 * T + m];
            sd += p[4 * T + m];
          }
          acc[2 * T * T + m] += sb_;
          acc[2 * T * T + T + m] += sd;
        }
      }
      __syncthreads();
    }
    // the staging slots are free now: dL/dQ and the sweep's vectors live there (T T + 3 T <= kStage T L floats, L >= T)
    if (active) flow_epilogue<T>(a, bb, k, slot, prm, acc, ort, stg);
    if (a.H) {
      __syncthreads();
      householder_sweep<T>(a, active, bb, k, slot, ort, stg);
    }
  }
  // z_0 = eps sigma + mu: grad_mu = sum_s zbar_0, grad_log_var = sigma / 2 sum_s zbar_0 eps; the base density adds -1/2
  // per unit of d loss / d kl_s.  Each lane stages its draw's zbar_0 and eps; lane d of the patient owns entry d.
  float gm = 0.f, ge = 0.f;
  for (int it = 0; it < n_it; ++it) {
    const int s = it * L + slot;
    const bool valid = active && s < a.S;
    const size_t row = valid ? ((size_t)s * a.B + bb) * a.D : 0;
    __syncthreads();  // the owners are done with the previous round (and with the last flow's epilogue)
    for (int d = 0; d < T; ++d) {
      mine[d] = valid && d < a.D ? zb[row + d] : 0.f;
      mine[T + d] = valid && d < a.D ? a.noise[row + d] : 0.f;
    }
    __syncthreads();
    if (active && slot < a.D) {
#pragma unroll 4
      for (int l = 0; l < L; ++l) {
        const float* p = stg + l * kStage * T;
        gm += p[slot];
        ge = __builtin_fmaf(p[slot], p[T + slot], ge);
      }
    }
  }
  if (active && slot < a.D) {
    a.g_mu[(size_t)bb * a.D + slot] = gm;
    a.g_lv[(size_t)bb * a.D + slot] = __builtin_fmaf(0.5f * base[T + slot], ge, -0.5f * ckl * n_kl);
  }
}

static int tile_of(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }

static size_t lds_per_patient(int T, int L, int H, bool bwd) {
  const size_t prm = 2 * (size_t)T * T + 4 * (size_t)T;
  const size_t fixed = prm + 2 * (size_t)T + 4 + (H ? (size_t)T * T + (size_t)kMaxH * T + kMaxH : 0);
  return sizeof(float) * (bwd ? fixed + prm + (size_t)L * kStage * T : fixed);
}

// lanes per patient and patients per workgroup, as in hode_sylvester.hip: enough lanes in flight at small B, no more than
// the draws but at least T (a lane per row of the tile in the prologue, the epilogue and the base sums), whole waves where
// a workgroup has 64 lanes, LDS within the limit
static void geometry(int B, int S, int T, int H, bool bwd, int* lanes, int* patients) {
  int L = 1;
  while (L < 64 && (long long)B * L < 131072) L <<= 1;
  int sp = 1;
  while (sp < S) sp <<= 1;
  if (L > sp) L = sp;
  if (L < T) L = T;
  if (L > 64) L = 64;
  int p = kBlock / L;
  const int cap = (int)(kLdsLimit / lds_per_patient(T, L, H, bwd));  // >= 1: T = 32, L = 64, H > 0 needs 63 792 B in the backward
  if (p > cap) p = cap;
  if (p * L >= 64) p -= p % (64 / L);
  if (p > B) p = B;
  *lanes = L;
  *patients = p;
}

static size_t ws_bytes(const hode_snf_desc* d) {
  const size_t n = (size_t)(d->n_flows + 2) * d->n_samples * d->batch * d->latent_dim * sizeof(float);
  return (n + 255) / 256 * 256;
}

static bool sizes_ok(const hode_snf_desc* d) {
  return d && d->struct_size == sizeof(hode_snf_desc) && d->batch >= 1 && d->latent_dim >= 1 &&
         d->latent_dim <= HODE_SNF_MAX_LATENT && d->n_flows >= 1 && d->n_flows <= HODE_SNF_MAX_FLOWS && d->n_samples >= 1 &&
         d->n_samples <= HODE_SNF_MAX_SAMPLES;
}

static int validate(const hode_snf_desc* d) {
  if (!d) return fail(HODE_SNF_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_snf_desc))
    return fail(HODE_SNF_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_snf_desc));
  if (d->batch < 1) return fail(HODE_SNF_E_SIZE, "batch %d must be >= 1", d->batch);
  if (d->latent_dim < 1 || d->latent_dim > HODE_SNF_MAX_LATENT)
    return fail(HODE_SNF_E_SIZE, "latent_dim %d outside 1..%d", d->latent_dim, HODE_SNF_MAX_LATENT);
  if (d->n_flows < 1 || d->n_flows > HODE_SNF_MAX_FLOWS)
    return fail(HODE_SNF_E_SIZE, "n_flows %d outside 1..%d", d->n_flows, HODE_SNF_MAX_FLOWS);
  if (d->n_samples < 1 || d->n_samples > HODE_SNF_MAX_SAMPLES)
    return fail(HODE_SNF_E_SIZE, "n_samples %d outside 1..%d", d->n_samples, HODE_SNF_MAX_SAMPLES);
  if (d->n_householder < 0 || d->n_householder > HODE_SNF_MAX_HOUSEHOLDER)
    return fail(HODE_SNF_E_SIZE, "n_householder %d outside 0..%d", d->n_householder, HODE_SNF_MAX_HOUSEHOLDER);
  if (d->s_kl < 0 || d->s_kl >= d->n_samples)
    return fail(HODE_SNF_E_SIZE, "s_kl %d outside 0..n_samples-1 = %d", d->s_kl, d->n_samples - 1);
  if (!d->mu || !d->log_var || !d->full_d || !d->diag1 || !d->diag2 || !d->bias || !d->noise)
    return fail(HODE_SNF_E_NULL, "mu / log_var / full_d / diag1 / diag2 / bias / noise must be non-NULL");
  if (d->n_householder && !d->v) return fail(HODE_SNF_E_NULL, "v must be non-NULL when n_householder > 0");
  return 0;
}

static int check_workspace(const hode_snf_desc* d) {
  if (!d->workspace) return fail(HODE_SNF_E_WORKSPACE, "workspace is NULL: the states of the %d flows live there", d->n_flows);
  const size_t need = ws_bytes(d);
  if (d->workspace_bytes < need) return fail(HODE_SNF_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  if ((uintptr_t)d->workspace % 16) return fail(HODE_SNF_E_WORKSPACE, "workspace must be 16-byte aligned");
  return 0;
}

static SnfArgs args_of(const hode_snf_desc* d) {
  SnfArgs a{};
  a.mu = d->mu; a.log_var = d->log_var; a.full_d = d->full_d; a.diag1 = d->diag1; a.diag2 = d->diag2; a.bias = d->bias;
  a.v = d->v; a.noise = d->noise; a.z_out = d->z_out; a.kl = d->kl; a.ws = (float*)d->workspace;
  a.gz = d->grad_z_out; a.gkl = d->grad_kl;
  a.g_mu = d->grad_mu; a.g_lv = d->grad_log_var; a.g_fd = d->grad_full_d; a.g_d1 = d->grad_diag1; a.g_d2 = d->grad_diag2;
  a.g_bias = d->grad_bias; a.g_v = d->grad_v;
  a.B = d->batch; a.D = d->latent_dim; a.K = d->n_flows; a.S = d->n_samples; a.H = d->n_householder; a.s_kl = d->s_kl;
  return a;
}

template <int T>
static int launch(SnfArgs a, bool bwd, hipStream_t st) {
  geometry(a.B, a.S, T, a.H, bwd, &a.L, &a.ppb);
  const unsigned blocks = (unsigned)((a.B + a.ppb - 1) / a.ppb);
  const size_t lds = (size_t)a.ppb * lds_per_patient(T, a.L, a.H, bwd);
  if (bwd)
    hipLaunchKernelGGL(snf_bwd_kernel<T>, dim3(blocks), dim3(a.ppb * a.L), lds, st, a);
  else
    hipLaunchKernelGGL(snf_fwd_kernel<T>, dim3(blocks), dim3(a.ppb * a.L), lds, st, a);
  return launch_fail(hipGetLastError(), bwd ? "hode_snf_bwd launch" : "hode_snf_fwd launch");
}

static int dispatch(const SnfArgs& a, bool bwd, hipStream_t st) {
  switch (tile_of(a.D)) {
    case 4: return launch<4>(a, bwd, st);
    case 8: return launch<8>(a, bwd, st);
    case 16: return launch<16>(a, bwd, st);
    default: return launch<32>(a, bwd, st);
  }
}

}  // namespace hode_snf

extern "C" int hode_snf_version(void) { return HODE_SNF_ABI_VERSION; }

extern "C" const char* hode_snf_last_error_string(void) { return hode_side::g_err; }

extern "C" size_t hode_snf_workspace_bytes(const hode_snf_desc* d) {
  using namespace hode_snf;
  return sizes_ok(d) ? ws_bytes(d) : 0;
}

extern "C" int hode_snf_fwd(const hode_snf_desc* d, void* stream) {
  using namespace hode_snf;
  if (int e = validate(d)) return e;
  if (!d->kl) return fail(HODE_SNF_E_NULL, "kl must be non-NULL");
  if (int e = check_workspace(d)) return e;
  return dispatch(args_of(d), false, (hipStream_t)stream);
}

extern "C" int hode_snf_bwd(const hode_snf_desc* d, void* stream) {
  using namespace hode_snf;
  if (int e = validate(d)) return e;
  if (!d->grad_mu || !d->grad_log_var || !d->grad_full_d || !d->grad_diag1 || !d->grad_diag2 || !d->grad_bias ||
      (d->n_householder && !d->grad_v))
    return fail(HODE_SNF_E_NULL,
                "grad_mu / grad_log_var / grad_full_d / grad_diag1 / grad_diag2 / grad_bias (and grad_v when n_householder > 0) "
                "must be non-NULL");
  if (int e = check_workspace(d)) return e;
  return dispatch(args_of(d), true, (hipStream_t)stream);
}
