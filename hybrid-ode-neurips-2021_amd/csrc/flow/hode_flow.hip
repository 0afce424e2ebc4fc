// Planar normalizing-flow posterior with its Monte-Carlo KL against the Exponential(100) prior, forward and backward,
// one launch each, gfx950 (libhode_flow.so, C ABI include/hode_flow.h).
//
// Reference: Planar.forward (flow.py:26-59), EncoderPlanarLSTM.reparameterize / log_density (model.py:116-153),
// VariationalInferenceFlow.mc_kl (model.py:1366-1380), ExponentialPrior (model.py:41-45).  Eagerly that is ~20 element-wise
// launches per flow and draw on (B, D) tensors, 50 draws per step, plus the autograd backward of all of it.
//
// Layout.  A workgroup of 256 lanes holds 256 / L patients; the L lanes of a patient (L a power of two <= 64, chosen on
// the host from B and S) take the samples s = slot, slot + L, ...  Each lane keeps its sample's D-vector (padded to the
// tile DT) and, in the backward, the K tanh values of the recomputed forward in VGPRs.  The per-patient flow constants
// (u_hat, w, w . u_hat, b) are formed once per patient and flow in a prologue and read from LDS.  Sums over samples run in
// a fixed order: a lane walks its samples in order, the L lanes fold by a butterfly of cross-lane moves, and in the
// backward lane 0 of the group adds each fold into the patient's LDS accumulators -- no float atomics, so repeated calls
// are bit-identical.  The u_hat reparameterisation's backward runs once per patient and flow after the last sample.
#include <hip/hip_runtime.h>

#include "../../../include/hode_flow.h"
#include "../hode_common.hpp"
#include "../hode_side_error.hpp"

namespace hode_flow {

using hode::exp_full_f32;
using hode::log_f32;
using hode::tanh_precise_f32;

constexpr int kBlock = 256;
constexpr int kMaxK = HODE_FLOW_MAX_FLOWS;
constexpr float kLogSqrt2Pi = 0.9189385332046727f;
constexpr float kLogRate = 4.605170185988092f;  // log 100
constexpr float kRate = 100.0f;
constexpr int kLdsLimit = 64 * 1024;

using hode_side::fail;
using hode_side::launch_fail;

struct FlowArgs {
  const float* __restrict__ mu;
  const float* __restrict__ log_var;
  const float* __restrict__ u;
  const float* __restrict__ w;
  const float* __restrict__ b;
  const float* __restrict__ noise;
  float* __restrict__ z_out;
  float* __restrict__ kl;
  const float* __restrict__ gz;
  const float* __restrict__ gkl;
  float* __restrict__ g_mu;
  float* __restrict__ g_lv;
  float* __restrict__ g_u;
  float* __restrict__ g_w;
  float* __restrict__ g_b;
  int B, D, K, S, s_kl, L;
};

// LDS per patient and flow: [u_hat (DT) | w (DT) | w . u_hat | b]
template <int DT>
constexpr int kStride = 2 * DT + 2;

__device__ __forceinline__ float softplus_t20(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

__device__ __forceinline__ float group_sum(float v, int L) {
  for (int off = L >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// u_hat, w and w . u_hat of patient `bb`, flows k = slot, slot + L, ... into the patient's LDS block
template <int DT>
__device__ __forceinline__ void flow_prologue(const FlowArgs& a, int bb, int slot, float* prm) {
  for (int k = slot; k < a.K; k += a.L) {
    const float* uk = a.u + ((size_t)bb * a.K + k) * a.D;
    const float* wk = a.w + ((size_t)bb * a.K + k) * a.D;
    float uv[DT], wv[DT];
    float uw = 0.f, n2 = 0.f;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      uv[d] = d < a.D ? uk[d] : 0.f;
      wv[d] = d < a.D ? wk[d] : 0.f;
      uw = __builtin_fmaf(wv[d], uv[d], uw);
      n2 = __builtin_fmaf(wv[d], wv[d], n2);
    }
    const float coef = (-1.0f + softplus_t20(uw) - uw) / n2;
    float* p = prm + k * kStride<DT>;
    float c = 0.f;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const float uh = __builtin_fmaf(coef, wv[d], uv[d]);
      p[d] = uh;
      p[DT + d] = wv[d];
      c = __builtin_fmaf(wv[d], uh, c);
    }
    p[2 * DT] = c;
    p[2 * DT + 1] = a.b[(size_t)bb * a.K + k];
  }
}

template <int DT>
__global__ __launch_bounds__(kBlock) void flow_fwd_kernel(FlowArgs a) {
  extern __shared__ float lds[];
  const int L = a.L, ppb = kBlock / L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * ppb + pl;
  const bool active = bb < a.B;
  float* prm = lds + pl * (a.K * kStride<DT>);
  if (active) flow_prologue<DT>(a, bb, slot, prm);
  __syncthreads();

  float kl_sum = 0.f;
  if (active) {
    float mu[DT], sg[DT];
    float gauss_const = 0.f;  // sum_d (-log sigma - log sqrt(2 pi))
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const float lv = d < a.D ? a.log_var[(size_t)bb * a.D + d] : 0.f;
      mu[d] = d < a.D ? a.mu[(size_t)bb * a.D + d] : 0.f;
      sg[d] = exp_full_f32(0.5f * lv);
      if (d < a.D) gauss_const -= 0.5f * lv + kLogSqrt2Pi;
    }
    for (int s = slot; s < a.S; s += L) {
      const size_t row = ((size_t)s * a.B + bb) * a.D;
      float z[DT];
      float log_q = gauss_const;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const float e = d < a.D ? a.noise[row + d] : 0.f;
        z[d] = __builtin_fmaf(e, sg[d], mu[d]);
        const float t = z[d] - mu[d];
        if (d < a.D) log_q -= t * t / (2.0f * sg[d] * sg[d]);
      }
      float logdet = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < a.K) {
          const float* p = prm + k * kStride<DT>;
          float act = p[2 * DT + 1];
#pragma unroll
          for (int d = 0; d < DT; ++d) act = __builtin_fmaf(p[DT + d], z[d], act);
          const float h = tanh_precise_f32(act);
#pragma unroll
          for (int d = 0; d < DT; ++d) z[d] = __builtin_fmaf(p[d], h, z[d]);
          logdet += log_f32(fabsf(__builtin_fmaf(__builtin_fmaf(-h, h, 1.0f), p[2 * DT], 1.0f)));
        }
      }
      float log_p = 0.f;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (d < a.D) {
          const float y = z[d] - 5.0f;
          const float zo = exp_full_f32(y);
          logdet += y;
          log_p += kLogRate - kRate * zo;
          if (a.z_out) a.z_out[row + d] = zo;
        }
      }
      if (s >= a.s_kl) kl_sum += log_q - logdet - log_p;
    }
  }
  if (a.kl) {
    kl_sum = group_sum(kl_sum, L);
    if (active && slot == 0) a.kl[bb] = kl_sum / (float)(a.S - a.s_kl);
  }
}

template <int DT>
__global__ __launch_bounds__(kBlock) void flow_bwd_kernel(FlowArgs a) {
  extern __shared__ float lds[];
  const int L = a.L, ppb = kBlock / L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * ppb + pl;
  const bool active = bb < a.B;
  const int pk = a.K * kStride<DT>;
  float* prm = lds + pl * pk;
  float* acc = lds + ppb * pk + pl * pk;  // [k]: [sum zbar h (DT) | sum da z_k (DT) | sum da | sum dL/d(w . u_hat)]
  if (active) {
    flow_prologue<DT>(a, bb, slot, prm);
    for (int i = slot; i < pk; i += L) acc[i] = 0.f;
  }
  __syncthreads();

  float mu[DT], sg[DT], acc_mu[DT], acc_e[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    mu[d] = active && d < a.D ? a.mu[(size_t)bb * a.D + d] : 0.f;
    sg[d] = exp_full_f32(0.5f * (active && d < a.D ? a.log_var[(size_t)bb * a.D + d] : 0.f));
    acc_mu[d] = 0.f;
    acc_e[d] = 0.f;
  }
  const float n_kl = (float)(a.S - a.s_kl);
  const float ckl = (a.gkl && active) ? a.gkl[bb] / n_kl : 0.f;
  const int n_it = (a.S + L - 1) / L;  // the same in every lane: the folds below involve the whole group
  for (int it = 0; it < n_it; ++it) {
    const int s = it * L + slot;
    const bool valid = active && s < a.S;
    const size_t row = ((size_t)(valid ? s : 0) * a.B + (active ? bb : 0)) * a.D;
    const float c = (valid && s >= a.s_kl) ? ckl : 0.f;  // d loss / d kl_s
    float eps[DT], z[DT], zb[DT], h[kMaxK];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      eps[d] = valid && d < a.D ? a.noise[row + d] : 0.f;
      z[d] = __builtin_fmaf(eps[d], sg[d], mu[d]);
    }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < a.K) {
        const float* p = prm + k * kStride<DT>;
        float act = p[2 * DT + 1];
#pragma unroll
        for (int d = 0; d < DT; ++d) act = __builtin_fmaf(p[DT + d], z[d], act);
        h[k] = tanh_precise_f32(act);
#pragma unroll
        for (int d = 0; d < DT; ++d) z[d] = __builtin_fmaf(p[d], h[k], z[d]);
      }
    }
    // z_out = exp(z - 5): d/dz = z_out (G_z + 100 c); logdet's sum_d (z - 5): -c
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const float gz = (a.gz && valid && d < a.D) ? a.gz[row + d] : 0.f;
      zb[d] = (valid && d < a.D) ? __builtin_fmaf(exp_full_f32(z[d] - 5.0f), __builtin_fmaf(kRate, c, gz), -c) : 0.f;
    }
#pragma unroll
    for (int k = kMaxK - 1; k >= 0; --k) {
      if (k < a.K) {
        const float* p = prm + k * kStride<DT>;
        float* q = acc + k * kStride<DT>;
        const float hk = valid ? h[k] : 0.f;
        const float one_m = __builtin_fmaf(-hk, hk, 1.0f);
        const float cw = p[2 * DT];
        const float rg = __builtin_amdgcn_rcpf(__builtin_fmaf(one_m, cw, 1.0f));
        float dh = c != 0.f ? 2.0f * c * hk * cw * rg : 0.f;  // -c d log|g| / dh
#pragma unroll
        for (int d = 0; d < DT; ++d) dh = __builtin_fmaf(p[d], zb[d], dh);
        const float da = valid ? dh * one_m : 0.f;
        const float r = (valid && c != 0.f) ? -c * one_m * rg : 0.f;
        float sb = group_sum(da, L), sr = group_sum(r, L);
        if (slot == 0 && active) {
          q[2 * DT] += sb;
          q[2 * DT + 1] += sr;
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d < a.D) {
            z[d] = __builtin_fmaf(-p[d], hk, z[d]);  // z_k
            float su = group_sum(zb[d] * hk, L), sw = group_sum(valid ? da * z[d] : 0.f, L);
            if (slot == 0 && active) {
              q[d] += su;
              q[DT + d] += sw;
            }
            zb[d] = __builtin_fmaf(p[DT + d], da, zb[d]);
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      acc_mu[d] += zb[d];
      acc_e[d] = __builtin_fmaf(zb[d], eps[d], acc_e[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    if (d < a.D) {
      const float gm = group_sum(acc_mu[d], L), ge = group_sum(acc_e[d], L);
      if (active && slot == 0) {
        a.g_mu[(size_t)bb * a.D + d] = gm;
        // z0 = eps sigma + mu; sum_d log N(z0) contributes -1/2 per unit of d loss / d kl_s
        a.g_lv[(size_t)bb * a.D + d] = __builtin_fmaf(0.5f * sg[d], ge, -0.5f * ckl * n_kl);
      }
    }
  }
  __syncthreads();
  if (!active) return;
  // u_hat = u + (m(uw) - uw) w / |w|^2 with m = -1 + softplus(uw): its backward once per patient and flow
  for (int k = slot; k < a.K; k += L) {
    const float* p = prm + k * kStride<DT>;
    const float* q = acc + k * kStride<DT>;
    const float* uk = a.u + ((size_t)bb * a.K + k) * a.D;
    float uv[DT], gh[DT];
    float uw = 0.f, n2 = 0.f, gcoef = 0.f;
    const float R = q[2 * DT + 1];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      uv[d] = d < a.D ? uk[d] : 0.f;
      uw = __builtin_fmaf(p[DT + d], uv[d], uw);
      n2 = __builtin_fmaf(p[DT + d], p[DT + d], n2);
      gh[d] = __builtin_fmaf(R, p[DT + d], q[d]);  // d loss / d u_hat
      gcoef = __builtin_fmaf(gh[d], p[DT + d], gcoef);
    }
    const float sp = softplus_t20(uw);
    const float coef = (-1.0f + sp - uw) / n2;
    const float dsp = uw > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-uw));
    const float guw = gcoef * (dsp - 1.0f) / n2;
    const float gn2 = -gcoef * coef / n2;
    float* gu = a.g_u + ((size_t)bb * a.K + k) * a.D;
    float* gw = a.g_w + ((size_t)bb * a.K + k) * a.D;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d < a.D) {
        const float wd = p[DT + d];
        gu[d] = __builtin_fmaf(guw, wd, gh[d]);
        float g = __builtin_fmaf(R, p[d], q[DT + d]);  // direct: sum da z_k + R u_hat
        g = __builtin_fmaf(coef, gh[d], g);
        g = __builtin_fmaf(guw, uv[d], g);
        gw[d] = __builtin_fmaf(2.0f * gn2, wd, g);
      }
    }
    a.g_b[(size_t)bb * a.K + k] = q[2 * DT];
  }
}

static int tile_of(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

// lanes per patient: enough lanes in flight at small B, no more than the samples, and the block's LDS within the limit
static int lanes_per_patient(int B, int S, int K, int DT) {
  int L = 1;
  while (L < 64 && (long long)B * L < 131072) L <<= 1;
  int sp = 1;
  while (sp < S) sp <<= 1;
  if (L > sp) L = sp;
  const long long per_patient = 2LL * K * (2 * DT + 2) * (long long)sizeof(float);
  while (L < 64 && (kBlock / L) * per_patient > kLdsLimit) L <<= 1;
  return L;
}

static int validate(const hode_flow_desc* d) {
  if (!d) return fail(HODE_FLOW_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_flow_desc))
    return fail(HODE_FLOW_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_flow_desc));
  if (d->batch < 1) return fail(HODE_FLOW_E_SIZE, "batch %d must be >= 1", d->batch);
  if (d->latent_dim < 1 || d->latent_dim > HODE_FLOW_MAX_LATENT)
    return fail(HODE_FLOW_E_SIZE, "latent_dim %d outside 1..%d", d->latent_dim, HODE_FLOW_MAX_LATENT);
  if (d->n_flows < 1 || d->n_flows > HODE_FLOW_MAX_FLOWS)
    return fail(HODE_FLOW_E_SIZE, "n_flows %d outside 1..%d", d->n_flows, HODE_FLOW_MAX_FLOWS);
  if (d->n_samples < 1 || d->n_samples > HODE_FLOW_MAX_SAMPLES)
    return fail(HODE_FLOW_E_SIZE, "n_samples %d outside 1..%d", d->n_samples, HODE_FLOW_MAX_SAMPLES);
  if (d->s_kl < 0 || d->s_kl > 1) return fail(HODE_FLOW_E_SIZE, "s_kl %d must be 0 or 1", d->s_kl);
  if (!d->mu || !d->log_var || !d->u || !d->w || !d->b || !d->noise)
    return fail(HODE_FLOW_E_NULL, "mu / log_var / u / w / b / noise must be non-NULL");
  return 0;
}

static FlowArgs args_of(const hode_flow_desc* d) {
  FlowArgs a{};
  a.mu = d->mu; a.log_var = d->log_var; a.u = d->u; a.w = d->w; a.b = d->b; a.noise = d->noise;
  a.z_out = d->z_out; a.kl = d->kl; a.gz = d->grad_z_out; a.gkl = d->grad_kl;
  a.g_mu = d->grad_mu; a.g_lv = d->grad_log_var; a.g_u = d->grad_u; a.g_w = d->grad_w; a.g_b = d->grad_b;
  a.B = d->batch; a.D = d->latent_dim; a.K = d->n_flows; a.S = d->n_samples; a.s_kl = d->s_kl;
  return a;
}

template <int DT>
static int launch(FlowArgs a, bool bwd, hipStream_t st) {
  a.L = lanes_per_patient(a.B, a.S, a.K, DT);
  const int ppb = kBlock / a.L;
  const unsigned blocks = (unsigned)((a.B + ppb - 1) / ppb);
  const size_t lds = (size_t)(bwd ? 2 : 1) * ppb * a.K * kStride<DT> * sizeof(float);
  if (bwd)
    hipLaunchKernelGGL(flow_bwd_kernel<DT>, dim3(blocks), dim3(kBlock), lds, st, a);
  else
    hipLaunchKernelGGL(flow_fwd_kernel<DT>, dim3(blocks), dim3(kBlock), lds, st, a);
  return launch_fail(hipGetLastError(), bwd ? "hode_flow_bwd launch" : "hode_flow_fwd launch");
}

static int dispatch(const FlowArgs& a, bool bwd, hipStream_t st) {
  switch (tile_of(a.D)) {
    case 4: return launch<4>(a, bwd, st);
    case 8: return launch<8>(a, bwd, st);
    case 16: return launch<16>(a, bwd, st);
    default: return launch<32>(a, bwd, st);
  }
}

}  // namespace hode_flow

extern "C" int hode_flow_version(void) { return HODE_FLOW_ABI_VERSION; }

extern "C" const char* hode_flow_last_error_string(void) { return hode_side::g_err; }

extern "C" int hode_flow_fwd(const hode_flow_desc* d, void* stream) {
  using namespace hode_flow;
  if (int e = validate(d)) return e;
  if (!d->z_out && !d->kl) return fail(HODE_FLOW_E_NULL, "z_out and kl are both NULL: nothing to compute");
  if (d->kl && d->s_kl >= d->n_samples) return fail(HODE_FLOW_E_SIZE, "kl needs s_kl < n_samples");
  return dispatch(args_of(d), false, (hipStream_t)stream);
}

extern "C" int hode_flow_bwd(const hode_flow_desc* d, void* stream) {
  using namespace hode_flow;
  if (int e = validate(d)) return e;
  if (!d->grad_mu || !d->grad_log_var || !d->grad_u || !d->grad_w || !d->grad_b)
    return fail(HODE_FLOW_E_NULL, "grad_mu / grad_log_var / grad_u / grad_w / grad_b must be non-NULL");
  if (d->grad_kl && d->s_kl >= d->n_samples) return fail(HODE_FLOW_E_SIZE, "grad_kl needs s_kl < n_samples");
  return dispatch(args_of(d), true, (hipStream_t)stream);
}
