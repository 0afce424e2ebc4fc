// Ensemble CRPS of a weighted sum of two models' posterior forecasts: the metric of the reference's
// training_utils.evaluate_ensemble / evaluate_ensemble_horizon (training_utils.py:383-565), which decodes mc_itr draws of
// BOTH models one by one, mixes the two x_hat, stacks (T', B, obs, mc_itr) and calls properscoring.crps_ensemble element
// by element from three nested Python loops.
//
// Here each model's draws are ONE solver launch over M * B latents and this kernel scores the mixture without
// materialising either x_hat.  A workgroup of 128 threads owns `rpw` consecutive (time, patient) rows and a thread owns
// one observed component of one row: with obs = 20 six rows share a workgroup (120 of 128 lanes busy; one row per
// workgroup, hode_crps.hip's layout, would idle 108).  The rows' member vectors of both models and the two readout
// matrices are staged in LDS; every thread forms its M mixture values
//     v_m = mix_e[t][o] (We[o] . he_m + be[o]) + mix_m[t][o] (Wm[o] . hm_m + bm[o])
// into an LDS column of its own and evaluates
//     CRPS = 1/M sum_m |v_m - y|  -  1/M^2 sum_{i<j} |v_i - v_j|          (properscoring's equal-weight estimator)
// in the pairwise form, as hode_crps.hip does.  Deterministic: fixed summation order, no atomics.
//
// A library of its own (C ABI: include/hode_mix.h): its kernel stays out of libhode.so.
#include <hip/hip_runtime.h>

#include "../../../include/hode_mix.h"
#include "../hode_side_error.hpp"

namespace hode_mix {

constexpr int kMixThreads = 128;
constexpr int kMixMaxRows = 8;                       // rows per workgroup, at most
constexpr size_t kMixPackLds = 64 * 1024;            // rows are packed only while the workgroup stays below this
constexpr size_t kMixLdsLimit = 160 * 1024;          // LDS of a gfx950 workgroup
constexpr size_t kMixStaticLds = kMixThreads * sizeof(float);  // the kernel's static block (per-thread scores)

using hode_side::fail;
using hode_side::launch_fail;

struct MixArgs {
  const float* __restrict__ he;
  const float* __restrict__ hm;
  const float* __restrict__ we;
  const float* __restrict__ be;
  const float* __restrict__ wm;
  const float* __restrict__ bm;
  const float* __restrict__ ge;   // mixing weights [T'][obs] or NULL
  const float* __restrict__ gm;
  const float* __restrict__ truth;
  float* __restrict__ crps;
  float* __restrict__ crps_sum;
  long long tse, mse, pse, tsm, msm, psm;
  long long rows;                 // T' * B
  int B, M, De, Dm, obs, rpw;
};

// dynamic LDS of a workgroup of `rpw` rows: member vectors of both models, both readouts, one value column per thread
static size_t mix_lds_bytes(int rpw, int M, int De, int Dm, int obs) {
  return sizeof(float) * ((size_t)rpw * M * (De + Dm) + (size_t)(De + Dm) * obs + (size_t)M * kMixThreads);
}

// as many rows as fit the workgroup's threads, at most kMixMaxRows, fewer while the LDS would pass kMixPackLds
static int mix_rows_per_workgroup(int M, int De, int Dm, int obs) {
  int rpw = kMixThreads / obs;
  if (rpw > kMixMaxRows) rpw = kMixMaxRows;
  while (rpw > 1 && mix_lds_bytes(rpw, M, De, Dm, obs) + kMixStaticLds > kMixPackLds) --rpw;
  return rpw;
}

__device__ __forceinline__ void stage_members(float* dst, const float* __restrict__ src, long long ms, int M, int D, int tid) {
  for (int idx = tid; idx < M * D; idx += kMixThreads) {
    const int m = idx / D, d = idx - m * D;
    dst[idx] = src[m * ms + d];
  }
}

__device__ __forceinline__ void stage_readout(float* dst, const float* __restrict__ w, int obs, int D, int tid) {
  for (int idx = tid; idx < obs * D; idx += kMixThreads) {
    const int o = idx / D, d = idx - o * D;
    dst[d * obs + o] = w[idx];   // component-minor: the lanes of a row read consecutive words
  }
}

__global__ __launch_bounds__(kMixThreads) void mix_crps_kernel(MixArgs a) {
  extern __shared__ float lds[];
  __shared__ float score[kMixThreads];                    // per-thread CRPS, summed per row in a fixed order
  static_assert(sizeof(score) == kMixStaticLds, "the host's LDS rule counts this block");
  float* he = lds;                                        // [rpw][M][De]
  float* hm = he + a.rpw * a.M * a.De;                    // [rpw][M][Dm]
  float* weT = hm + a.rpw * a.M * a.Dm;                   // [De][obs]
  float* wmT = weT + a.De * a.obs;                        // [Dm][obs]
  float* vals = wmT + a.Dm * a.obs;                       // [M][128] mixture values, one column per thread
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * a.rpw;
  for (int r = 0; r < a.rpw; ++r) {
    const long long row = row0 + r;
    if (row >= a.rows) break;
    const long long t = row / a.B, b = row - t * a.B;
    stage_members(he + r * a.M * a.De, a.he + t * a.tse + b * a.pse, a.mse, a.M, a.De, tid);
    stage_members(hm + r * a.M * a.Dm, a.hm + t * a.tsm + b * a.psm, a.msm, a.M, a.Dm, tid);
  }
  stage_readout(weT, a.we, a.obs, a.De, tid);
  stage_readout(wmT, a.wm, a.obs, a.Dm, tid);
  __syncthreads();
  const int r = tid / a.obs, o = tid - r * a.obs;
  const long long row = row0 + r;
  const bool active = r < a.rpw && row < a.rows;
  float c = 0.f;
  if (active) {
    const long long t = row / a.B;
    const float y = a.truth[row * a.obs + o];
    const float ge = a.ge ? a.ge[t * a.obs + o] : 1.f;
    const float gm = a.gm ? a.gm[t * a.obs + o] : 1.f;
    const float be = a.be ? a.be[o] : 0.f;
    const float bm = a.bm ? a.bm[o] : 0.f;
    const float* hre = he + r * a.M * a.De;
    const float* hrm = hm + r * a.M * a.Dm;
    float s1 = 0.f;
    for (int m = 0; m < a.M; ++m) {
      float ve = be, vm = bm;
      for (int d = 0; d < a.De; ++d) ve = __builtin_fmaf(weT[d * a.obs + o], hre[m * a.De + d], ve);
      for (int d = 0; d < a.Dm; ++d) vm = __builtin_fmaf(wmT[d * a.obs + o], hrm[m * a.Dm + d], vm);
      const float v = __builtin_fmaf(gm, vm, ge * ve);
      vals[m * kMixThreads + tid] = v;
      s1 += __builtin_fabsf(v - y);
    }
    // each thread reads back only its own column: no barrier needed
    float s2 = 0.f;
    for (int i = 1; i < a.M; ++i) {
      const float xi = vals[i * kMixThreads + tid];
      float acc = 0.f;
      for (int j = 0; j < i; ++j) acc += __builtin_fabsf(xi - vals[j * kMixThreads + tid]);
      s2 += acc;
    }
    const float inv = 1.0f / (float)a.M;
    c = s1 * inv - s2 * inv * inv;
    if (a.crps) a.crps[row * a.obs + o] = c;
  }
  if (a.crps_sum) {
    score[tid] = c;
    __syncthreads();
    if (active && o == 0) {
      float s = 0.f;
      for (int k = 0; k < a.obs; ++k) s += score[tid + k];   // tid + k <= r * obs + obs - 1 < 128
      a.crps_sum[row] = s;
    }
  }
}

}  // namespace hode_mix

extern "C" int hode_mix_version(void) { return HODE_MIX_ABI_VERSION; }

extern "C" const char* hode_mix_last_error_string(void) { return hode_side::g_err; }

extern "C" int hode_mix_crps(const hode_mix_crps_desc* d, void* stream) {
  using namespace hode_mix;
  if (!d) return fail(HODE_MIX_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_mix_crps_desc))
    return fail(HODE_MIX_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_mix_crps_desc));
  if (d->n_times <= 0 || d->batch <= 0) return fail(HODE_MIX_E_SIZE, "n_times %d / batch %d must be positive", d->n_times, d->batch);
  if (d->obs_dim < 1 || d->obs_dim > HODE_MIX_MAX_DIM)
    return fail(HODE_MIX_E_SIZE, "obs_dim %d outside 1..%d", d->obs_dim, HODE_MIX_MAX_DIM);
  if (d->n_members < 1 || d->n_members > HODE_MIX_MAX_DIM)
    return fail(HODE_MIX_E_SIZE, "n_members %d outside 1..%d", d->n_members, HODE_MIX_MAX_DIM);
  if (d->latent_dim_e < 1 || d->latent_dim_e > HODE_MIX_MAX_DIM || d->latent_dim_m < 1 || d->latent_dim_m > HODE_MIX_MAX_DIM)
    return fail(HODE_MIX_E_SIZE, "latent_dim_e %d / latent_dim_m %d outside 1..%d", d->latent_dim_e, d->latent_dim_m,
                HODE_MIX_MAX_DIM);
  if ((long long)d->n_times * d->batch > 0x7fffffffLL) return fail(HODE_MIX_E_SIZE, "n_times * batch exceeds 2^31");
  if (d->time_stride_e < 0 || d->member_stride_e < 0 || d->patient_stride_e < 0 || d->time_stride_m < 0 ||
      d->member_stride_m < 0 || d->patient_stride_m < 0)
    return fail(HODE_MIX_E_SIZE, "negative stride");
  const int rpw = mix_rows_per_workgroup(d->n_members, d->latent_dim_e, d->latent_dim_m, d->obs_dim);
  const size_t lds = mix_lds_bytes(rpw, d->n_members, d->latent_dim_e, d->latent_dim_m, d->obs_dim);
  if (lds + kMixStaticLds > kMixLdsLimit)
    return fail(HODE_MIX_E_UNSUPPORTED, "obs_dim %d, n_members %d, latent_dim %d + %d need %zu B of LDS (limit %zu)",
                d->obs_dim, d->n_members, d->latent_dim_e, d->latent_dim_m, lds + kMixStaticLds, kMixLdsLimit);
  if (!d->h_e || !d->h_m || !d->w_e || !d->w_m || !d->truth) return fail(HODE_MIX_E_NULL, "h_e / h_m / w_e / w_m / truth is NULL");
  if (!d->crps && !d->crps_sum) return fail(HODE_MIX_E_NULL, "crps and crps_sum are both NULL: nothing to compute");
  MixArgs a{};
  a.he = d->h_e; a.hm = d->h_m; a.we = d->w_e; a.be = d->b_e; a.wm = d->w_m; a.bm = d->b_m;
  a.ge = d->mix_e; a.gm = d->mix_m; a.truth = d->truth; a.crps = d->crps; a.crps_sum = d->crps_sum;
  a.tse = d->time_stride_e; a.mse = d->member_stride_e; a.pse = d->patient_stride_e;
  a.tsm = d->time_stride_m; a.msm = d->member_stride_m; a.psm = d->patient_stride_m;
  a.rows = (long long)d->n_times * d->batch;
  a.B = d->batch; a.M = d->n_members; a.De = d->latent_dim_e; a.Dm = d->latent_dim_m; a.obs = d->obs_dim; a.rpw = rpw;
  if (lds + kMixStaticLds > 64 * 1024)
    if (int e = launch_fail(hipFuncSetAttribute((const void*)mix_crps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)lds), "mix crps LDS attribute")) return e;
  const long long blocks = (a.rows + rpw - 1) / rpw;
  hipLaunchKernelGGL(mix_crps_kernel, dim3((unsigned)blocks), dim3(kMixThreads), lds, (hipStream_t)stream, a);
  return launch_fail(hipGetLastError(), "hode_mix_crps launch");
}
