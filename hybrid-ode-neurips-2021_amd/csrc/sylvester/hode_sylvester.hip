// A chain of K Sylvester normalizing flows over S draws per patient, forward and backward, one launch each, gfx950
// (libhode_sylvester.so, C ABI include/hode_sylvester.h).
//
// Reference: Sylvester._forward (flow.py:86-134) and TriangularSylvester._forward (flow.py:160-215).  Eagerly that is four
// bmm calls on per-patient (D x M) / (M x M) matrices and a dozen element-wise launches per flow and draw, plus the
// autograd backward of all of it.
//
// Layout.  A workgroup holds `ppb` patients of L lanes each (L a power of two <= 64, ppb L <= 256, both chosen on the
// host from B, S, the tile and the LDS a patient needs); the L lanes of a patient take the draws s = slot, slot + L, ...
// The flows are streamed: per flow a prologue forms the patient's A = Q R2^T, C = Q R1 (or their gathers in triangular
// mode), b and the diagonal products r1_mm r2_mm once, into LDS, zero-padded to the tile T >= max(D, M); then every lane
// walks its draws with the M-vectors (a, h, hbar, abar) in VGPRs and the loops over d left as loops (the D-vectors are read
// where they lie, in global memory or in the lane's LDS slots: 143 VGPRs at the largest tile, no scratch).  Between flows a draw's state lives in global memory: the forward
// writes z_1 .. z_{K-1} into the caller's workspace (the tape) and the backward reads them back, keeping the running
// cotangent of z in grad_z0.  A lane only ever re-reads rows it wrote itself.
//
// Parameter gradients are sums over the draws of a patient of outer products (zbar h^T, z abar^T).  Folding D M values
// across lanes by butterflies would cost 2 D M log2(L) cross-lane moves per draw; instead every lane stages its five
// vectors (zbar, h, z, abar, the diagonal term) in LDS, and the lanes of the patient each own a slice of the (d, m)
// entries and add the L staged draws in lane order into the patient's LDS accumulators.  One owner per entry and a fixed
// order: no float atomics, repeated calls are bit-identical.  The chain rule through A, C and the diagonal products runs
// once per patient and flow in an epilogue.
#include <hip/hip_runtime.h>

#include "../../../include/hode_sylvester.h"
#include "../hode_common.hpp"
#include "../hode_side_error.hpp"

namespace hode_sylvester {

using hode::log_f32;
using hode::tanh_precise_f32;
using hode_side::fail;
using hode_side::launch_fail;

constexpr int kBlock = 256;
constexpr int kLdsLimit = 64 * 1024;
constexpr int kStage = 5;  // staged vectors per lane in the backward: zbar | h | z | abar | diagonal term

struct SylArgs {
  const float* __restrict__ z0;
  const float* __restrict__ r1;
  const float* __restrict__ r2;
  const float* __restrict__ b;
  const float* __restrict__ q;
  const int* __restrict__ perm;
  float* z_out;
  float* logdet;
  float* log_diag;
  float* tape;
  const float* gz;
  const float* gld;
  const float* gdiag;
  float* g_z0;
  float* g_r1;
  float* g_r2;
  float* g_b;
  float* g_q;
  int B, D, M, K, S, L, ppb;
};

// LDS per patient, one flow at a time: [A (T x T) | C (T x T) | b (T) | r1_mm r2_mm (T)]; the backward's accumulators
// [sum z abar^T | sum zbar h^T | sum abar | sum diagonal term] have the same shape
template <int T>
constexpr int kPrm = 2 * T * T + 2 * T;

// how many iterations of a loop over d (one row of A or C against an M-vector in VGPRs) are in flight at once: each waits
// for a load of z[d], so one at a time leaves its latency bare; more than this spills at the largest tile
template <int T>
constexpr int kUnroll = T >= 32 ? 2 : 4;

// A, C, b and the diagonal products of patient `bb`, flow `k`, zero outside D x M
template <int T>
__device__ __forceinline__ void flow_prologue(const SylArgs& a, int bb, int k, int slot, float* prm) {
  const int D = a.D, M = a.M;
  const size_t pk = (size_t)bb * a.K + k;
  const float* r1 = a.r1 + pk * M * M;
  const float* r2 = a.r2 + pk * M * M;
  const float* q = a.q ? a.q + pk * D * M : nullptr;
  const int* p = a.perm ? a.perm + (size_t)k * D : nullptr;
  for (int idx = slot; idx < T * T; idx += a.L) {
    const int d = idx / T, m = idx % T;
    float av = 0.f, cv = 0.f;
    if (d < D && m < M) {
      if (q) {
#pragma unroll 4
        for (int j = 0; j < M; ++j) {
          const float qv = q[d * M + j];
          av = __builtin_fmaf(qv, r2[m * M + j], av);
          cv = __builtin_fmaf(qv, r1[j * M + m], cv);
        }
      } else {
#pragma unroll 4
        for (int j = 0; j < M; ++j)
          if ((p ? p[j] : j) == d) av += r2[m * M + j];
        const int pd = p ? p[d] : d;
        if ((unsigned)pd < (unsigned)D) cv = r1[pd * M + m];
      }
    }
    prm[idx] = av;
    prm[T * T + idx] = cv;
  }
  for (int m = slot; m < T; m += a.L) {
    prm[2 * T * T + m] = m < M ? a.b[pk * M + m] : 0.f;
    prm[2 * T * T + T + m] = m < M ? r1[m * M + m] * r2[m * M + m] : 0.f;
  }
}

// h = tanh(z A + b), zero past M; z[d] is read through `zrow` (global or LDS), so that only the M-vector is in VGPRs and
// the loop over d stays a loop
template <int T>
__device__ __forceinline__ void flow_act(const SylArgs& a, const float* prm, const float* zrow, float (&h)[T]) {
#pragma unroll
  for (int m = 0; m < T; ++m) h[m] = prm[2 * T * T + m];
#pragma unroll kUnroll<T>
  for (int d = 0; d < a.D; ++d) {
    const float zd = zrow[d];
#pragma unroll
    for (int m = 0; m < T; ++m) h[m] = __builtin_fmaf(zd, prm[d * T + m], h[m]);
  }
#pragma unroll
  for (int m = 0; m < T; ++m) h[m] = m < a.M ? tanh_precise_f32(h[m]) : 0.f;
}

template <int T>
__global__ __launch_bounds__(kBlock) void sylvester_fwd_kernel(SylArgs a) {
  extern __shared__ float lds[];
  const int L = a.L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * a.ppb + pl;
  const bool active = bb < a.B;
  float* prm = lds + pl * kPrm<T>;
  const size_t sbd = (size_t)a.S * a.B * a.D;
  for (int k = 0; k < a.K; ++k) {
    if (k) __syncthreads();  // every lane is done with the previous flow's constants
    if (active) flow_prologue<T>(a, bb, k, slot, prm);
    __syncthreads();
    if (!active) continue;
    const float* src = k == 0 ? a.z0 : (a.tape ? a.tape + (size_t)(k - 1) * sbd : a.z_out);
    float* dst = k == a.K - 1 ? a.z_out : (a.tape ? a.tape + (size_t)k * sbd : a.z_out);
    for (int s = slot; s < a.S; s += L) {
      const size_t sb = (size_t)s * a.B + bb;
      const size_t row = sb * a.D;
      float h[T];
      flow_act<T>(a, prm, src + row, h);
#pragma unroll kUnroll<T>
      for (int d = 0; d < a.D; ++d) {
        float v = src[row + d];
#pragma unroll
        for (int m = 0; m < T; ++m) v = __builtin_fmaf(h[m], prm[T * T + d * T + m], v);
        dst[row + d] = v;  // dst may be src (no tape): row d is read before it is written, by this lane alone
      }
      float ld = 0.f;
#pragma unroll
      for (int m = 0; m < T; ++m) {
        if (m < a.M) {
          const float v = log_f32(fabsf(__builtin_fmaf(__builtin_fmaf(-h[m], h[m], 1.0f), prm[2 * T * T + T + m], 1.0f)));
          ld += v;
          if (a.log_diag) a.log_diag[(sb * a.K + k) * a.M + m] = v;
        }
      }
      a.logdet[sb] = k == 0 ? ld : a.logdet[sb] + ld;
    }
  }
}

// the chain rule through A, C and the diagonal products of patient `bb`, flow `k`, from the patient's accumulators
template <int T>
__device__ __forceinline__ void flow_epilogue(const SylArgs& a, int bb, int k, int slot, const float* acc) {
  const int D = a.D, M = a.M;
  const size_t pk = (size_t)bb * a.K + k;
  const float* r1 = a.r1 + pk * M * M;
  const float* r2 = a.r2 + pk * M * M;
  const float* q = a.q ? a.q + pk * D * M : nullptr;
  const int* p = a.perm ? a.perm + (size_t)k * D : nullptr;
  const float* acc_a = acc;
  const float* acc_c = acc + T * T;
  const float* acc_b = acc + 2 * T * T;
  const float* acc_dd = acc_b + T;
  if (q) {
    float* gq = a.g_q + pk * D * M;
    for (int idx = slot; idx < D * M; idx += a.L) {
      const int d = idx / M, j = idx % M;
      float v = 0.f;
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        v = __builtin_fmaf(acc_a[d * T + m], r2[m * M + j], v);
        v = __builtin_fmaf(acc_c[d * T + m], r1[j * M + m], v);
      }
      gq[idx] = v;
    }
  }
  float* gr1 = a.g_r1 + pk * M * M;
  float* gr2 = a.g_r2 + pk * M * M;
  for (int idx = slot; idx < M * M; idx += a.L) {
    const int row = idx / M, col = idx % M;  // grad_r2[m = row][j = col], grad_r1[j = row][m = col]
    float v2 = 0.f, v1 = 0.f;
    if (q) {
#pragma unroll 4
      for (int d = 0; d < D; ++d) {
        v2 = __builtin_fmaf(acc_a[d * T + row], q[d * M + col], v2);
        v1 = __builtin_fmaf(q[d * M + row], acc_c[d * T + col], v1);
      }
    } else {
      const int pj = p ? p[col] : col;
      if ((unsigned)pj < (unsigned)D) v2 = acc_a[pj * T + row];
      for (int i = 0; i < D; ++i)
        if ((p ? p[i] : i) == row) v1 += acc_c[i * T + col];
    }
    if (row == col) {
      v2 = __builtin_fmaf(acc_dd[row], r1[idx], v2);
      v1 = __builtin_fmaf(acc_dd[row], r2[idx], v1);
    }
    gr2[idx] = v2;
    gr1[idx] = v1;
  }
  for (int m = slot; m < M; m += a.L) a.g_b[pk * M + m] = acc_b[m];
}

template <int T>
__global__ __launch_bounds__(kBlock) void sylvester_bwd_kernel(SylArgs a) {
  extern __shared__ float lds[];
  const int L = a.L;
  const int pl = threadIdx.x / L, slot = threadIdx.x % L;
  const int bb = blockIdx.x * a.ppb + pl;
  const bool active = bb < a.B;
  float* prm = lds + (size_t)pl * (2 * kPrm<T> + L * kStage * T);
  float* acc = prm + kPrm<T>;
  float* stg = acc + kPrm<T>;
  float* mine = stg + slot * kStage * T;
  const size_t sbd = (size_t)a.S * a.B * a.D;
  const int n_it = (a.S + L - 1) / L;  // the same in every lane: the barriers below involve the whole workgroup
  for (int k = a.K - 1; k >= 0; --k) {
    __syncthreads();  // the previous flow's epilogue is done with the constants and the accumulators
    if (active) {
      flow_prologue<T>(a, bb, k, slot, prm);
      for (int i = slot; i < kPrm<T>; i += L) acc[i] = 0.f;
    }
    __syncthreads();
    const float* src = k == 0 ? a.z0 : a.tape + (size_t)(k - 1) * sbd;
    const float* zb_src = k == a.K - 1 ? a.gz : a.g_z0;
    for (int it = 0; it < n_it; ++it) {
      const int s = it * L + slot;
      const bool valid = active && s < a.S;
      const size_t sb = valid ? (size_t)s * a.B + bb : 0;
      const size_t row = sb * a.D;
      float h[T], hb[T];
      // this lane's z_k and zbar go to its LDS slots first and are read back from there (by this lane here, by the
      // owners of the accumulators after the barrier)
      for (int d = 0; d < T; ++d) {
        mine[d] = valid && d < a.D && zb_src ? zb_src[row + d] : 0.f;
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
      const float g_sum = a.gld && valid ? a.gld[sb] : 0.f;
#pragma unroll
      for (int m = 0; m < T; ++m) {
        const bool live = valid && m < a.M;
        const float g = g_sum + (a.gdiag && live ? a.gdiag[(sb * a.K + k) * a.M + m] : 0.f);
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
        if (valid) a.g_z0[row + d] = v;
      }
      __syncthreads();
      if (active) {
        for (int idx = slot; idx < T * T; idx += L) {
          const int d = idx / T, m = idx % T;
          if (d < a.D && m < a.M) {
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
        for (int m = slot; m < a.M; m += L) {
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
    if (active) flow_epilogue<T>(a, bb, k, slot, acc);
  }
}

static int tile_of(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }

static size_t lds_per_patient(int T, int L, bool bwd) {
  const size_t prm = 2 * (size_t)T * T + 2 * (size_t)T;
  return sizeof(float) * (bwd ? 2 * prm + (size_t)L * kStage * T : prm);
}

// lanes per patient and patients per workgroup: enough lanes in flight at small B, no more than the draws but at least
// min(T, 64) for the per-patient prologue and epilogue, whole waves where a workgroup has 64 lanes, LDS within the limit
static void geometry(int B, int S, int T, bool bwd, int* lanes, int* patients) {
  int L = 1;
  while (L < 64 && (long long)B * L < 131072) L <<= 1;
  int sp = 1;
  while (sp < S) sp <<= 1;
  if (L > sp) L = sp;
  if (L < T) L = T;
  if (L > 64) L = 64;
  int p = kBlock / L;
  const int cap = (int)(kLdsLimit / lds_per_patient(T, L, bwd));  // >= 1: T = 32, L = 64 needs 57 856 B in the backward
  if (p > cap) p = cap;
  if (p * L >= 64) p -= p % (64 / L);
  if (p > B) p = B;
  *lanes = L;
  *patients = p;
}

static size_t tape_bytes(const hode_sylvester_desc* d) {
  const size_t n = (size_t)(d->n_flows - 1) * d->n_samples * d->batch * d->latent_dim * sizeof(float);
  return (n + 255) / 256 * 256;
}

static int validate(const hode_sylvester_desc* d) {
  if (!d) return fail(HODE_SYLVESTER_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_sylvester_desc))
    return fail(HODE_SYLVESTER_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_sylvester_desc));
  if (d->batch < 1) return fail(HODE_SYLVESTER_E_SIZE, "batch %d must be >= 1", d->batch);
  if (d->latent_dim < 1 || d->latent_dim > HODE_SYLVESTER_MAX_LATENT)
    return fail(HODE_SYLVESTER_E_SIZE, "latent_dim %d outside 1..%d", d->latent_dim, HODE_SYLVESTER_MAX_LATENT);
  if (d->n_ortho < 1 || d->n_ortho > HODE_SYLVESTER_MAX_ORTHO)
    return fail(HODE_SYLVESTER_E_SIZE, "n_ortho %d outside 1..%d", d->n_ortho, HODE_SYLVESTER_MAX_ORTHO);
  if (d->n_flows < 1 || d->n_flows > HODE_SYLVESTER_MAX_FLOWS)
    return fail(HODE_SYLVESTER_E_SIZE, "n_flows %d outside 1..%d", d->n_flows, HODE_SYLVESTER_MAX_FLOWS);
  if (d->n_samples < 1 || d->n_samples > HODE_SYLVESTER_MAX_SAMPLES)
    return fail(HODE_SYLVESTER_E_SIZE, "n_samples %d outside 1..%d", d->n_samples, HODE_SYLVESTER_MAX_SAMPLES);
  if (!d->q && d->n_ortho != d->latent_dim)
    return fail(HODE_SYLVESTER_E_SIZE, "triangular mode (q is NULL) needs n_ortho %d == latent_dim %d", d->n_ortho, d->latent_dim);
  if (d->q && d->perm) return fail(HODE_SYLVESTER_E_SIZE, "perm belongs to triangular mode (q must be NULL)");
  if (!d->z0 || !d->r1 || !d->r2 || !d->b) return fail(HODE_SYLVESTER_E_NULL, "z0 / r1 / r2 / b must be non-NULL");
  return 0;
}

static int check_tape(const hode_sylvester_desc* d, bool required) {
  if (!d->workspace) {
    if (required) return fail(HODE_SYLVESTER_E_WORKSPACE, "workspace is NULL: the backward of %d flows reads the forward's tape", d->n_flows);
    return 0;
  }
  const size_t need = tape_bytes(d);
  if (d->workspace_bytes < need)
    return fail(HODE_SYLVESTER_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  if ((uintptr_t)d->workspace % 16) return fail(HODE_SYLVESTER_E_WORKSPACE, "workspace must be 16-byte aligned");
  return 0;
}

static SylArgs args_of(const hode_sylvester_desc* d) {
  SylArgs a{};
  a.z0 = d->z0; a.r1 = d->r1; a.r2 = d->r2; a.b = d->b; a.q = d->q; a.perm = d->perm;
  a.z_out = d->z_out; a.logdet = d->logdet; a.log_diag = d->log_diag;
  a.tape = d->n_flows > 1 ? (float*)d->workspace : nullptr;
  a.gz = d->grad_z_out; a.gld = d->grad_logdet; a.gdiag = d->grad_log_diag;
  a.g_z0 = d->grad_z0; a.g_r1 = d->grad_r1; a.g_r2 = d->grad_r2; a.g_b = d->grad_b; a.g_q = d->grad_q;
  a.B = d->batch; a.D = d->latent_dim; a.M = d->n_ortho; a.K = d->n_flows; a.S = d->n_samples;
  return a;
}

template <int T>
static int launch(SylArgs a, bool bwd, hipStream_t st) {
  geometry(a.B, a.S, T, bwd, &a.L, &a.ppb);
  const unsigned blocks = (unsigned)((a.B + a.ppb - 1) / a.ppb);
  const size_t lds = (size_t)a.ppb * lds_per_patient(T, a.L, bwd);
  if (bwd)
    hipLaunchKernelGGL(sylvester_bwd_kernel<T>, dim3(blocks), dim3(a.ppb * a.L), lds, st, a);
  else
    hipLaunchKernelGGL(sylvester_fwd_kernel<T>, dim3(blocks), dim3(a.ppb * a.L), lds, st, a);
  return launch_fail(hipGetLastError(), bwd ? "hode_sylvester_bwd launch" : "hode_sylvester_fwd launch");
}

static int dispatch(const SylArgs& a, bool bwd, hipStream_t st) {
  switch (tile_of(a.D > a.M ? a.D : a.M)) {
    case 4: return launch<4>(a, bwd, st);
    case 8: return launch<8>(a, bwd, st);
    case 16: return launch<16>(a, bwd, st);
    default: return launch<32>(a, bwd, st);
  }
}

}  // namespace hode_sylvester

extern "C" int hode_sylvester_version(void) { return HODE_SYLVESTER_ABI_VERSION; }

extern "C" const char* hode_sylvester_last_error_string(void) { return hode_side::g_err; }

extern "C" size_t hode_sylvester_workspace_bytes(const hode_sylvester_desc* d) {
  using namespace hode_sylvester;
  if (!d || d->struct_size != sizeof(hode_sylvester_desc) || d->batch < 1 || d->latent_dim < 1 ||
      d->latent_dim > HODE_SYLVESTER_MAX_LATENT || d->n_flows < 1 || d->n_flows > HODE_SYLVESTER_MAX_FLOWS ||
      d->n_samples < 1 || d->n_samples > HODE_SYLVESTER_MAX_SAMPLES)
    return 0;
  return tape_bytes(d);
}

extern "C" int hode_sylvester_fwd(const hode_sylvester_desc* d, void* stream) {
  using namespace hode_sylvester;
  if (int e = validate(d)) return e;
  if (!d->z_out || !d->logdet) return fail(HODE_SYLVESTER_E_NULL, "z_out / logdet must be non-NULL");
  if (int e = check_tape(d, false)) return e;
  return dispatch(args_of(d), false, (hipStream_t)stream);
}

extern "C" int hode_sylvester_bwd(const hode_sylvester_desc* d, void* stream) {
  using namespace hode_sylvester;
  if (int e = validate(d)) return e;
  if (!d->grad_z0 || !d->grad_r1 || !d->grad_r2 || !d->grad_b || (d->q && !d->grad_q))
    return fail(HODE_SYLVESTER_E_NULL, "grad_z0 / grad_r1 / grad_r2 / grad_b (and grad_q in dense mode) must be non-NULL");
  if (int e = check_tape(d, d->n_flows > 1)) return e;
  return dispatch(args_of(d), true, (hipStream_t)stream);
}
