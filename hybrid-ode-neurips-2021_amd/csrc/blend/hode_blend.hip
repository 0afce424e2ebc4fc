// The scoring arithmetic of the reference's real-data two-model scripts (experiments/run_real_ensemble.py,
// run_real_residual.py; the horizon tail is run_real.py's too), which the scripts keep in run():
//
//  * the stacking fit (run_real_ensemble.py:109-117): per forecast step a two-column scipy.optimize.nnls over the step's
//    B * obs entries, one torch -> numpy -> scipy round trip per step.  Here ONE launch covers all steps: the five Gram sums
//    of a step are reduced in float64 (fp32 x fp32 products are exact there; det = a11 a22 - a12^2 cancels when the two
//    forecasts are close, which they are) and the 2-column problem is solved in closed form (include/hode_blend.h).
//    Steps of at most kWaveRows entries take one wave each, four steps per workgroup (nnls2_wave_kernel); longer steps
//    take a workgroup each (nnls2_block_kernel).
//
//  * the horizon tail (run_real_ensemble.py:144-154): for each of four horizons the blend, the masked squared error and
//    the mask count are re-formed from full (T', B, obs) slices.  Here a thread owns one (patient, component) pair, walks
//    the forecast steps once and snapshots its running float64 sums at every horizon end; the workgroup then adds a
//    patient's components in a fixed order (horizon_sse_kernel).  A workgroup's threads read consecutive words of a step.
//
// Deterministic: fixed summation order, no atomics.  A library of its own (C ABI: include/hode_blend.h).
#include <hip/hip_runtime.h>

#include "../../../include/hode_blend.h"
#include "../hode_side_error.hpp"

namespace hode_blend {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaveRows = 256;       // steps of at most this many entries are reduced by one wave each
constexpr double kDecreaseSlack = 1e-9;  // relative slack of solve2's check of the unconstrained candidate

using hode_side::fail;
using hode_side::launch_fail;

struct Nnls2Args {
  const float* __restrict__ xe;
  const float* __restrict__ xm;
  const float* __restrict__ b;
  float* __restrict__ w;
  long long rows, se, sm, sb;
  int steps;
};

// the closed form of the two-column problem, float64 (include/hode_blend.h).  Plain IEEE arithmetic, no contraction: with
// a fused det = fma(a11, a22, -(a12 * a12)) a rank-deficient step (one row; x_m = x_e) gets the rounding residue of
// a12 * a12 as its determinant instead of 0, and weights that are noise over noise.
__device__ __forceinline__ void solve2(double a11, double a22, double a12, double b1, double b2, float* w) {
#pragma clang fp contract(off)
  double w1 = 0.0, w2 = 0.0;
  bool both = false;
  const double g1 = (a11 > 0.0 && b1 > 0.0) ? b1 * b1 / a11 : 0.0;   // residual decrease of each column alone
  const double g2 = (a22 > 0.0 && b2 > 0.0) ? b2 * b2 / a22 : 0.0;
  const double gmax = g1 >= g2 ? g1 : g2;
  const double det = a11 * a22 - a12 * a12;
  if (det > 0.0) {
    const double u1 = (a22 * b1 - a12 * b2) / det, u2 = (a11 * b2 - a12 * b1) / det;
    if (u1 > 0.0 && u2 > 0.0) {
      // the unconstrained minimiser decreases the residual by at least what either column does alone; a candidate that
      // does not (or is not finite: the comparison is then false) came from a determinant that is rounding noise
      const double dec = 2.0 * (u1 * b1 + u2 * b2) - (u1 * u1 * a11 + 2.0 * (u1 * u2 * a12) + u2 * u2 * a22);
      if (dec >= gmax - kDecreaseSlack * gmax) { w1 = u1; w2 = u2; both = true; }
    }
  }
  if (!both) {
    if (g1 >= g2) { if (g1 > 0.0) w1 = b1 / a11; }
    else w2 = b2 / a22;
  }
  w[0] = (float)w1;
  w[1] = (float)w2;
}

// G consecutive threads (G = 64 or 256) reduce the Gram sums of one step; every thread of the workgroup calls this
template <int G>
__device__ __forceinline__ void nnls2_step(const Nnls2Args& a, long long step, bool live, double (*red)[kThreads]) {
  const int tid = threadIdx.x, lane = tid % G;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
    const float* __restrict__ xe = a.xe + step * a.se;
    const float* __restrict__ xm = a.xm + step * a.sm;
    const float* __restrict__ b = a.b + step * a.sb;
#pragma unroll 4
    for (long long r = lane; r < a.rows; r += G) {
      const double e = (double)xe[r], m = (double)xm[r], y = (double)b[r];
      s[0] += e * e; s[1] += m * m; s[2] += e * m; s[3] += e * y; s[4] += m * y;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int half = G / 2; half > 0; half >>= 1) {
    if (lane < half) {
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + half];
    }
    __syncthreads();
  }
  if (live && lane == 0) solve2(red[0][tid], red[1][tid], red[2][tid], red[3][tid], red[4][tid], a.w + 2 * step);
}

__global__ __launch_bounds__(kThreads) void nnls2_wave_kernel(Nnls2Args a) {
  __shared__ double red[5][kThreads];
  const long long step = (long long)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  nnls2_step<kWave>(a, step, step < a.steps, red);
}

__global__ __launch_bounds__(kThreads) void nnls2_block_kernel(Nnls2Args a) {
  __shared__ double red[5][kThreads];
  nnls2_step<kThreads>(a, blockIdx.x, true, red);
}

struct HorizonArgs {
  const float* __restrict__ xe;
  const float* __restrict__ xm;
  const float* __restrict__ we;
  const float* __restrict__ wm;
  const float* __restrict__ truth;
  const float* __restrict__ mask;
  float* __restrict__ sse;
  float* __restrict__ cnt;
  long long ts, ps;
  int B, obs, H, ppw;                     // ppw: patients per workgroup, ppw * obs <= kThreads
  int ends[HODE_BLEND_MAX_HORIZONS];      // clipped to T', non-decreasing, >= 1
};

__global__ __launch_bounds__(kThreads) void horizon_sse_kernel(HorizonArgs a) {
  __shared__ double snap_s[HODE_BLEND_MAX_HORIZONS][kThreads];
  __shared__ double snap_c[HODE_BLEND_MAX_HORIZONS][kThreads];
  const int tid = threadIdx.x;
  const int pl = tid / a.obs, o = tid - pl * a.obs;
  const long long p0 = (long long)blockIdx.x * a.ppw;
  const long long p = p0 + pl;
  const bool live = pl < a.ppw && p < a.B;
  double acc_s = 0.0, acc_c = 0.0;
  if (live) {
    const long long off = p * a.ps + o;
    int h = 0;
    const int last = a.ends[a.H - 1];
#pragma unroll 4
    for (int t = 0; t < last; ++t) {
      const long long i = t * a.ts + off;
      float pred = a.xe[i];
      if (a.we) pred *= a.we[(long long)t * a.obs + o];
      if (a.xm) {
        const float m = a.xm[i];
        pred = a.wm ? __builtin_fmaf(a.wm[(long long)t * a.obs + o], m, pred) : pred + m;
      }
      const float d = a.truth[i] - pred;
      const float mk = a.mask[i];
      acc_s += (double)(d * d * mk);
      acc_c += (double)mk;
      while (h < a.H && a.ends[h] == t + 1) {
        snap_s[h][tid] = acc_s;
        snap_c[h][tid] = acc_c;
        ++h;
      }
    }
  }
  __syncthreads();
  // thread (h, patient): the patient's components in a fixed order
  if (tid < a.H * a.ppw) {
    const int h = tid / a.ppw, q = tid - h * a.ppw;
    if (p0 + q < a.B) {
      double s = 0.0, c = 0.0;
      for (int k = 0; k < a.obs; ++k) {
        s += snap_s[h][q * a.obs + k];      // q * obs + k < ppw * obs <= kThreads
        c += snap_c[h][q * a.obs + k];
      }
      a.sse[(long long)h * a.B + p0 + q] = (float)s;
      a.cnt[(long long)h * a.B + p0 + q] = (float)c;
    }
  }
}

}  // namespace hode_blend

extern "C" int hode_blend_version(void) { return HODE_BLEND_ABI_VERSION; }

extern "C" const char* hode_blend_last_error_string(void) { return hode_side::g_err; }

extern "C" int hode_blend_nnls2(const hode_blend_nnls2_desc* d, void* stream) {
  using namespace hode_blend;
  if (!d) return fail(HODE_BLEND_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_blend_nnls2_desc))
    return fail(HODE_BLEND_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_blend_nnls2_desc));
  if (d->n_steps <= 0) return fail(HODE_BLEND_E_SIZE, "n_steps %d must be positive", d->n_steps);
  if (d->rows <= 0 || d->rows > 0x7fffffffLL) return fail(HODE_BLEND_E_SIZE, "rows %lld outside 1..2^31-1", (long long)d->rows);
  if (d->step_stride_e < 0 || d->step_stride_m < 0 || d->step_stride_b < 0) return fail(HODE_BLEND_E_SIZE, "negative stride");
  if (!d->x_e || !d->x_m || !d->truth || !d->w) return fail(HODE_BLEND_E_NULL, "x_e / x_m / truth / w is NULL");
  Nnls2Args a{};
  a.xe = d->x_e; a.xm = d->x_m; a.b = d->truth; a.w = d->w;
  a.rows = d->rows; a.se = d->step_stride_e; a.sm = d->step_stride_m; a.sb = d->step_stride_b; a.steps = d->n_steps;
  if (d->rows <= kWaveRows) {
    const int per = kThreads / kWave;
    hipLaunchKernelGGL(nnls2_wave_kernel, dim3((unsigned)((d->n_steps + per - 1) / per)), dim3(kThreads), 0,
                       (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(nnls2_block_kernel, dim3((unsigned)d->n_steps), dim3(kThreads), 0, (hipStream_t)stream, a);
  }
  return launch_fail(hipGetLastError(), "hode_blend_nnls2 launch");
}

extern "C" int hode_blend_horizon_sse(const hode_blend_horizon_desc* d, void* stream) {
  using namespace hode_blend;
  if (!d) return fail(HODE_BLEND_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_blend_horizon_desc))
    return fail(HODE_BLEND_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_blend_horizon_desc));
  if (d->n_times <= 0 || d->batch <= 0) return fail(HODE_BLEND_E_SIZE, "n_times %d / batch %d must be positive", d->n_times, d->batch);
  if (d->obs_dim < 1 || d->obs_dim > HODE_BLEND_MAX_OBS)
    return fail(HODE_BLEND_E_SIZE, "obs_dim %d outside 1..%d", d->obs_dim, HODE_BLEND_MAX_OBS);
  if (d->n_horizons < 1 || d->n_horizons > HODE_BLEND_MAX_HORIZONS)
    return fail(HODE_BLEND_E_SIZE, "n_horizons %d outside 1..%d", d->n_horizons, HODE_BLEND_MAX_HORIZONS);
  if ((long long)d->n_times * d->batch > 0x7fffffffLL) return fail(HODE_BLEND_E_SIZE, "n_times * batch exceeds 2^31");
  if (d->time_stride < 0 || d->patient_stride < 0) return fail(HODE_BLEND_E_SIZE, "negative stride");
  HorizonArgs a{};
  for (int h = 0; h < d->n_horizons; ++h) {
    if (d->horizons[h] < 1 || (h && d->horizons[h] < d->horizons[h - 1]))
      return fail(HODE_BLEND_E_SIZE, "horizons must be >= 1 and non-decreasing (horizons[%d] = %d)", h, d->horizons[h]);
    a.ends[h] = d->horizons[h] < d->n_times ? d->horizons[h] : d->n_times;
  }
  if (!d->x_e || !d->truth || !d->mask || !d->sse || !d->cnt) return fail(HODE_BLEND_E_NULL, "x_e / truth / mask / sse / cnt is NULL");
  if (d->w_m && !d->x_m) return fail(HODE_BLEND_E_NULL, "w_m without x_m");
  a.xe = d->x_e; a.xm = d->x_m; a.we = d->w_e; a.wm = d->w_m; a.truth = d->truth; a.mask = d->mask;
  a.sse = d->sse; a.cnt = d->cnt;
  a.ts = d->time_stride; a.ps = d->patient_stride;
  a.B = d->batch; a.obs = d->obs_dim; a.H = d->n_horizons;
  a.ppw = kThreads / d->obs_dim;     // >= 2 (obs <= 128); ppw * H may exceed kThreads only if obs = 1 and H > 1
  if (a.ppw * a.H > kThreads) a.ppw = kThreads / a.H;
  const long long blocks = ((long long)d->batch + a.ppw - 1) / a.ppw;
  hipLaunchKernelGGL(horizon_sse_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  return launch_fail(hipGetLastError(), "hode_blend_horizon_sse launch");
}
