// The synthetic data generator of the reference's simulation experiments (dataloader.py DataGeneratorRoche.solve and
// generate_data; one scipy LSODA loop per patient there), as three launches (C ABI and arithmetic: include/hode_datagen.h):
//
//  * datagen_solve_kernel<D, NREG>: one patient per lane, one wave per workgroup.  The state and the first NREG of the
//    seven Dormand-Prince stage vectors live in float64 registers, the other stages in LDS ([stage][component][lane], a
//    lane reads only its own column: no bank conflict, no barrier).  D = 20 keeps two stages in registers, every other D
//    all seven.  The adaptive loop is per lane; lanes that have reached the interval end wait masked until the wave
//    reconverges at the grid point.  ml_coef, output_coef and the 13 rate constants are the same for every lane: they are
//    read through uniform addresses (kernel arguments, and scalar loads of the two tables), never replicated per lane.
//    At a grid point a lane writes its latents, forms its obs raw outputs and parks them as float32 in an LDS tile
//    [lane][obs | 1] that aliases the dead stage storage; the wave then walks the tile channel-major: lane c owns channels
//    c and c + 64, adds the patients' values to its float64 sum and sum of squares in lane order and writes the rows
//    with consecutive addresses.  A workgroup's sums go to a workspace row of its own.
//  * datagen_fold_kernel adds the workspace rows in row order and leaves mean and unbiased std per channel.
//  * datagen_finish_kernel z-scores the measurements in place and draws the masks, four consecutive elements per thread.
//
// Deterministic: fixed summation orders, no atomics; the random numbers are a function of (seed, element).
#include <hip/hip_runtime.h>

#include "../../../include/hode_datagen.h"
#include "../hode_side_error.hpp"

namespace hode_datagen {

constexpr int kWave = 64;           // patients per workgroup = lanes of its one wave
constexpr int kFinishThreads = 256;
constexpr int kTileStrideMax = HODE_DATAGEN_MAX_OBS | 1;
constexpr int kTileBytes = kWave * kTileStrideMax * 4;
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kInv32 = 2.3283064365386962890625e-10;  // 2^-32

using hode_side::fail;
using hode_side::launch_fail;

struct Args {
  const double* __restrict__ init;
  const double* __restrict__ dose_times;
  const double* __restrict__ dose_amount;
  const double* __restrict__ ml;
  const double* __restrict__ oc;
  const float* __restrict__ noise;
  float* __restrict__ latents;
  float* __restrict__ actions;
  float* __restrict__ meas;
  float* __restrict__ masks;
  double* __restrict__ noise_out;
  int* __restrict__ status;
  int* __restrict__ steps;
  double* __restrict__ ws;     // [2 * obs] mean, std; then one row [2 * obs] (sum, sum of squares) per workgroup
  double th[HODE_DATAGEN_N_THETA];
  double step, rtol, atol, sigma, p_remove;
  unsigned long long seed;
  int N, T, K, obs, max_steps, blocks;
};

// ---- Philox4x32-10 (Salmon et al., SC'11), hand-written: counter (c0..c3), key (k0, k1)
struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ double normal_at(unsigned long long seed, unsigned t, unsigned n, unsigned o) {
  const U4 r = philox(t, n, o, 0u, (unsigned)seed, (unsigned)(seed >> 32));
  const double u1 = ((double)r.x + 0.5) * kInv32, u2 = ((double)r.y + 0.5) * kInv32;
  return sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
}

__device__ __forceinline__ double uniform_at(unsigned long long seed, unsigned t, unsigned n, unsigned o) {
  const U4 r = philox(t, n, o, 1u, (unsigned)seed, (unsigned)(seed >> 32));
  return ((double)r.x + 0.5) * kInv32;
}

// ---- Dormand-Prince 5(4): row s of kA gives stage s + 1 (row 5 is the 5th-order solution), kE the error weights
__constant__ const double kA[6][6] = {
    {1.0 / 5.0, 0, 0, 0, 0, 0},
    {3.0 / 40.0, 9.0 / 40.0, 0, 0, 0, 0},
    {44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0, 0, 0, 0},
    {19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0, 0, 0},
    {9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0, 0},
    {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0}};
__constant__ const double kC[6] = {1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0};
__constant__ const double kE[7] = {71.0 / 57600.0, 0.0, -71.0 / 16695.0, 71.0 / 1920.0, -17253.0 / 339200.0, 22.0 / 525.0,
                                   -1.0 / 40.0};

// A table every lane reads at the same address (ml_coef, output_coef), seen through the constant address space: the loads
// become scalar loads and the products take the value from scalar registers, so no lane holds a copy of its own.
typedef const double __attribute__((address_space(4))) * UniformTable;
__device__ __forceinline__ UniformTable uniform_table(const double* p) {
  return reinterpret_cast<UniformTable>(reinterpret_cast<uintptr_t>(p));
}

struct Rates {  // the 13 constants by name, plus what does not change over a call
  double hc, hp, ec50, emax, kdexa, kcir, kci, kprog, kid, kfb, koff, kim, kel, ecp;
  bool hill2;
};

// the generator's right-hand side (dataloader.py:105-149) at state Y with Dose(t) = dose
template <int D>
__device__ __forceinline__ void rhs(const Rates& r, UniformTable ml, double dose, const double (&Y)[D],
                                    double (&k)[D]) {
  constexpr int M = D - 4;
  const double dis = Y[0], ir = Y[1], imm = Y[2], d2 = Y[3];
  double immp, irp;
  if (r.hill2) { immp = imm * imm; irp = ir * ir; }   // both exponents 2: every shipped configuration
  else { immp = pow(imm, r.hc); irp = pow(ir, r.hp); }
  k[0] = dis * r.kprog - dis * immp * r.kci - dis * ir * r.kcir;
  k[1] = dis * r.kid - ir * r.koff + dis * ir * r.kfb + (irp * r.emax) / (r.ecp + irp) - d2 * ir * r.kdexa;
  k[2] = ir * r.kim;
  k[3] = r.kel * dose - r.kel * d2;
  if constexpr (M > 0) {
    double z[M];
#pragma unroll
    for (int j = 0; j < M; ++j) z[j] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) z[j] = __builtin_fma(Y[i], ml[i * M + j], z[j]);   // ml: uniform address
#pragma unroll
    for (int j = 0; j < M; ++j) k[4 + j] = tanh(z[j]);
  }
}

template <int D>
__device__ __forceinline__ bool all_finite(const double (&v)[D]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < D; ++i) ok = ok && (__builtin_fabs(v[i]) <= 1.7976931348623157e308);
  return ok;
}

template <int D, int NREG>
__global__ __launch_bounds__(kWave) void datagen_solve_kernel(Args a) {
  constexpr int NL = 7 - NREG;                       // stages kept in LDS
  constexpr int kStageBytes = NL * D * kWave * 8;
  constexpr int kBytes = kStageBytes > kTileBytes ? kStageBytes : kTileBytes;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
  double* const kl = reinterpret_cast<double*>(smem);
  float* const tile = reinterpret_cast<float*>(smem);

  const int lane = threadIdx.x;
  const long long n0 = (long long)blockIdx.x * kWave;
  const long long n = n0 + lane;
  const bool live = n < a.N;
  const int nl = (a.N - n0) < kWave ? (int)(a.N - n0) : kWave;   // patients of this workgroup
  const int stride = a.obs | 1;

  Rates r;
  r.hc = a.th[0]; r.hp = a.th[1]; r.ec50 = a.th[2]; r.emax = a.th[3]; r.kdexa = a.th[4]; r.kcir = a.th[5]; r.kci = a.th[6];
  r.kprog = a.th[7]; r.kid = a.th[8]; r.kfb = a.th[9]; r.koff = a.th[10]; r.kim = a.th[11]; r.kel = a.th[12];
  r.hill2 = (r.hc == 2.0 && r.hp == 2.0);
  r.ecp = r.hill2 ? r.ec50 * r.ec50 : pow(r.ec50, r.hp);

  double y[D];
#pragma unroll
  for (int i = 0; i < D; ++i) y[i] = live ? a.init[n * D + i] : 0.0;
  const double amount = live ? a.dose_amount[n] : 0.0;
  const double* __restrict__ taus = a.dose_times + (live ? n : 0) * a.K;

  const UniformTable ml = uniform_table(a.ml), oc = uniform_table(a.oc);

  double kr[NREG][D];
  auto getk = [&](int s, int i) -> double { return s < NREG ? kr[s < NREG ? s : 0][i] : kl[((s - NREG) * D + i) * kWave + lane]; };
  auto setk = [&](int s, int i, double v) {
    if (s < NREG) kr[s < NREG ? s : 0][i] = v;
    else kl[((s - NREG) * D + i) * kWave + lane] = v;
  };

  bool alive = live && all_finite<D>(y);
  int stop = (live && !alive) ? -1 : 0;
  int nsteps = 0;
  double h = 0.0;
  double sum[2] = {0.0, 0.0}, sq[2] = {0.0, 0.0};

  for (int gi = 0; gi < a.T; ++gi) {
    // ------------------------------------------------------------------ advance the lane's patient to grid point gi
    if (gi > 0 && alive) {
      const double t_end = gi * a.step;
      double t = (gi - 1) * a.step;
      int tries = 0;
      bool ok = true;
      while (ok && t < t_end) {
        // one smooth piece [t, nxt]: up to the next dose strictly inside the interval, with the doses given by t active
        double nxt = t_end, amp = 0.0;
        for (int k = 0; k < a.K; ++k) {
          const double tau = taus[k];
          if (tau > t && tau < nxt) nxt = tau;
          if (tau <= t) amp += exp(r.kel * (tau - t));
        }
        amp *= amount;                                  // Dose(s) = amp exp(-kel (s - t0)) on the piece
        const double t0 = t;
        {
          double k1[D];
          rhs<D>(r, ml, amp, y, k1);
#pragma unroll
          for (int i = 0; i < D; ++i) setk(0, i, k1[i]);
          if (h == 0.0) {                               // first step of the patient: h = 0.01 |y| / |f|, scaled norms
            double d0 = 0.0, d1 = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
              const double sc = a.atol + a.rtol * __builtin_fabs(y[i]);
              d0 += (y[i] / sc) * (y[i] / sc);
              d1 += (k1[i] / sc) * (k1[i] / sc);
            }
            h = (d0 > 1e-10 * D && d1 > 1e-10 * D) ? 0.01 * sqrt(d0 / d1) : 1e-6;
            if (!(h <= a.step)) h = a.step;
          }
        }
        while (t < nxt) {
          if (tries >= a.max_steps) { ok = false; break; }
          ++tries;
          double hs = h;
          bool last = false;
          if (t + 1.01 * hs >= nxt) { hs = nxt - t; last = true; }
          if (!(t + hs > t)) { ok = false; break; }     // the step no longer moves t
          double yn[D];
#pragma unroll
          for (int s = 0; s < 6; ++s) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
              double acc = 0.0;
#pragma unroll
              for (int j = 0; j <= s; ++j)
                if (kA[s][j] != 0.0) acc = __builtin_fma(kA[s][j], getk(j, i), acc);
              yn[i] = __builtin_fma(hs, acc, y[i]);
            }
            const double ts = (s >= 4) ? (last ? nxt : t + hs) : t + kC[s] * hs;
            double ks[D];
            rhs<D>(r, ml, amp * exp(-r.kel * (ts - t0)), yn, ks);
#pragma unroll
            for (int i = 0; i < D; ++i) setk(s + 1, i, ks[i]);
          }
          // yn is the 5th-order solution and stage 6 its derivative; RMS of the embedded error estimate
          double e2 = 0.0;
#pragma unroll
          for (int i = 0; i < D; ++i) {
            double e = 0.0;
#pragma unroll
            for (int s = 0; s < 7; ++s)
              if (kE[s] != 0.0) e = __builtin_fma(kE[s], getk(s, i), e);
            const double ay = __builtin_fabs(y[i]), an = __builtin_fabs(yn[i]);
            const double q = hs * e / (a.atol + a.rtol * (ay > an ? ay : an));
            e2 = __builtin_fma(q, q, e2);
          }
          const double err = sqrt(e2 / D);
          const bool accept = (err <= 1.0) && all_finite<D>(yn);
          double factor;
          if (err == 0.0) factor = 10.0;
          else if (err < 1e300) {                        // finite and positive
            factor = 0.9 * exp(-0.2 * log(err));
            factor = factor > 10.0 ? 10.0 : (factor < 0.2 ? 0.2 : factor);
          } else factor = 0.2;
          if (accept) {
            t = last ? nxt : t + hs;
#pragma unroll
            for (int i = 0; i < D; ++i) { y[i] = yn[i]; setk(0, i, getk(6, i)); }   // FSAL
            const double hn = hs * factor;
            h = (last && hn < h) ? h : hn;               // a step clipped to the piece end does not shrink the carried h
          } else {
            h = hs * (factor < 1.0 ? factor : 0.9);
          }
        }
      }
      nsteps += tries;
      if (!ok) { alive = false; stop = gi; }
    }
    // ------------------------------------------------------------------ grid point gi: the lane's rows
    const double tg = gi * a.step;
    const long long row = (long long)gi * a.N + n;
    if (live) {
#pragma unroll
      for (int i = 0; i < D; ++i) a.latents[row * D + i] = alive ? (float)y[i] : 0.0f;
      bool hit = false;
      for (int k = 0; k < a.K; ++k) hit = hit || (taus[k] == tg);
      a.actions[row] = (alive && hit) ? (float)amount : 0.0f;
    }
    __syncthreads();                                     // the stage columns are dead: the tile may overwrite them
    for (int o = 0; o < a.obs; ++o) {
      const UniformTable c = oc + o * (D + 1);
      double v = c[D];
#pragma unroll
      for (int i = 0; i < D; ++i) v = __builtin_fma(c[i], y[i], v);
      double eps = 0.0;
      if (live) {
        eps = a.noise ? (double)a.noise[row * a.obs + o] : normal_at(a.seed, (unsigned)gi, (unsigned)n, (unsigned)o);
        if (a.noise_out) a.noise_out[row * a.obs + o] = eps;
      }
      tile[lane * stride + o] = alive ? (float)(v + a.sigma * eps) : 0.0f;
    }
    __syncthreads();
    // channel-major walk: lane c owns channels c and c + 64; patients in lane order
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int o = lane + half * kWave;
      if (o < a.obs) {
        float* __restrict__ out = a.meas + ((long long)gi * a.N + n0) * a.obs + o;
        for (int l = 0; l < nl; ++l) {
          const float v = tile[l * stride + o];
          out[(long long)l * a.obs] = v;
          sum[half] += (double)v;
          sq[half] = __builtin_fma((double)v, (double)v, sq[half]);
        }
      }
    }
    __syncthreads();                                     // the tile is read: the stages may overwrite it
  }
  if (live) {
    a.status[n] = stop;
    if (a.steps) a.steps[n] = nsteps;
  }
  double* __restrict__ wrow = a.ws + 2LL * a.obs * (1 + (long long)blockIdx.x);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int o = lane + half * kWave;
    if (o < a.obs) { wrow[o] = sum[half]; wrow[a.obs + o] = sq[half]; }
  }
}

// thread j < 2 * obs adds column j of the workgroup rows in row order; then mean and unbiased std (torch.std) per channel
__global__ __launch_bounds__(2 * HODE_DATAGEN_MAX_OBS) void datagen_fold_kernel(Args a) {
  __shared__ double tot[2 * HODE_DATAGEN_MAX_OBS];
  const int j = threadIdx.x;
  if (j < 2 * a.obs) {
    double s = 0.0;
    const double* __restrict__ p = a.ws + 2 * a.obs + j;
    for (int b = 0; b < a.blocks; ++b) s += p[2LL * a.obs * b];
    tot[j] = s;
  }
  __syncthreads();
  if (j < a.obs) {
    const double cnt = (double)a.T * (double)a.N;
    const double mean = tot[j] / cnt;
    const double var = (tot[a.obs + j] - tot[j] * mean) / (cnt - 1.0);
    a.ws[j] = mean;
    a.ws[a.obs + j] = sqrt(var > 0.0 ? var : 0.0);
  }
}

// four consecutive elements of the contiguous (T * N * obs) range per thread
__global__ __launch_bounds__(kFinishThreads) void datagen_finish_kernel(Args a, long long total, int vec) {
  const long long base = ((long long)blockIdx.x * kFinishThreads + threadIdx.x) * 4;
  if (base >= total) return;
  const int cnt = (total - base) < 4 ? (int)(total - base) : 4;
  float m[4], k[4];
  if (vec && cnt == 4) {
    const float4 v = *reinterpret_cast<const float4*>(a.meas + base);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
  } else {
    for (int e = 0; e < cnt; ++e) m[e] = a.meas[base + e];
  }
  long long rown = base / a.obs;                 // t * N + n
  int o = (int)(base - rown * a.obs);
  int t = (int)(rown / a.N);
  int n = (int)(rown - (long long)t * a.N);
  int st = a.status[n];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < cnt) {
      const bool alive = st == 0 || (st > 0 && t < st);
      const double u = uniform_at(a.seed, (unsigned)t, (unsigned)n, (unsigned)o);
      m[e] = alive ? (float)(((double)m[e] - a.ws[o]) / a.ws[a.obs + o]) : 0.0f;
      k[e] = (alive && u > a.p_remove) ? 1.0f : 0.0f;
      if (++o == a.obs) {
        o = 0;
        if (++n == a.N) { n = 0; ++t; }
        st = a.status[n];
      }
    }
  }
  if (vec && cnt == 4) {
    *reinterpret_cast<float4*>(a.meas + base) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(a.masks + base) = make_float4(k[0], k[1], k[2], k[3]);
  } else {
    for (int e = 0; e < cnt; ++e) { a.meas[base + e] = m[e]; a.masks[base + e] = k[e]; }
  }
}

template <int D, int NREG>
void launch_solve(const Args& a, hipStream_t s) {
  hipLaunchKernelGGL((datagen_solve_kernel<D, NREG>), dim3((unsigned)a.blocks), dim3(kWave), 0, s, a);
}

bool sizes_ok(long long N, long long obs) { return N >= 1 && N <= 0x7fffffffLL && obs >= 1 && obs <= HODE_DATAGEN_MAX_OBS; }

}  // namespace hode_datagen

extern "C" int hode_datagen_version(void) { return HODE_DATAGEN_ABI_VERSION; }

extern "C" const char* hode_datagen_last_error_string(void) { return hode_side::g_err; }

extern "C" uint64_t hode_datagen_workspace_bytes(int32_t n_patients, int32_t obs_dim) {
  using namespace hode_datagen;
  if (!sizes_ok(n_patients, obs_dim)) return 0;
  const uint64_t blocks = ((uint64_t)n_patients + kWave - 1) / kWave;
  return 2ull * (uint64_t)obs_dim * (1 + blocks) * sizeof(double);
}

extern "C" int hode_datagen_generate(const hode_datagen_desc* d, void* stream) {
  using namespace hode_datagen;
  if (!d) return fail(HODE_DATAGEN_E_NULL, "desc is NULL");
  if (d->struct_size != sizeof(hode_datagen_desc))
    return fail(HODE_DATAGEN_E_SIZE, "struct_size %u != %zu", d->struct_size, sizeof(hode_datagen_desc));
  if (d->flags != 0) return fail(HODE_DATAGEN_E_UNSUPPORTED, "flags 0x%x: none is defined", d->flags);
  const int D = d->latent_dim;
  if (D != 4 && D != 6 && D != 8 && D != 12 && D != 20)
    return fail(HODE_DATAGEN_E_UNSUPPORTED, "latent_dim %d has no compiled kernel (4, 6, 8, 12, 20)", D);
  if (d->obs_dim < 1 || d->obs_dim > HODE_DATAGEN_MAX_OBS)
    return fail(HODE_DATAGEN_E_SIZE, "obs_dim %d outside 1..%d", d->obs_dim, HODE_DATAGEN_MAX_OBS);
  if (d->n_dose < 1 || d->n_dose > HODE_DATAGEN_MAX_DOSES)
    return fail(HODE_DATAGEN_E_SIZE, "n_dose %d outside 1..%d", d->n_dose, HODE_DATAGEN_MAX_DOSES);
  if (d->n_times < 2) return fail(HODE_DATAGEN_E_SIZE, "n_times %d must be at least 2", d->n_times);
  if (d->n_patients < 1) return fail(HODE_DATAGEN_E_SIZE, "n_patients %d must be positive", d->n_patients);
  if ((long long)d->n_times * d->n_patients > 0x7fffffffLL) return fail(HODE_DATAGEN_E_SIZE, "n_times * n_patients exceeds 2^31");
  if (d->max_steps < 1) return fail(HODE_DATAGEN_E_SIZE, "max_steps %d must be positive", d->max_steps);
  if (!(d->step > 0.0)) return fail(HODE_DATAGEN_E_SIZE, "step %g must be positive", d->step);
  if (!(d->rtol >= 0.0) || !(d->atol >= 0.0) || !(d->rtol + d->atol > 0.0))
    return fail(HODE_DATAGEN_E_SIZE, "rtol %g / atol %g must be non-negative and not both zero", d->rtol, d->atol);
  if (!d->init || !d->dose_times || !d->dose_amount || !d->output_coef || (D > 4 && !d->ml_coef))
    return fail(HODE_DATAGEN_E_NULL, "init / dose_times / dose_amount / output_coef / ml_coef is NULL");
  if (!d->latents || !d->actions || !d->measurements || !d->masks || !d->status || !d->workspace)
    return fail(HODE_DATAGEN_E_NULL, "latents / actions / measurements / masks / status / workspace is NULL");
  const uint64_t need = hode_datagen_workspace_bytes(d->n_patients, d->obs_dim);
  if (d->workspace_bytes < need)
    return fail(HODE_DATAGEN_E_SIZE, "workspace_bytes %llu < %llu", (unsigned long long)d->workspace_bytes, (unsigned long long)need);
  if ((uintptr_t)d->workspace % 8) return fail(HODE_DATAGEN_E_SIZE, "workspace is not 8-byte aligned");

  Args a{};
  a.init = d->init; a.dose_times = d->dose_times; a.dose_amount = d->dose_amount; a.ml = d->ml_coef; a.oc = d->output_coef;
  a.noise = d->noise; a.latents = d->latents; a.actions = d->actions; a.meas = d->measurements; a.masks = d->masks;
  a.noise_out = d->noise_out; a.status = d->status; a.steps = d->steps; a.ws = static_cast<double*>(d->workspace);
  for (int i = 0; i < HODE_DATAGEN_N_THETA; ++i) a.th[i] = d->theta[i];
  a.step = d->step; a.rtol = d->rtol; a.atol = d->atol; a.sigma = d->sigma; a.p_remove = d->p_remove; a.seed = d->seed;
  a.N = d->n_patients; a.T = d->n_times; a.K = d->n_dose; a.obs = d->obs_dim; a.max_steps = d->max_steps;
  a.blocks = (d->n_patients + kWave - 1) / kWave;
  hipStream_t s = (hipStream_t)stream;
  switch (D) {
    case 4: launch_solve<4, 7>(a, s); break;
    case 6: launch_solve<6, 7>(a, s); break;
    case 8: launch_solve<8, 7>(a, s); break;
    case 12: launch_solve<12, 7>(a, s); break;
    default: launch_solve<20, 2>(a, s); break;
  }
  int rc = launch_fail(hipGetLastError(), "datagen_solve_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(datagen_fold_kernel, dim3(1), dim3(2 * HODE_DATAGEN_MAX_OBS), 0, s, a);
  rc = launch_fail(hipGetLastError(), "datagen_fold_kernel launch");
  if (rc) return rc;
  const long long total = (long long)a.T * a.N * a.obs;
  const long long threads = (total + 3) / 4;
  const int vec = ((uintptr_t)d->measurements % 16 == 0 && (uintptr_t)d->masks % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(datagen_finish_kernel, dim3((unsigned)((threads + kFinishThreads - 1) / kFinishThreads)),
                     dim3(kFinishThreads), 0, s, a, total, vec);
  return launch_fail(hipGetLastError(), "datagen_finish_kernel launch");
}
