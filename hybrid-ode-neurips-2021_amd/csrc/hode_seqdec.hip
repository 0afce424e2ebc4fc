// Real-data recurrent baseline decoders (reference DecoderRealBenchmark, model.py:889-966) on the matrix cores, gfx950.
//
//   tlstm : nn.LSTM(2, D) stepped over k = 0 .. T'-1 with h0 = c0 = init and input [a[idx[k]], tau[k]]; h[k] = h_k.
//   gruode: GRUODECell(D) (model.py:865-886).  The reference calls it as `out, (hidden, c) = rnn(obs, (hidden, c))` and the
//           cell returns (dh, (h_all[0], 0)), so the hidden state it is handed is `init` at EVERY step and
//           h[k] = (1 - z[:D]) * (tanh(W_n (z * x_k)) - init), x_k = [init, a[idx[k]], tau[k]], z = sigmoid(W_z x_k).
//           This is what the published numbers ran and it is reproduced as is: there is no recurrence.
//
// Layout (as hode_neural_mf.hip / hode_real_mf.hip): one wave owns 16 patients for the whole time loop, the patients on
// the MFMA N axis.  With v_mfma_f32_16x16x4_f32 (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], C/D
// row 4 (lane >> 4) + reg, column lane & 15), g = lane >> 4 and n = lane & 15 (the patient):
//   * a vector over rows is a set of accumulator tiles: lane (g, n) holds rows 16 j + 4 g + r of tile j in register r;
//   * k-chunk r of a 16-row contraction tile is the rows {4 g + r}, so the B fragment of chunk r IS register r of the tile
//     an earlier product or element-wise step left: no cross-lane traffic in the recurrence;
//   * the weights are gathered once per launch into A fragments in that order and stay in registers;
//   * the input vector is [h or init (D rows), a, tau, 1 (tlstm only: the bias column)], KT = ceil((D + 3) / 16) tiles;
//     the LSTM gate rows are ordered (gate q, hidden tile u) so that i, f, g, o of hidden unit 16 u + 4 g + r sit in the
//     same lane and register: the cell update is lane-local.
// The weight gradients are outer products over the wave's patients, contracted on the matrix cores after a
// patient-major transpose through LDS (OuterAcc); one partial block per wave, folded in a fixed order by seqdec_fold_kernel
// (no float atomics: two identical backward calls are bit-identical).  D is a run-time value, 1 .. HODE_SEQDEC_MAX_LATENT;
// the tile counts (HT hidden tiles, KT input tiles) are compile-time.
#include <hip/hip_runtime.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_host.hpp"

namespace hode {
namespace {

struct SeqArgs {
  const int* __restrict__ idx;    // [T] action row of step k
  const float* __restrict__ tau;  // [T] time feature of step k
  const float* __restrict__ a;    // [Ta][B] (action_dim 1)
  const float* __restrict__ init; // [B][D]
  const float* __restrict__ w0;   // tlstm: weight_ih [4D][2]; gruode: lin_hz [D+2][D+2]
  const float* __restrict__ w1;   // tlstm: weight_hh [4D][D]; gruode: lin_hn [D][D+2]
  const float* __restrict__ b0;   // tlstm: bias_ih [4D]
  const float* __restrict__ b1;   // tlstm: bias_hh [4D]
  float* __restrict__ h;          // [T][B][D]
  float* __restrict__ c;          // tlstm: [T][B][D] cell-state tape (NULL: not written by the forward)
  const float* __restrict__ gh;   // [T][B][D]
  float* __restrict__ ginit;      // [B][D]
  float* __restrict__ partials;   // [n_waves][NP]
  int T, Ta, B, D;
};

HODE_DEV v4 zero4() { return v4{0.f, 0.f, 0.f, 0.f}; }

// rows 16 j + 4 g + r < D of one patient's row vector; the rest 0
HODE_DEV v4 load_tile(const float* __restrict__ src, int j, int g, int D) {
  v4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * j + 4 * g + r;
    v[r] = row < D ? src[row] : 0.f;
  }
  return v;
}
HODE_DEV void store_tile(float* __restrict__ dst, int j, int g, int D, const v4& v, bool live) {
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * j + 4 * g + r;
    if (row < D) dst[row] = v[r];
  }
}

// rows 16 j + 4 g + r < n keep their value, the padding rows become an exact 0.  A select, not a product: a padding row of a
// gate product is 0 * input, which is NaN -- not 0 -- for a patient whose action or state is infinite, and the next
// product would multiply it by a zero-padded weight column (0 * NaN) into every real row of that patient, where the
// reference's gates only saturate (sigmoid -> 0 / 1, tanh -> +-1).  On finite data the padding rows are 0 either way.
HODE_DEV v4 keep_rows(const v4& v, int j, int g, int n) {
  v4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = 16 * j + 4 * g + r < n ? v[r] : 0.f;
  return o;
}

// which registers of the input tiles carry the action (row D), the time feature (row D + 1) and the constant 1 (row D + 2)
template <int KT>
struct InputRows {
  bool ia[KT][4], it[KT][4], i1[KT][4];
  HODE_DEV void init(int g, int D, bool ones) {
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * j + 4 * g + r;
        ia[j][r] = row == D;
        it[j][r] = row == D + 1;
        i1[j][r] = ones && row == D + 2;
      }
  }
  // x = [s (rows < D), a, tau, 1?, 0 ...]; s has zeros past row D - 1
  template <int HT>
  HODE_DEV void fill(v4 (&x)[KT], const v4 (&s)[HT], float av, float tv) const {
#pragma unroll
    for (int j = HT; j < KT; ++j) x[j] = zero4();
#pragma unroll
    for (int j = 0; j < HT; ++j) x[j] = s[j];
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[j][r] = ia[j][r] ? av : (it[j][r] ? tv : (i1[j][r] ? 1.0f : x[j][r]));
  }
};

// out[o] = sum over contraction tiles t and chunks r of A[o][t][r] * in[t][r]  (two partial accumulators per output
// tile: one dependent chain would serialise on the MFMA latency when there are few output tiles)
template <int NO, int NK>
HODE_DEV void mfma_product(const float (&A)[NO][NK][4], const v4 (&in)[NK], v4 (&out)[NO]) {
  v4 p0[NO], p1[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) p0[o] = p1[o] = zero4();
#pragma unroll
  for (int t = 0; t < NK; ++t)
#pragma unroll
    for (int r = 0; r < 4; r += 2)
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        p0[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[o][t][r], in[t][r], p0[o], 0, 0, 0);
        p1[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[o][t][r + 1], in[t][r + 1], p1[o], 0, 0, 0);
      }
#pragma unroll
  for (int o = 0; o < NO; ++o) out[o] = p0[o] + p1[o];
}

// G[a][b] += sum over the wave's 16 patients of U[16 a + i][p] X[16 b + j][p].  The tiles hold [row][patient] with the
// patient in (lane & 15); the contraction runs over PATIENTS, so both operands go through LDS patient-major (16-byte
// stores: a lane's four rows are consecutive) and come back with lane (m, kk) reading image[4 c + kk][16 t + m]: the
// A[m][kk] / B[kk][m] fragments of patient chunk c.
template <int NA, int NB>
struct OuterAcc {
  static constexpr int P = ((16 * (NA + NB) - 16 + 63) / 64) * 64 + 16;  // image pitch == 16 mod 64 (bank spread)
  static constexpr int kLdsFloats = 16 * P;
  static constexpr int NP = NA * NB * 256;  // floats of one wave's partial block: [a * NB + b][lane][4]
  v4 G[NA][NB];
  float* img;
  HODE_DEV void init(float* lds) {
    img = lds;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) G[a][b] = zero4();
  }
  HODE_DEV void add(const v4 (&u)[NA], const v4 (&x)[NB], int g, int n) {
    __syncthreads();  // the previous call's reads are done
#pragma unroll
    for (int a = 0; a < NA; ++a) *reinterpret_cast<v4*>(img + n * P + 16 * a + 4 * g) = u[a];
#pragma unroll
    for (int b = 0; b < NB; ++b) *reinterpret_cast<v4*>(img + n * P + 16 * (NA + b) + 4 * g) = x[b];
    __syncthreads();
    const int m = n, kk = g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* rowp = img + (4 * c + kk) * P + m;
      float ua[NA], xb[NB];
#pragma unroll
      for (int a = 0; a < NA; ++a) ua[a] = rowp[16 * a];
#pragma unroll
      for (int b = 0; b < NB; ++b) xb[b] = rowp[16 * (NA + b)];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) G[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[a], xb[b], G[a][b], 0, 0, 0);
    }
  }
  HODE_DEV void store(float* __restrict__ out, int lane) const {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) *reinterpret_cast<v4*>(out + ((size_t)(a * NB + b) * 64 + lane) * 4) = G[a][b];
  }
};

HODE_DEV int clamp_row(int t, int Ta) { return t < 0 ? 0 : (t >= Ta ? Ta - 1 : t); }

// ================================================================================================================ tlstm
// gate tile t = q * HT + u holds gate q (i, f, g, o) of hidden units 16 u + 4 g + r; PyTorch row q * D + unit
template <int HT, int KT>
struct LstmFrag {
  static constexpr int NG = 4 * HT;
  float W[NG][KT][4];   // gates = W [h, a, tau, 1]:  A[unit row m][input 16 j + 4 g + r]
  HODE_DEV void load(const SeqArgs& s, int g, int m) {
    const int D = s.D;
#pragma unroll
    for (int t = 0; t < NG; ++t)
#pragma unroll
      for (int j = 0; j < KT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int unit = 16 * (t % HT) + m, col = 16 * j + 4 * g + r;
          const size_t row = (size_t)(t / HT) * D + unit;
          float w = 0.f;
          if (unit < D) {
            if (col < D) w = s.w1[row * D + col];
            else if (col == D) w = s.w0[row * 2];
            else if (col == D + 1) w = s.w0[row * 2 + 1];
            else if (col == D + 2) w = s.b0[row] + s.b1[row];
          }
          W[t][j][r] = w;
        }
  }
};

// W_hh^T for the backward: dh_prev = W_hh^T dgates, output tile j (h rows 16 j + m), contraction over the gate tiles
template <int HT>
struct LstmFragT {
  float W[HT][4 * HT][4];
  HODE_DEV void load(const SeqArgs& s, int g, int m) {
    const int D = s.D;
#pragma unroll
    for (int j = 0; j < HT; ++j)
#pragma unroll
      for (int t = 0; t < 4 * HT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int unit = 16 * (t % HT) + 4 * g + r, col = 16 * j + m;
          W[j][t][r] = (unit < D && col < D) ? s.w1[((size_t)(t / HT) * D + unit) * D + col] : 0.f;
        }
  }
};

template <int HT, int KT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void tlstm_fwd_kernel(SeqArgs s) {
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < s.B;
  const int p = live ? pr : s.B - 1;
  const int D = s.D;
  LstmFrag<HT, KT> fw;
  fw.load(s, g, n);
  InputRows<KT> rows;
  rows.init(g, D, true);
  v4 h[HT], c[HT];
#pragma unroll
  for (int u = 0; u < HT; ++u) h[u] = c[u] = load_tile(s.init + (size_t)p * D, u, g, D);
  const size_t step = (size_t)s.B * D;
  float a_nx = s.a[(size_t)clamp_row(s.idx[0], s.Ta) * s.B + p], t_nx = s.tau[0];
  for (int k = 0; k < s.T; ++k) {
    const float av = a_nx, tv = t_nx;
    if (k + 1 < s.T) {  // next step's inputs are independent of the recurrence: issue their loads now
      a_nx = s.a[(size_t)clamp_row(s.idx[k + 1], s.Ta) * s.B + p];
      t_nx = s.tau[k + 1];
    }
    v4 x[KT], z[4 * HT];
    rows.fill(x, h, av, tv);
    mfma_product(fw.W, x, z);
#pragma unroll
    for (int u = 0; u < HT; ++u) {
      const v4 zi = z[u], zf = z[HT + u], zg = z[2 * HT + u], zo = z[3 * HT + u];
      f2 hc[2], cc[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const f2 i = sigmoid2(e ? hi2(zi) : lo2(zi)), f = sigmoid2(e ? hi2(zf) : lo2(zf));
        const f2 gg = tanh_f32(e ? hi2(zg) : lo2(zg)), o = sigmoid2(e ? hi2(zo) : lo2(zo));
        cc[e] = vfma(f, e ? hi2(c[u]) : lo2(c[u]), i * gg);
        hc[e] = o * tanh_f32(cc[e]);
      }
      c[u] = cat4(cc[0], cc[1]);
      h[u] = keep_rows(cat4(hc[0], hc[1]), u, g, D);   // the next step's input: padding rows exactly 0
      store_tile(s.h + k * step + (size_t)p * D, u, g, D, h[u], live);
      if (s.c) store_tile(s.c + k * step + (size_t)p * D, u, g, D, c[u], live);
    }
  }
}

// BPTT.  Step k recomputes its gates from (h[k-1], c[k-1]) (init for k = 0), so only c is taped by the forward.
template <int HT, int KT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void tlstm_bwd_kernel(SeqArgs s) {
  using Acc = OuterAcc<4 * HT, KT>;
  __shared__ __attribute__((aligned(16))) float lds[Acc::kLdsFloats];
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < s.B;
  const int p = live ? pr : s.B - 1;
  const float lv = live ? 1.0f : 0.0f;  // dead lanes carry zero cotangents: they add nothing to the weight gradients
  const int D = s.D;
  LstmFrag<HT, KT> fw;
  fw.load(s, g, n);
  LstmFragT<HT> bw;
  bw.load(s, g, n);
  InputRows<KT> rows;
  rows.init(g, D, true);
  Acc acc;
  acc.init(lds);
  const size_t step = (size_t)s.B * D;
  const float* init = s.init + (size_t)p * D;

  // the operands of step k: h[k-1], c[k-1] (init at k = 0), grad_h[k], a, tau
  struct Fetch {
    v4 hp[HT], cp[HT], gh[HT];
    float av, tv;
  };
  auto fetch = [&](int k, Fetch& f) {
    const float* hs = k > 0 ? s.h + (k - 1) * step + (size_t)p * D : init;
    const float* cs = k > 0 ? s.c + (k - 1) * step + (size_t)p * D : init;
#pragma unroll
    for (int u = 0; u < HT; ++u) {
      f.hp[u] = load_tile(hs, u, g, D);
      f.cp[u] = load_tile(cs, u, g, D);
      f.gh[u] = lv * load_tile(s.gh + k * step + (size_t)p * D, u, g, D);
    }
    f.av = s.a[(size_t)clamp_row(s.idx[k], s.Ta) * s.B + p];
    f.tv = s.tau[k];
  };
  v4 dh[HT], dc[HT];
#pragma unroll
  for (int u = 0; u < HT; ++u) dh[u] = dc[u] = zero4();
  Fetch nx;
  fetch(s.T - 1, nx);
  for (int k = s.T - 1; k >= 0; --k) {
    const Fetch cur = nx;
    if (k > 0) fetch(k - 1, nx);
    v4 x[KT], z[4 * HT], dz[4 * HT];
    rows.fill(x, cur.hp, cur.av, cur.tv);
    mfma_product(fw.W, x, z);
#pragma unroll
    for (int u = 0; u < HT; ++u) {
      const v4 dhu = dh[u] + cur.gh[u];
      f2 dzi[2], dzf[2], dzg[2], dzo[2], dcp[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const f2 i = sigmoid2(e ? hi2(z[u]) : lo2(z[u])), f = sigmoid2(e ? hi2(z[HT + u]) : lo2(z[HT + u]));
        const f2 gg = tanh_f32(e ? hi2(z[2 * HT + u]) : lo2(z[2 * HT + u]));
        const f2 o = sigmoid2(e ? hi2(z[3 * HT + u]) : lo2(z[3 * HT + u]));
        const f2 cp = e ? hi2(cur.cp[u]) : lo2(cur.cp[u]);
        const f2 tc = tanh_f32(vfma(f, cp, i * gg));
        const f2 dhe = e ? hi2(dhu) : lo2(dhu);
        const f2 one = splat2(1.0f);
        const f2 dce = vfma(dhe * o, vfma(-tc, tc, one), e ? hi2(dc[u]) : lo2(dc[u]));
        dzi[e] = (dce * gg) * (i * (one - i));
        dzf[e] = (dce * cp) * (f * (one - f));
        dzg[e] = (dce * i) * vfma(-gg, gg, one);
        dzo[e] = (dhe * tc) * (o * (one - o));
        dcp[e] = dce * f;
      }
      // padding rows exactly 0 (keep_rows): their recomputed gates are 0 * input, and W_hh^T's zero columns would carry a
      // NaN from there into dh of every real unit
      dz[u] = keep_rows(cat4(dzi[0], dzi[1]), u, g, D);
      dz[HT + u] = keep_rows(cat4(dzf[0], dzf[1]), u, g, D);
      dz[2 * HT + u] = keep_rows(cat4(dzg[0], dzg[1]), u, g, D);
      dz[3 * HT + u] = keep_rows(cat4(dzo[0], dzo[1]), u, g, D);
      dc[u] = cat4(dcp[0], dcp[1]);
    }
    mfma_product(bw.W, dz, dh);
    acc.add(dz, x, g, n);  // dW[gate][input] += dz x^T; the ones row collects db (= db_ih = db_hh)
  }
#pragma unroll
  for (int u = 0; u < HT; ++u) store_tile(s.ginit + (size_t)p * D, u, g, D, dh[u] + dc[u], live);  // h0 = c0 = init
  acc.store(s.partials + (size_t)blockIdx.x * Acc::NP, lane);
}

// =============================================================================================================== gruode
template <int HT, int KT>
struct GruFrag {
  float Z[KT][KT][4];   // z = sigmoid(W_z x):   A[row 16 o + m][col 16 j + 4 g + r]
  float N[HT][KT][4];   // n = tanh(W_n (z x))
  float NT[KT][HT][4];  // d(zx) = W_n^T dn':     A[col 16 j + m][row 16 u + 4 g + r]
  float ZT[HT][KT][4];  // dx += W_z^T dz' (rows < D only)
  HODE_DEV void load(const SeqArgs& s, int g, int m) {
    const int D = s.D, K = D + 2;
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * j + 4 * g + r;
#pragma unroll
        for (int o = 0; o < KT; ++o) {
          const int row = 16 * o + m;
          Z[o][j][r] = (row < K && col < K) ? s.w0[(size_t)row * K + col] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < HT; ++u) {
          const int row = 16 * u + m;
          N[u][j][r] = (row < D && col < K) ? s.w1[(size_t)row * K + col] : 0.f;
        }
      }
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int u = 0; u < HT; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * u + 4 * g + r, col = 16 * j + m;
          NT[j][u][r] = (row < D && col < K) ? s.w1[(size_t)row * K + col] : 0.f;
        }
#pragma unroll
    for (int u = 0; u < HT; ++u)
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * t + 4 * g + r, col = 16 * u + m;
          ZT[u][t][r] = (row < K && col < D) ? s.w0[(size_t)row * K + col] : 0.f;
        }
  }
};

template <int HT, int KT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gruode_fwd_kernel(SeqArgs s) {
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < s.B;
  const int p = live ? pr : s.B - 1;
  const int D = s.D;
  GruFrag<HT, KT> fw;
  fw.load(s, g, n);
  InputRows<KT> rows;
  rows.init(g, D, false);
  v4 h0[HT];
#pragma unroll
  for (int u = 0; u < HT; ++u) h0[u] = load_tile(s.init + (size_t)p * D, u, g, D);
  const size_t step = (size_t)s.B * D;
  float a_nx = s.a[(size_t)clamp_row(s.idx[0], s.Ta) * s.B + p], t_nx = s.tau[0];
  for (int k = 0; k < s.T; ++k) {
    const float av = a_nx, tv = t_nx;
    if (k + 1 < s.T) {
      a_nx = s.a[(size_t)clamp_row(s.idx[k + 1], s.Ta) * s.B + p];
      t_nx = s.tau[k + 1];
    }
    v4 x[KT], z[KT], zx[KT], nn[HT];
    rows.fill(x, h0, av, tv);
    mfma_product(fw.Z, x, z);
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      z[j] = sigmoid4(z[j]);
      zx[j] = keep_rows(z[j] * x[j], j, g, D + 2);   // rows past [init, a, tau]: exactly 0, not sigmoid(0 * inf) * 0
    }
    mfma_product(fw.N, zx, nn);
#pragma unroll
    for (int u = 0; u < HT; ++u) {
      const v4 out = (v4{1.f, 1.f, 1.f, 1.f} - z[u]) * (tanh4(nn[u]) - h0[u]);
      store_tile(s.h + k * step + (size_t)p * D, u, g, D, out, live);
    }
  }
}

template <int HT, int KT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gruode_bwd_kernel(SeqArgs s) {
  using AccZ = OuterAcc<KT, KT>;
  using AccN = OuterAcc<HT, KT>;
  __shared__ __attribute__((aligned(16))) float lds[AccZ::kLdsFloats + AccN::kLdsFloats];
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < s.B;
  const int p = live ? pr : s.B - 1;
  const float lv = live ? 1.0f : 0.0f;
  const int D = s.D;
  GruFrag<HT, KT> fw;
  fw.load(s, g, n);
  InputRows<KT> rows;
  rows.init(g, D, false);
  AccZ accz;
  accz.init(lds);
  AccN accn;
  accn.init(lds + AccZ::kLdsFloats);
  v4 h0[HT], gi[HT];
#pragma unroll
  for (int u = 0; u < HT; ++u) {
    h0[u] = load_tile(s.init + (size_t)p * D, u, g, D);
    gi[u] = zero4();
  }
  const v4 one = v4{1.f, 1.f, 1.f, 1.f};
  const size_t step = (size_t)s.B * D;
  struct Fetch {
    v4 gh[HT];
    float av, tv;
  };
  auto fetch = [&](int k, Fetch& f) {
#pragma unroll
    for (int u = 0; u < HT; ++u) f.gh[u] = lv * load_tile(s.gh + k * step + (size_t)p * D, u, g, D);
    f.av = s.a[(size_t)clamp_row(s.idx[k], s.Ta) * s.B + p];
    f.tv = s.tau[k];
  };
  Fetch nx;
  fetch(0, nx);
  for (int k = 0; k < s.T; ++k) {
    const Fetch cur = nx;
    if (k + 1 < s.T) fetch(k + 1, nx);
    v4 x[KT], z[KT], zx[KT], nn[HT], dn[HT], dzx[KT], dz[KT], dx[HT];
    rows.fill(x, h0, cur.av, cur.tv);
    mfma_product(fw.Z, x, z);
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      z[j] = sigmoid4(z[j]);
      zx[j] = z[j] * x[j];
    }
    mfma_product(fw.N, zx, nn);
    // out = (1 - z) (n - init): dn' = g (1 - z) (1 - n^2), dz (direct) = -g (n - init), dinit (direct) = -g (1 - z)
    v4 dzd[HT];
#pragma unroll
    for (int u = 0; u < HT; ++u) {
      const v4 nt = tanh4(nn[u]);
      const v4 gz = cur.gh[u] * (one - z[u]);
      dn[u] = gz * (one - nt * nt);
      dzd[u] = -cur.gh[u] * (nt - h0[u]);
      gi[u] = gi[u] - gz;
    }
    mfma_product(fw.NT, dn, dzx);
#pragma unroll
    for (int j = 0; j < KT; ++j) dz[j] = dzx[j] * x[j];
#pragma unroll
    for (int u = 0; u < HT; ++u) dz[u] = dz[u] + dzd[u];
#pragma unroll
    for (int j = 0; j < KT; ++j) dz[j] = dz[j] * (z[j] * (one - z[j]));  // through the sigmoid
    mfma_product(fw.ZT, dz, dx);
#pragma unroll
    for (int u = 0; u < HT; ++u) gi[u] = gi[u] + dx[u] + dzx[u] * z[u];  // x = [init, ...]: both paths into init
    accz.add(dz, x, g, n);
    accn.add(dn, zx, g, n);
  }
#pragma unroll
  for (int u = 0; u < HT; ++u) store_tile(s.ginit + (size_t)p * D, u, g, D, gi[u], live);
  float* out = s.partials + (size_t)blockIdx.x * (AccZ::NP + AccN::NP);
  accz.store(out, lane);
  accn.store(out + AccZ::NP, lane);
}

// ============================================================================================================== fold
struct FoldOut {
  float *g0, *g1, *gb0, *gb1;  // tlstm: grad w_ih, w_hh, b_ih, b_hh; gruode: grad lin_hz, lin_hn
};

// one wave per slot of the per-wave block: lane l adds waves l, l + 64, ... in order, then a fixed-shape wave sum;
// the summation tree depends only on the wave count, so the result is bit-reproducible.  Every weight entry is exactly
// one slot, so the gradients are written, not accumulated.
template <int KIND, int HT, int KT>
__global__ __launch_bounds__(64) void seqdec_fold_kernel(const float* __restrict__ partials, int n_waves, int D, FoldOut o) {
  constexpr int NPZ = KIND == HODE_SEQDEC_TLSTM ? OuterAcc<4 * HT, KT>::NP : OuterAcc<KT, KT>::NP;
  constexpr int NP = KIND == HODE_SEQDEC_TLSTM ? NPZ : NPZ + OuterAcc<HT, KT>::NP;
  const int j = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int w = lane; w < n_waves; w += 64) s += partials[(size_t)w * NP + j];
  s = wave_sum(s);
  if (lane != 0) return;
  const int jj = j < NPZ ? j : j - NPZ;
  const int tile = jj / 256, l = (jj % 256) / 4, rr = jj % 4;
  const int ri = 4 * (l >> 4) + rr, ci = l & 15;
  const int ta = tile / KT, col = 16 * (tile % KT) + ci;  // B operand (input) row
  if constexpr (KIND == HODE_SEQDEC_TLSTM) {
    const int unit = 16 * (ta % HT) + ri;
    if (unit >= D) return;
    const size_t row = (size_t)(ta / HT) * D + unit;
    if (col < D) o.g1[row * D + col] = s;
    else if (col == D) o.g0[row * 2] = s;
    else if (col == D + 1) o.g0[row * 2 + 1] = s;
    else if (col == D + 2) o.gb0[row] = o.gb1[row] = s;
  } else {
    const int K = D + 2, row = 16 * ta + ri;
    if (col >= K) return;
    if (j < NPZ) {
      if (row < K) o.g0[(size_t)row * K + col] = s;
    } else if (row < D) {
      o.g1[(size_t)row * K + col] = s;
    }
  }
}

template <int HT, int KT>
size_t partial_floats(int kind) {
  return kind == HODE_SEQDEC_TLSTM ? (size_t)OuterAcc<4 * HT, KT>::NP : (size_t)OuterAcc<KT, KT>::NP + OuterAcc<HT, KT>::NP;
}

// tile counts: HT = ceil(D / 16) hidden tiles, KT = ceil((D + 3) / 16) input tiles ([h, a, tau, 1]; gruode has no ones
// row but uses the same split)
int tile_config(int D) { return D <= 13 ? 0 : (D <= 16 ? 1 : 2); }

size_t partial_bytes(const hode_seqdec_desc* d) {
  const size_t nw = ((size_t)d->batch + 15) / 16;
  switch (tile_config(d->latent_dim)) {
    case 0: return nw * partial_floats<1, 1>(d->kind) * sizeof(float);
    case 1: return nw * partial_floats<1, 2>(d->kind) * sizeof(float);
    default: return nw * partial_floats<2, 2>(d->kind) * sizeof(float);
  }
}

template <int HT, int KT>
int launch(const hode_seqdec_desc* d, const SeqArgs& a, bool bwd, hipStream_t st) {
  const dim3 grid((d->batch + 15) / 16), block(64);
  if (d->kind == HODE_SEQDEC_TLSTM) {
    if (bwd) hipLaunchKernelGGL((tlstm_bwd_kernel<HT, KT>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((tlstm_fwd_kernel<HT, KT>), grid, block, 0, st, a);
  } else {
    if (bwd) hipLaunchKernelGGL((gruode_bwd_kernel<HT, KT>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((gruode_fwd_kernel<HT, KT>), grid, block, 0, st, a);
  }
  if (int e = hip_fail(hipGetLastError(), bwd ? "seqdec backward launch" : "seqdec forward launch")) return e;
  if (!bwd) return 0;
  FoldOut o{d->grad_w0, d->grad_w1, d->grad_b0, d->grad_b1};
  const int np = (int)partial_floats<HT, KT>(d->kind);
  if (d->kind == HODE_SEQDEC_TLSTM)
    hipLaunchKernelGGL((seqdec_fold_kernel<HODE_SEQDEC_TLSTM, HT, KT>), dim3(np), block, 0, st, a.partials, (int)grid.x, d->latent_dim, o);
  else
    hipLaunchKernelGGL((seqdec_fold_kernel<HODE_SEQDEC_GRUODE, HT, KT>), dim3(np), block, 0, st, a.partials, (int)grid.x, d->latent_dim, o);
  return hip_fail(hipGetLastError(), "seqdec fold launch");
}

int validate(const hode_seqdec_desc* d, bool bwd) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_seqdec_desc)) return fail(HODE_E_SIZE, "struct_size mismatch (ABI)");
  if (d->kind != HODE_SEQDEC_TLSTM && d->kind != HODE_SEQDEC_GRUODE) return fail(HODE_E_UNSUPPORTED, "unknown seqdec kind %d", d->kind);
  if (d->n_steps <= 0 || d->n_action_times <= 0 || d->batch <= 0)
    return fail(HODE_E_SIZE, "bad sizes n_steps=%d n_action_times=%d batch=%d", d->n_steps, d->n_action_times, d->batch);
  if (d->latent_dim < 1 || d->latent_dim > HODE_SEQDEC_MAX_LATENT)
    return fail(HODE_E_UNSUPPORTED, "seqdec: latent_dim %d outside the compiled tile range 1..%d", d->latent_dim, HODE_SEQDEC_MAX_LATENT);
  if (d->action_dim != 1) return fail(HODE_E_UNSUPPORTED, "seqdec: action_dim %d (only 1 is built)", d->action_dim);
  const bool lstm = d->kind == HODE_SEQDEC_TLSTM;
  if (!d->step_index || !d->step_time || !d->a || !d->init || !d->w0 || !d->w1 || !d->h)
    return fail(HODE_E_NULL, "step_index / step_time / a / init / w0 / w1 / h must be non-NULL");
  if (lstm && (!d->b0 || !d->b1)) return fail(HODE_E_NULL, "tlstm: b0 / b1 must be non-NULL");
  if (!bwd) return 0;
  if (lstm && !d->c) return fail(HODE_E_NULL, "tlstm backward: the cell-state tape c must be non-NULL");
  if (!d->grad_h || !d->grad_init || !d->grad_w0 || !d->grad_w1 || (lstm && (!d->grad_b0 || !d->grad_b1)))
    return fail(HODE_E_NULL, "backward: grad_h / grad_init / grad_w0 / grad_w1 (and grad_b0 / grad_b1 for tlstm) must be non-NULL");
  const size_t need = partial_bytes(d);
  if (!d->workspace || d->workspace_bytes < need) return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  return 0;
}

int run(const hode_seqdec_desc* d, bool bwd, void* stream) {
  if (int e = validate(d, bwd)) return e;
  SeqArgs a{};
  a.idx = d->step_index; a.tau = d->step_time; a.a = d->a; a.init = d->init;
  a.w0 = d->w0; a.w1 = d->w1; a.b0 = d->b0; a.b1 = d->b1;
  a.h = d->h; a.c = d->c; a.gh = d->grad_h; a.ginit = d->grad_init; a.partials = (float*)d->workspace;
  a.T = d->n_steps; a.Ta = d->n_action_times; a.B = d->batch; a.D = d->latent_dim;
  hipStream_t st = (hipStream_t)stream;
  switch (tile_config(d->latent_dim)) {
    case 0: return launch<1, 1>(d, a, bwd, st);
    case 1: return launch<1, 2>(d, a, bwd, st);
    default: return launch<2, 2>(d, a, bwd, st);
  }
}

}  // namespace
}  // namespace hode

extern "C" size_t hode_seqdec_workspace_bytes(const hode_seqdec_desc* d) {
  if (!d || d->struct_size != sizeof(hode_seqdec_desc) || d->batch <= 0 || d->latent_dim < 1 ||
      d->latent_dim > HODE_SEQDEC_MAX_LATENT || (d->kind != HODE_SEQDEC_TLSTM && d->kind != HODE_SEQDEC_GRUODE))
    return 0;
  return hode::partial_bytes(d);
}

extern "C" int hode_seqdec_fwd(const hode_seqdec_desc* d, void* stream) { return hode::run(d, false, stream); }

extern "C" int hode_seqdec_bwd(const hode_seqdec_desc* d, void* stream) { return hode::run(d, true, stream); }
