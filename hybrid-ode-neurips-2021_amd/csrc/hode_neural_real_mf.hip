// Neural ODE baselines of the real-data experiment on the matrix cores (reference NeuralODEReal / NeuralODEReal2nd,
// model.py:660-769), gfx950:
//   HODE_RHS_NEURAL_REAL     : dy/dt = m([y, dose])                       m = tanh(W2 tanh(W1 . + b1) + b2), Dm = D
//   HODE_RHS_NEURAL_REAL_2ND : dy/dt = [m([y, dose]), y[:D/2]]                                              Dm = D / 2
// inside the fixed-grid euler / midpoint / rk4(3/8) loop and its discrete adjoint.  The dose input of every
// (interval, stage) comes from a host-gathered table (desc->dosage = [T-1][stages][B]), so the torchdiffeq stage-time
// semantics (perturb, int(t), the >= Ta zero branch) stay on the host (hode/neural_real.py::stage_rows).
//
// The recipe of hode_neural_mf.hip extended to several tiles: a wave owns 16 patients for the whole grid; with
// v_mfma_f32_16x16x4_f32 and g = lane >> 4, n = lane & 15 (the patient) a vector over 16 "positions" is one accumulator
// tile (lane (g, n) holds positions 4g + r in register r) and k-chunk r of every product is register r of the tile the
// previous step left -- no cross-lane traffic in the loop.  Vectors longer than 16 are several tiles:
//   ST state tiles, IT >= ST input tiles ([y, dose] plus, in the weight-gradient products, a ones row), HT hidden tiles,
//   OT output tiles of m.
// Position layout (NrLayout): `neural` keeps y at positions 0..D-1, then dose, then the ones row.  `2nd` pads each half
// of the state to its own QT = ceil(D/32) tiles -- y1 at 0.., y2 at 16 QT.., dose and ones behind y2 -- so the
// passthrough y1 -> dy2/dt is a copy of whole tiles and m's output tiles line up with y1's.
// The four weight operands (W1, W2 scaled by 2 log2(e) for the exp2-based tanh; W2^T, W1^T unscaled) are gathered into
// fragment order once per launch and stay in registers.  The backward recomputes the stages of each step from h[n],
// runs the VJPs and accumulates the weight gradients on the matrix cores (outer products over the wave's 16 patients,
// operands transposed through LDS as in NeuralGradAcc); one partial block per wave, folded in a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_host.hpp"
#include "hode_neural_args.hpp"
#include "hode_neural_mf.hpp"

namespace hode {

namespace {

struct NrArgs {
  const float* __restrict__ t;     // [T] grid
  const float* __restrict__ y0;    // [B][D]
  const float* __restrict__ dose;  // [T-1][S][B]
  const float* __restrict__ w1;    // [H][D+1]
  const float* __restrict__ b1;    // [H]
  const float* __restrict__ w2;    // [Dm][H]
  const float* __restrict__ b2;    // [Dm]
  float* __restrict__ h;           // [T][B][D]
  const float* __restrict__ grad_h;
  float* __restrict__ grad_y0;
  float* __restrict__ partials;    // [n_waves][NP]
  int B, T, D, H, kind;
};

// positions of [y, dose, 1] inside the stacked tiles (see the top of the file)
struct NrLayout {
  int D, n1, off2, n2, pdose;
  __host__ __device__ NrLayout(int kind, int D_) : D(D_) {
    if (kind == HODE_RHS_NEURAL_REAL_2ND) {
      n1 = n2 = D / 2;
      off2 = 16 * ((n1 + 15) / 16);
    } else {
      n1 = D;
      n2 = 0;
      off2 = D;
    }
    pdose = off2 + n2;
  }
  // logical column of W1 at position pos: 0..D-1 state, D dose, D+1 the ones row (bias), -1 padding
  __host__ __device__ int col(int pos) const {
    if (pos < n1) return pos;
    if (pos >= off2 && pos - off2 < n2) return n1 + (pos - off2);
    if (pos == pdose) return D;
    if (pos == pdose + 1) return D + 1;
    return -1;
  }
};

// step size of interval n.  t0 goes through a VGPR first: with both grid values in SGPRs the compiler has emitted a
// v_sub with two constant-bus operands, which gfx9 does not have
HODE_DEV float nr_dt(const float* __restrict__ t, int n) {
  float t0;
  asm volatile("v_mov_b32 %0, %1" : "=v"(t0) : "s"(t[n]));
  return t[n + 1] - t0;
}

constexpr int kNrStages(int method) { return method == HODE_METHOD_EULER ? 1 : (method == HODE_METHOD_MIDPOINT ? 2 : 4); }

// a vector of N tiles
template <int N>
struct Tv {
  v4 t[N];
  HODE_DEV Tv operator+(const Tv& o) const {
    Tv r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.t[i] = t[i] + o.t[i];
    return r;
  }
  HODE_DEV Tv operator-(const Tv& o) const {
    Tv r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.t[i] = t[i] - o.t[i];
    return r;
  }
  HODE_DEV Tv operator*(float s) const {
    Tv r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.t[i] = t[i] * s;
    return r;
  }
  friend HODE_DEV Tv operator*(float s, const Tv& a) { return a * s; }
};

// per-lane bit masks (bit 4c + r) of the two scalar positions (dose, ones) inside the input tiles
template <int IT>
struct NrSlots {
  uint32_t dose, one;
  HODE_DEV NrSlots(const NrLayout& L, int g) : dose(0), one(0) {
#pragma unroll
    for (int c = 0; c < IT; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pos = 16 * c + 4 * g + r;
        dose |= (pos == L.pdose ? 1u : 0u) << (4 * c + r);
        one |= (pos == L.pdose + 1 ? 1u : 0u) << (4 * c + r);
      }
  }
  HODE_DEV bool is_dose(int c, int r) const { return (dose >> (4 * c + r)) & 1u; }
  HODE_DEV bool is_one(int c, int r) const { return (one >> (4 * c + r)) & 1u; }
};

template <int KIND, int ST, int IT, int HT>
struct NrNet {
  static constexpr int OT = KIND == HODE_RHS_NEURAL_REAL_2ND ? ST / 2 : ST;
  static constexpr int NZ = OT == 1 ? 4 : 2;                  // partial accumulators per output tile (MFMA latency)
  static constexpr int NG = ST == 1 ? 4 : (ST == 2 ? 2 : 1);  // ... per input-cotangent tile
  static constexpr float kS = NeuralMf<4>::kTanhScale;
  float A1[HT][IT][4];  // kS W1[16i + m][col(16c + 4g + r)]
  float A2[OT][HT][4];  // kS W2[16o + m][16i + 4g + r]
  float A3[HT][OT][4];  // W2[16o + 4g + r][16i + m]        (W2^T)
  float A4[ST][HT][4];  // W1[16i + 4g + r][col(16c + m)]   (W1^T, state columns only)
  v4 bias1[HT], bias2[OT];

  HODE_DEV void load(const NrArgs& a, const NrLayout& L, int lane) {
    const int g = lane >> 4, m = lane & 15;
    const int D = a.D, H = a.H, Dm = KIND == HODE_RHS_NEURAL_REAL_2ND ? a.D / 2 : a.D;
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int hrow = 16 * i + m, hk = 16 * i + 4 * g + r;
#pragma unroll
        for (int c = 0; c < IT; ++c) {
          const int cc = L.col(16 * c + 4 * g + r);
          A1[i][c][r] = (hrow < H && cc >= 0 && cc <= D) ? kS * a.w1[(size_t)hrow * (D + 1) + cc] : 0.f;
        }
#pragma unroll
        for (int o = 0; o < OT; ++o) {
          A2[o][i][r] = (16 * o + m < Dm && hk < H) ? kS * a.w2[(size_t)(16 * o + m) * H + hk] : 0.f;
          A3[i][o][r] = (hrow < H && 16 * o + 4 * g + r < Dm) ? a.w2[(size_t)(16 * o + 4 * g + r) * H + hrow] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < ST; ++c) {
          const int cc = L.col(16 * c + m);
          A4[c][i][r] = (cc >= 0 && cc < D && hk < H) ? a.w1[(size_t)hk * (D + 1) + cc] : 0.f;
        }
        bias1[i][r] = hk < H ? kS * a.b1[hk] : 0.f;
      }
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) bias2[o][r] = (16 * o + 4 * g + r) < Dm ? kS * a.b2[16 * o + 4 * g + r] : 0.f;
  }

  HODE_DEV void hidden(const Tv<IT>& e, v4 (&a1)[HT]) const {
    v4 acc[HT];
#pragma unroll
    for (int i = 0; i < HT; ++i) acc[i] = bias1[i];
#pragma unroll
    for (int c = 0; c < IT; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < HT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[i][c][r], e.t[c][r], acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < HT; ++i) a1[i] = NeuralMf<4>::tanh_scaled(acc[i]);
  }

  // m(e) (OT tiles); a1 is left for the caller
  HODE_DEV Tv<OT> mlp(const Tv<IT>& e, v4 (&a1)[HT]) const {
    hidden(e, a1);
    v4 z[OT][NZ];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      z[o][0] = bias2[o];
#pragma unroll
      for (int q = 1; q < NZ; ++q) z[o][q] = splat4(0.f);
    }
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 0; o < OT; ++o)
          z[o][(4 * i + r) % NZ] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[o][i][r], a1[i][r], z[o][(4 * i + r) % NZ], 0, 0, 0);
    Tv<OT> k;
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      v4 s = z[o][0];
#pragma unroll
      for (int q = 1; q < NZ; ++q) s = s + z[o][q];
      k.t[o] = NeuralMf<4>::tanh_scaled(s);
    }
    return k;
  }

  // dy/dt in state layout from the stage input e and m's output k
  HODE_DEV static Tv<ST> deriv(const Tv<IT>& e, const Tv<OT>& k) {
    Tv<ST> f;
#pragma unroll
    for (int c = 0; c < ST; ++c) {
      if constexpr (KIND == HODE_RHS_NEURAL_REAL_2ND) f.t[c] = c < OT ? k.t[c < OT ? c : 0] : e.t[c < OT ? 0 : c - OT];  // dy2/dt = y1
      else f.t[c] = k.t[c < OT ? c : 0];
    }
    return f;
  }

  // VJP at a stage (input e, activations a1, output k) for the cotangent gf of dy/dt: returns the state cotangent;
  // u2 / u1 are the pre-activation cotangents of the two layers (weight-gradient operands)
  HODE_DEV Tv<ST> vjp(const v4 (&a1)[HT], const Tv<OT>& k, const Tv<ST>& gf, v4 (&u2)[OT], v4 (&u1)[HT]) const {
#pragma unroll
    for (int o = 0; o < OT; ++o) u2[o] = gf.t[o] * __builtin_elementwise_fma(-k.t[o], k.t[o], splat4(1.0f));
    v4 acc[HT];
#pragma unroll
    for (int i = 0; i < HT; ++i) acc[i] = splat4(0.f);
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < HT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[i][o][r], u2[o][r], acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < HT; ++i) u1[i] = acc[i] * __builtin_elementwise_fma(-a1[i], a1[i], splat4(1.0f));
    v4 z[ST][NG];
#pragma unroll
    for (int c = 0; c < ST; ++c)
#pragma unroll
      for (int q = 0; q < NG; ++q) z[c][q] = splat4(0.f);
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < ST; ++c)
          z[c][(4 * i + r) % NG] = __builtin_amdgcn_mfma_f32_16x16x4f32(A4[c][i][r], u1[i][r], z[c][(4 * i + r) % NG], 0, 0, 0);
    Tv<ST> ge;
#pragma unroll
    for (int c = 0; c < ST; ++c) {
      v4 s = z[c][0];
#pragma unroll
      for (int q = 1; q < NG; ++q) s = s + z[c][q];
      ge.t[c] = s;
    }
    if constexpr (KIND == HODE_RHS_NEURAL_REAL_2ND) {
#pragma unroll
      for (int c = 0; c < OT; ++c) ge.t[c] = ge.t[c] + gf.t[c + OT];  // the passthrough y1 -> dy2/dt
    }
    return ge;
  }
};

// stage input: the state tiles plus the dose at its position
template <int ST, int IT>
HODE_DEV Tv<IT> nr_input(const Tv<ST>& y, float dose, const NrSlots<IT>& sl) {
  Tv<IT> e;
#pragma unroll
  for (int c = 0; c < IT; ++c) {
    e.t[c] = c < ST ? y.t[c < ST ? c : 0] : splat4(0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) e.t[c][r] = sl.is_dose(c, r) ? dose : e.t[c][r];
  }
  return e;
}

template <int ST>
HODE_DEV Tv<ST> nr_load_state(const float* __restrict__ src, const NrLayout& L, int g) {
  Tv<ST> v;
#pragma unroll
  for (int c = 0; c < ST; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = L.col(16 * c + 4 * g + r);
      v.t[c][r] = (j >= 0 && j < L.D) ? src[j] : 0.f;
    }
  return v;
}

template <int ST>
HODE_DEV void nr_store_state(float* __restrict__ dst, const NrLayout& L, int g, const Tv<ST>& v, bool live) {
  if (!live) return;
#pragma unroll
  for (int c = 0; c < ST; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = L.col(16 * c + 4 * g + r);
      if (j >= 0 && j < L.D) dst[j] = v.t[c][r];
    }
}

// ------------------------------------------------------------------------------ weight gradients on the matrix cores
// dW1[h][pos] += sum_n u1[h][n] e[pos][n] (the ones row of e collects db1), dW2[o][h] += sum_n u2[o][n] a1[h][n],
// db2 += sum_n u2 over the wave's 16 patients, per stage VJP; operands go through LDS patient-major as in NeuralGradAcc.
constexpr int nr_pitch(int n) { return ((n - 16 + 63) / 64) * 64 + 16; }  // >= n and == 16 mod 64: conflict-free reads

template <int HT, int IT, int OT>
struct NrGradAcc {
  static constexpr int PH = nr_pitch(16 * HT), PE = nr_pitch(16 * IT), PO = nr_pitch(16 * OT);
  static constexpr int kLdsFloats = 16 * (2 * PH + PE + PO);
  static constexpr int NP = 256 * (HT * IT + OT * HT) + 16 * OT;  // floats per wave in the partial array
  v4 dW1[HT][IT], dW2[OT][HT], db2[OT];
  float *U1, *A1, *E, *U2;

  HODE_DEV void init(float* lds) {
    U1 = lds;
    A1 = lds + 16 * PH;
    E = lds + 32 * PH;
    U2 = E + 16 * PE;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
#pragma unroll
      for (int c = 0; c < IT; ++c) dW1[i][c] = splat4(0.f);
#pragma unroll
      for (int o = 0; o < OT; ++o) dW2[o][i] = splat4(0.f);
    }
#pragma unroll
    for (int o = 0; o < OT; ++o) db2[o] = splat4(0.f);
  }

  HODE_DEV void add(const v4 (&u1)[HT], const Tv<IT>& e, const NrSlots<IT>& sl, const v4 (&u2)[OT], const v4 (&a1)[HT],
                    int g, int n) {
    __syncthreads();  // the previous call's reads are done
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      *reinterpret_cast<v4*>(U1 + n * PH + 16 * i + 4 * g) = u1[i];
      *reinterpret_cast<v4*>(A1 + n * PH + 16 * i + 4 * g) = a1[i];
    }
#pragma unroll
    for (int c = 0; c < IT; ++c) {
      v4 x = e.t[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = sl.is_one(c, r) ? 1.0f : x[r];
      *reinterpret_cast<v4*>(E + n * PE + 16 * c + 4 * g) = x;
    }
#pragma unroll
    for (int o = 0; o < OT; ++o) *reinterpret_cast<v4*>(U2 + n * PO + 16 * o + 4 * g) = u2[o];
    __syncthreads();
    const int m = n, kk = g;  // fragment coordinates of this lane
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // patient chunk
      float eB[IT], u2A[OT];
#pragma unroll
      for (int c = 0; c < IT; ++c) eB[c] = E[(4 * q + kk) * PE + 16 * c + m];
#pragma unroll
      for (int o = 0; o < OT; ++o) u2A[o] = U2[(4 * q + kk) * PO + 16 * o + m];
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        const float au = U1[(4 * q + kk) * PH + 16 * i + m];
        const float ba = A1[(4 * q + kk) * PH + 16 * i + m];
#pragma unroll
        for (int c = 0; c < IT; ++c) dW1[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(au, eB[c], dW1[i][c], 0, 0, 0);
#pragma unroll
        for (int o = 0; o < OT; ++o) dW2[o][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(u2A[o], ba, dW2[o][i], 0, 0, 0);
      }
    }
#pragma unroll
    for (int o = 0; o < OT; ++o) db2[o] = db2[o] + u2[o];
  }

  // one block of NP floats per wave: [dW1 tiles (i, c) | dW2 tiles (o, i)] as [tile][lane][4], then db2[16 OT]
  HODE_DEV void store(float* __restrict__ out, int lane) {
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int c = 0; c < IT; ++c) *reinterpret_cast<v4*>(out + ((size_t)(i * IT + c) * 64 + lane) * 4) = dW1[i][c];
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
      for (int i = 0; i < HT; ++i)
        *reinterpret_cast<v4*>(out + ((size_t)(HT * IT + o * HT + i) * 64 + lane) * 4) = dW2[o][i];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      v4 s;
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = row_sum(db2[o][r]);  // over the 16 patients of this row group
      if ((lane & 15) == 0) *reinterpret_cast<v4*>(out + 256 * (HT * IT + OT * HT) + 16 * o + 4 * (lane >> 4)) = s;
    }
  }
};

template <int KIND, int ST, int IT, int HT, int METHOD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void neural_real_fwd_kernel(NrArgs a) {
  using Net = NrNet<KIND, ST, IT, HT>;
  constexpr int S = kNrStages(METHOD);
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const NrLayout L(KIND, a.D);
  const NrSlots<IT> sl(L, g);
  Net net;
  net.load(a, L, lane);
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const size_t row = (size_t)a.B * a.D;
  Tv<ST> y = nr_load_state<ST>(a.y0 + (size_t)p * a.D, L, g);
  float* hp = a.h + (size_t)p * a.D;
  nr_store_state<ST>(hp, L, g, y, live);
  v4 a1[HT];
  float dn[S];  // the doses of the step, loaded one step ahead
  if (a.T > 1) {
#pragma unroll
    for (int s = 0; s < S; ++s) dn[s] = a.dose[(size_t)s * a.B + p];
  }
  for (int nstep = 0; nstep + 1 < a.T; ++nstep) {
    float ds[S];
#pragma unroll
    for (int s = 0; s < S; ++s) ds[s] = dn[s];
    if (nstep + 2 < a.T) {
#pragma unroll
      for (int s = 0; s < S; ++s) dn[s] = a.dose[((size_t)(nstep + 1) * S + s) * a.B + p];
    }
    const float dt = nr_dt(a.t, nstep);
    Tv<IT> e = nr_input<ST, IT>(y, ds[0], sl);
    const Tv<ST> k1 = Net::deriv(e, net.mlp(e, a1));
    if constexpr (METHOD == HODE_METHOD_EULER) {
      y = y + dt * k1;
    } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      e = nr_input<ST, IT>(y + (0.5f * dt) * k1, ds[1], sl);
      const Tv<ST> k2 = Net::deriv(e, net.mlp(e, a1));
      y = y + dt * k2;
    } else {
      e = nr_input<ST, IT>(y + (dt * k1) * kThird, ds[1], sl);
      const Tv<ST> k2 = Net::deriv(e, net.mlp(e, a1));
      e = nr_input<ST, IT>(y + dt * (k2 - k1 * kThird), ds[2], sl);
      const Tv<ST> k3 = Net::deriv(e, net.mlp(e, a1));
      e = nr_input<ST, IT>(y + dt * ((k1 - k2) + k3), ds[3], sl);
      const Tv<ST> k4 = Net::deriv(e, net.mlp(e, a1));
      y = y + ((k1 + 3.0f * (k2 + k3)) + k4) * (dt * 0.125f);
    }
    hp += row;
    nr_store_state<ST>(hp, L, g, y, live);
  }
}

template <int KIND, int ST, int IT, int HT, int METHOD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void neural_real_bwd_kernel(NrArgs a) {
  using Net = NrNet<KIND, ST, IT, HT>;
  constexpr int OT = Net::OT;
  constexpr int S = kNrStages(METHOD);
  using Acc = NrGradAcc<HT, IT, OT>;
  __shared__ __attribute__((aligned(16))) float lds[Acc::kLdsFloats];
  Acc acc;
  acc.init(lds);
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const NrLayout L(KIND, a.D);
  const NrSlots<IT> sl(L, g);
  Net net;
  net.load(a, L, lane);
  const int pr = blockIdx.x * 16 + n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const float lv = live ? 1.0f : 0.0f;  // idle lanes carry zero cotangents: they add nothing to the weight gradients
  const size_t row = (size_t)a.B * a.D;
  const float* hp = a.h + (size_t)p * a.D;
  const float* gp = a.grad_h + (size_t)p * a.D;
  Tv<ST> lam = lv * nr_load_state<ST>(gp + (size_t)(a.T - 1) * row, L, g);
  Tv<ST> yn;
  if (a.T > 1) yn = nr_load_state<ST>(hp + (size_t)(a.T - 2) * row, L, g);
  for (int nstep = a.T - 2; nstep >= 0; --nstep) {
    const Tv<ST> y = yn;
    const Tv<ST> gh = nr_load_state<ST>(gp + (size_t)nstep * row, L, g);  // used at the end of the step
    if (nstep > 0) yn = nr_load_state<ST>(hp + (size_t)(nstep - 1) * row, L, g);
    float ds[S];
#pragma unroll
    for (int s = 0; s < S; ++s) ds[s] = a.dose[((size_t)nstep * S + s) * a.B + p];
    const float dt = nr_dt(a.t, nstep);
    // ---- recompute the stages; only the last stage's activations stay, the VJPs recompute theirs
    Tv<IT> e[S];
    Tv<OT> k[S];
    v4 a1[HT];
    e[0] = nr_input<ST, IT>(y, ds[0], sl);
    k[0] = net.mlp(e[0], a1);
    if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      e[1] = nr_input<ST, IT>(y + (0.5f * dt) * Net::deriv(e[0], k[0]), ds[1], sl);
      k[1] = net.mlp(e[1], a1);
    } else if constexpr (METHOD == HODE_METHOD_RK4_38) {
      const Tv<ST> f0 = Net::deriv(e[0], k[0]);
      e[1] = nr_input<ST, IT>(y + (dt * f0) * kThird, ds[1], sl);
      k[1] = net.mlp(e[1], a1);
      const Tv<ST> f1 = Net::deriv(e[1], k[1]);
      e[2] = nr_input<ST, IT>(y + dt * (f1 - f0 * kThird), ds[2], sl);
      k[2] = net.mlp(e[2], a1);
      e[3] = nr_input<ST, IT>(y + dt * ((f0 - f1) + Net::deriv(e[2], k[2])), ds[3], sl);
      k[3] = net.mlp(e[3], a1);
    }
    // ---- adjoint of the stages
    auto vjp = [&](int s, const Tv<ST>& gf) {
      v4 u2[OT], u1[HT];
      if (s != S - 1) net.hidden(e[s], a1);
      const Tv<ST> ge = net.vjp(a1, k[s], gf, u2, u1);
      acc.add(u1, e[s], sl, u2, a1, g, n);
      return ge;
    };
    if constexpr (METHOD == HODE_METHOD_EULER) {
      lam = lam + vjp(0, dt * lam);
    } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
      const Tv<ST> a1v = vjp(1, dt * lam);
      lam = lam + a1v;
      lam = lam + vjp(0, (0.5f * dt) * a1v);
    } else {
      const float w1 = dt * 0.125f, w3 = dt * 0.375f;
      const Tv<ST> a3 = vjp(3, w1 * lam);
      Tv<ST> da = dt * a3;
      Tv<ST> g1 = w1 * lam + da;
      Tv<ST> g2 = w3 * lam - da;
      const Tv<ST> gg = w3 * lam + da;
      lam = lam + a3;
      const Tv<ST> a2 = vjp(2, gg);
      da = dt * a2;
      g2 = g2 + da;
      g1 = g1 - kThird * da;
      lam = lam + a2;
      const Tv<ST> a1v = vjp(1, g2);
      g1 = g1 + kThird * (dt * a1v);
      lam = lam + a1v;
      lam = lam + vjp(0, g1);
    }
    lam = lam + lv * gh;
  }
  nr_store_state<ST>(a.grad_y0 + (size_t)p * a.D, L, g, lam, live);
  acc.store(a.partials + (size_t)blockIdx.x * Acc::NP, lane);
}

// fixed-order fold of the per-wave blocks into the caller's accumulators (one wave per element of the block)
__global__ __launch_bounds__(64) void neural_real_fold_kernel(const float* __restrict__ partials, int n_waves, int NP, int kind,
                                                              int D, int H, int HT, int IT, int OT, float* __restrict__ gw1,
                                                              float* __restrict__ gb1, float* __restrict__ gw2,
                                                              float* __restrict__ gb2) {
  const int j = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int w = lane; w < n_waves; w += 64) s += partials[(size_t)w * NP + j];
  s = wave_sum(s);
  if (lane != 0) return;
  const NrLayout L(kind, D);
  const int Dm = kind == HODE_RHS_NEURAL_REAL_2ND ? D / 2 : D;
  const int n1 = 256 * HT * IT, n2 = n1 + 256 * OT * HT;
  if (j >= n2) {
    const int o = j - n2;
    if (o < Dm && gb2) gb2[o] += s;
    return;
  }
  const int jj = j < n1 ? j : j - n1;
  const int tile = jj / 256, l = (jj % 256) / 4, r = jj % 4;
  const int rw = 4 * (l >> 4) + r, cl = l & 15;
  if (j < n1) {
    const int hid = 16 * (tile / IT) + rw, cc = L.col(16 * (tile % IT) + cl);
    if (hid >= H || cc < 0) return;
    if (cc <= D) { if (gw1) gw1[(size_t)hid * (D + 1) + cc] += s; }
    else if (gb1) gb1[hid] += s;
  } else {
    const int o = 16 * (tile / HT) + rw, hid = 16 * (tile % HT) + cl;
    if (o < Dm && hid < H && gw2) gw2[(size_t)o * H + hid] += s;
  }
}

// tile counts of a descriptor (the template arguments of its kernels)
struct NrShape {
  int ST, IT, HT, OT;
};
NrShape nr_shape(const hode_solve_desc* d) {
  const NrLayout L(d->rhs_kind, d->latent_dim);
  NrShape s;
  s.ST = d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND ? 2 * (L.off2 / 16) : (d->latent_dim + 15) / 16;
  s.IT = (L.pdose + 2 + 15) / 16;
  s.HT = (d->hidden_dim + 15) / 16;
  s.OT = d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND ? s.ST / 2 : s.ST;
  return s;
}

size_t nr_np(const NrShape& s) { return 256 * (size_t)(s.HT * s.IT + s.OT * s.HT) + 16 * (size_t)s.OT; }

template <int KIND, int ST, int IT, int HT>
int nr_launch(const hode_solve_desc* d, const NrArgs& a, bool bwd, hipStream_t s) {
  const dim3 grid((d->batch + 15) / 16), block(64);
#define HODE_NR_LAUNCH(M)                                                                             \
  if (bwd) hipLaunchKernelGGL((neural_real_bwd_kernel<KIND, ST, IT, HT, M>), grid, block, 0, s, a);  \
  else hipLaunchKernelGGL((neural_real_fwd_kernel<KIND, ST, IT, HT, M>), grid, block, 0, s, a);
  switch (d->method) {
    case HODE_METHOD_EULER: HODE_NR_LAUNCH(HODE_METHOD_EULER) break;
    case HODE_METHOD_MIDPOINT: HODE_NR_LAUNCH(HODE_METHOD_MIDPOINT) break;
    default: HODE_NR_LAUNCH(HODE_METHOD_RK4_38) break;
  }
#undef HODE_NR_LAUNCH
  return hip_fail(hipGetLastError(), "neural-real MFMA kernel launch");
}

template <int KIND, int ST, int IT>
int nr_launch_ht(const hode_solve_desc* d, const NrArgs& a, bool bwd, hipStream_t s, int HT) {
  switch (HT) {
    case 1: return nr_launch<KIND, ST, IT, 1>(d, a, bwd, s);
    case 2: return nr_launch<KIND, ST, IT, 2>(d, a, bwd, s);
    case 3: return nr_launch<KIND, ST, IT, 3>(d, a, bwd, s);
    default: return nr_launch<KIND, ST, IT, 4>(d, a, bwd, s);
  }
}

int check_neural_real(const hode_solve_desc* d, bool bwd) {
  const int D = d->latent_dim, H = d->hidden_dim;
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "neural-real rhs: unknown fixed-grid method %d", d->method);
  if (d->batch <= 0 || d->n_times <= 0 || D <= 0 || H <= 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d latent_dim=%d hidden_dim=%d", d->batch, d->n_times, D, H);
  if (d->rhs_kind == HODE_RHS_NEURAL_REAL && D > 30)
    return fail(HODE_E_UNSUPPORTED, "neural-real rhs: latent_dim %d outside 1..30", D);
  if (d->rhs_kind == HODE_RHS_NEURAL_REAL_2ND && (D % 2 != 0 || D > 60))
    return fail(HODE_E_UNSUPPORTED, "neural-real 2nd rhs: latent_dim %d is not an even number in 2..60", D);
  if (H > 64) return fail(HODE_E_UNSUPPORTED, "neural-real rhs: hidden_dim %d outside 1..64", H);
  if (!d->t || !d->y0 || !d->h || !d->w1 || !d->b1 || !d->w2 || !d->b2 || (d->n_times > 1 && !d->dosage))
    return fail(HODE_E_NULL, "t / y0 / h / w1 / b1 / w2 / b2 / dosage (dose table) must be non-NULL");
  if (bwd) {
    if (!d->grad_h || !d->grad_y0) return fail(HODE_E_NULL, "grad_h / grad_y0 required by the backward");
    if (d->flags & (HODE_FLAG_OVERWRITE_GRADS | HODE_FLAG_SKIP_FOLD))
      return fail(HODE_E_UNSUPPORTED, "neural-real backward: HODE_FLAG_OVERWRITE_GRADS / HODE_FLAG_SKIP_FOLD are not implemented");
  }
  return 0;
}

}  // namespace

size_t neural_real_workspace_bytes(const hode_solve_desc* d, bool bwd) {
  if (!bwd || d->batch <= 0 || d->hidden_dim <= 0 || d->latent_dim <= 0) return 0;
  return (size_t)((d->batch + 15) / 16) * nr_np(nr_shape(d)) * sizeof(float);
}

int neural_real_rk(const hode_solve_desc* d, bool bwd, hipStream_t s) {
  if (int e = check_neural_real(d, bwd)) return e;
  const size_t need = neural_real_workspace_bytes(d, bwd);
  if (need && (!d->workspace || d->workspace_bytes < need))
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  NrArgs a{};
  a.t = d->t; a.y0 = d->y0; a.dose = d->dosage; a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  a.h = d->h; a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0; a.partials = (float*)d->workspace;
  a.B = d->batch; a.T = d->n_times; a.D = d->latent_dim; a.H = d->hidden_dim; a.kind = d->rhs_kind;
  const NrShape sh = nr_shape(d);
  int e;
  if (d->rhs_kind == HODE_RHS_NEURAL_REAL) {
    if (sh.ST == 1 && sh.IT == 1) e = nr_launch_ht<HODE_RHS_NEURAL_REAL, 1, 1>(d, a, bwd, s, sh.HT);
    else if (sh.ST == 1) e = nr_launch_ht<HODE_RHS_NEURAL_REAL, 1, 2>(d, a, bwd, s, sh.HT);
    else e = nr_launch_ht<HODE_RHS_NEURAL_REAL, 2, 2>(d, a, bwd, s, sh.HT);
  } else {
    if (sh.ST == 2 && sh.IT == 2) e = nr_launch_ht<HODE_RHS_NEURAL_REAL_2ND, 2, 2>(d, a, bwd, s, sh.HT);
    else if (sh.ST == 2) e = nr_launch_ht<HODE_RHS_NEURAL_REAL_2ND, 2, 3>(d, a, bwd, s, sh.HT);
    else e = nr_launch_ht<HODE_RHS_NEURAL_REAL_2ND, 4, 4>(d, a, bwd, s, sh.HT);
  }
  if (e || !bwd) return e;
  const int np = (int)nr_np(sh);
  hipLaunchKernelGGL(neural_real_fold_kernel, dim3(np), dim3(64), 0, s, a.partials, (d->batch + 15) / 16, np, d->rhs_kind,
                     d->latent_dim, d->hidden_dim, sh.HT, sh.IT, sh.OT, d->grad_w1, d->grad_b1, d->grad_w2, d->grad_b2);
  return hip_fail(hipGetLastError(), "neural-real gradient fold launch");
}

}  // namespace hode
