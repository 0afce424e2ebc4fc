// Device code of the real-data hybrid rhs on the matrix cores, shared by the two libraries that hold it: libhode.so
// (hode_real_mf.hip: D = 20, the GRU block fills its 16-row tile) and libhode_real_dims.so (real_dims/: D = 5 .. 20, a ragged
// tile with M = D - 4 as a runtime argument).  RealMf is the rhs and its VJP on register-resident weight operands,
// RealGradAcc the on-chip weight-gradient accumulator, real_grad_fold its fold, real_step_fwd / HODE_REAL_STEP_STAGES /
// HODE_REAL_STEP_CHAIN one solver step and its adjoint, real_mf_body the time loop over them and its discrete adjoint; the kernels
// of either library are thin __global__ wrappers around the fold and the body.  libhode_real_step.so (real_step/) walks
// independent intervals with the same pieces.  See hode_real_mf.hip for the recipe.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_real_args.hpp"

namespace hode {

// how the GRU states fill the H tile (see real_mf_body)
struct RealTileFull {
  static constexpr bool kRagged = false;
  HODE_DEV constexpr int m() const { return 16; }
};
struct RealTileRagged {
  static constexpr bool kRagged = true;
  int M;  // 1 .. 16
  HODE_DEV int m() const { return M; }
};

HODE_DEV v4 mfma4(float a, float b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr float kTanhScale = 2.885390081777927f;   // 2 log2(e)
// the activations are tanh_scaled4 (hode_common.hpp) of z' = kTanhScale z

template <int HT, class Tile = RealTileFull>
struct RealMf {
  static constexpr int NT2 = 2 * HT;
  float A1a[HT][3], A1b[HT][2];   // hidden layers: W11[16i+m][r], W21[16i+m][r] in lanes g == 0
  float A2[NT2][4];               // output layer: row 0 <- w12, row 1 <- w22
  float A3[NT2];                  // hidden cotangent: w12[16i+m] (chunk 0) / w22[16(i-HT)+m] (chunk 1), lanes g == 0
  float A4[NT2][4];               // input cotangent: W11[16i+4g+r][m] (m < 3) / W21[..][m] (m < 2)
  float Gr[4], Gz[4], Gh[4], GrT[4], GzT[4], GhT[4];
  v4 b1[NT2];
  v4 b2;
  int g, n;
  float kim, kel, kel2;

  HODE_DEV void load(const RealArgs& a, const Tile& tile, int lane) {
    const int M = tile.m();
    g = lane >> 4;
    n = lane & 15;
    const int m = lane & 15;
    const int H = a.H;
    const RealW w(a.wflat, H, M);
    kim = a.theta[0]; kel = a.theta[1]; kel2 = a.theta[2];
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      const int j = 16 * i + m;  // hidden unit addressed as an A ROW
      // the hidden layers' tanh takes its argument pre-multiplied by 2 log2(e) (kTanhScale, folded into W11 / W21 / b11 / b21 here):
      // v_exp, add, v_rcp, fma per activation, the fma on pairs -- see NeuralMf::tanh_scaled
#pragma unroll
      for (int r = 0; r < 3; ++r) A1a[i][r] = (g == 0 && j < H) ? kTanhScale * w.W11[3 * j + r] : 0.f;
#pragma unroll
      for (int r = 0; r < 2; ++r) A1b[i][r] = (g == 0 && j < H) ? kTanhScale * w.W21[2 * j + r] : 0.f;
      A3[i] = (g == 0 && j < H) ? w.w12[j] : 0.f;
      A3[HT + i] = (g == 0 && j < H) ? w.w22[j] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jc = 16 * i + 4 * g + r;  // hidden unit addressed as a K index / tile row
        A2[i][r] = (m == 0 && jc < H) ? w.w12[jc] : 0.f;
        A2[HT + i][r] = (m == 1 && jc < H) ? w.w22[jc] : 0.f;
        A4[i][r] = (m < 3 && jc < H) ? w.W11[3 * jc + m] : 0.f;
        A4[HT + i][r] = (m < 2 && jc < H) ? w.W21[2 * jc + m] : 0.f;
        b1[i][r] = jc < H ? kTanhScale * w.b11[jc] : 0.f;
        b1[HT + i][r] = jc < H ? kTanhScale * w.b21[jc] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 4 * g + r;
      if constexpr (Tile::kRagged) {  // rows and columns >= M of the 16 x 16 operands are zero: they are not in memory
        const bool in = m < M && c < M;
        Gr[r] = in ? w.Whr[m * M + c] : 0.f; Gz[r] = in ? w.Whz[m * M + c] : 0.f; Gh[r] = in ? w.Whh[m * M + c] : 0.f;
        GrT[r] = in ? w.Whr[c * M + m] : 0.f; GzT[r] = in ? w.Whz[c * M + m] : 0.f; GhT[r] = in ? w.Whh[c * M + m] : 0.f;
      } else {
        Gr[r] = w.Whr[m * M + c]; Gz[r] = w.Whz[m * M + c]; Gh[r] = w.Whh[m * M + c];
        GrT[r] = w.Whr[c * M + m]; GzT[r] = w.Whz[c * M + m]; GhT[r] = w.Whh[c * M + m];
      }
    }
    b2 = v4{0.f, 0.f, 0.f, 0.f};
    if (g == 0) {
      b2[0] = w.b12[0];
      b2[1] = w.b22[0];
    }
  }

  struct Stage {  // what the VJP needs of one evaluation
    v4 X, Hs, KX, ah[NT2], r, z, u, RH;
    float dv, ddk;
  };

  // k = f(X, Hs); dose = (Dose(t), dDose/dkel) in lanes g == 0, zeros elsewhere
  HODE_DEV void rhs(Stage& s, v4& KH) const {
    v4 acc[NT2];
#pragma unroll
    for (int i = 0; i < NT2; ++i) acc[i] = b1[i];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        acc[i] = mfma4(A1a[i][r], s.X[r], acc[i]);
        if (r < 2) acc[HT + i] = mfma4(A1b[i][r < 2 ? r : 0], s.X[r], acc[HT + i]);
      }
#pragma unroll
    for (int i = 0; i < NT2; ++i) s.ah[i] = tanh_scaled4(acc[i]);
    v4 zz[4];
    zz[0] = b2;
    zz[1] = zz[2] = zz[3] = v4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NT2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) zz[r] = mfma4(A2[i][r], s.ah[i][r], zz[r]);
    const v4 S = (zz[0] + zz[1]) + (zz[2] + zz[3]);
    s.KX[0] = tanh_f32(S[0]);           // rows 4g + r of lanes g > 0 are not state: everything below is 0 there
    s.KX[1] = tanh_f32(S[1]);
    s.KX[2] = s.X[1] * kim;
    s.KX[3] = __builtin_fmaf(kel, s.dv, -kel2 * s.X[3]);
    // GRU block
    v4 ar = v4{0.f, 0.f, 0.f, 0.f}, az = ar, au = ar;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ar = mfma4(Gr[r], s.Hs[r], ar);
      az = mfma4(Gz[r], s.Hs[r], az);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s.r[r] = sigm(ar[r]);
      s.z[r] = sigm(az[r]);
      s.RH[r] = s.r[r] * s.Hs[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) au = mfma4(Gh[r], s.RH[r], au);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s.u[r] = tanh_f32(au[r]);
      KH[r] = (1.0f - s.z[r]) * (s.u[r] - s.Hs[r]);
    }
  }

  // (aX, aH) = (df/dy)^T (gX, gH) at stage s; cotangent tiles for the tape; scalar gradients into dth
  HODE_DEV void vjp(const Stage& s, const v4& gX, const v4& gH, v4& aX, v4& aH, v4 (&U1)[NT2], float& u12, float& u22,
                    v4& ur, v4& uz, v4& uh, float (&dth)[3]) const {
    u12 = gX[0] * __builtin_fmaf(-s.KX[0], s.KX[0], 1.0f);
    u22 = gX[1] * __builtin_fmaf(-s.KX[1], s.KX[1], 1.0f);
    v4 da[NT2];
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      da[i] = mfma4(A3[i], u12, v4{0.f, 0.f, 0.f, 0.f});
      da[HT + i] = mfma4(A3[HT + i], u22, v4{0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int i = 0; i < NT2; ++i)   // the same two operations per value (fma, mul), on pairs
      U1[i] = da[i] * __builtin_elementwise_fma(-s.ah[i], s.ah[i], v4{1.0f, 1.0f, 1.0f, 1.0f});
    v4 zz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) zz[r] = v4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NT2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) zz[r] = mfma4(A4[i][r], U1[i][r], zz[r]);
    aX = (zz[0] + zz[1]) + (zz[2] + zz[3]);
    aX[1] = __builtin_fmaf(gX[2], kim, aX[1]);
    aX[3] = __builtin_fmaf(-kel2, gX[3], aX[3]);
    dth[0] = __builtin_fmaf(gX[2], s.X[1], dth[0]);
    dth[1] = __builtin_fmaf(gX[3], __builtin_fmaf(kel, s.ddk, s.dv), dth[1]);
    dth[2] = __builtin_fmaf(-gX[3], s.X[3], dth[2]);
    // GRU block
    v4 drh = v4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uz[r] = -gH[r] * (s.u[r] - s.Hs[r]) * s.z[r] * (1.0f - s.z[r]);
      uh[r] = gH[r] * (1.0f - s.z[r]) * __builtin_fmaf(-s.u[r], s.u[r], 1.0f);
      aH[r] = -gH[r] * (1.0f - s.z[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) drh = mfma4(GhT[r], uh[r], drh);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ur[r] = drh[r] * s.Hs[r] * s.r[r] * (1.0f - s.r[r]);
      aH[r] = __builtin_fmaf(drh[r], s.r[r], aH[r]);
    }
    v4 acc = v4{0.f, 0.f, 0.f, 0.f}, acc2 = acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc = mfma4(GrT[r], ur[r], acc);
      acc2 = mfma4(GzT[r], uz[r], acc2);
    }
    aH = aH + (acc + acc2);
  }
};

// ------------------------------------------------------------------------------ weight gradients on the matrix cores
// The eleven weight gradients of the rhs are outer products summed over patients (recipe of NeuralGradAcc in
// hode_neural_mf.hpp: operands transposed through patient-major LDS images so that the patient index becomes the MFMA
// contraction index).  Per stage VJP, over the wave's 16 patients:
//   dWa[i] += U1 tile i (x) [X | 1]      i <  HT: rows of dW11 (cols 0..2) and db11 (col 4, the ones row behind X)
//                                         i >= HT: rows of dW21 (cols 0..1) and db21 (col 4)
//   dWb[i] += [u12; u22] (x) ah tile i    i <  HT: row 0 = dw12;  i >= HT: row 1 = dw22   (the cross terms are not read)
//   dHh += uh (x) r*h,  dHz += uz (x) h,  dHr += ur (x) h;   db12 / db22: per-lane sums of u12 / u22
// 60 MFMAs, 19 ds_write_b128 and 76 ds_read_b32 per stage at HT = 3 instead of ~70 strided tape stores per lane; one block
// of NP floats per wave, folded in a fixed order by real_grad_fold_kernel into the flat weight-gradient buffer.
template <int HT>
struct RealGradAcc {
  static constexpr int NT2 = 2 * HT;
  static constexpr int PH = ((16 * NT2 - 16 + 63) / 64) * 64 + 16;  // pitch == 16 mod 64: conflict-free fragment reads
  static constexpr int kLdsFloats = 2 * 16 * PH + 7 * 256;
  static constexpr int NP = (2 * NT2 + 3) * 256 + 16;
  v4 dWa[NT2], dWb[NT2], dHh, dHz, dHr, db2;
  float *U1i, *AHi, *Xi, *U2i, *UHi, *UZi, *URi, *RHi, *HHi;
  HODE_DEV void init(float* lds) {
    U1i = lds; AHi = lds + 16 * PH;
    float* sm = lds + 32 * PH;
    Xi = sm; U2i = sm + 256; UHi = sm + 512; UZi = sm + 768; URi = sm + 1024; RHi = sm + 1280; HHi = sm + 1536;
    const v4 z = v4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NT2; ++i) dWa[i] = dWb[i] = z;
    dHh = dHz = dHr = db2 = z;
  }
  HODE_DEV void add(const v4 (&U1)[NT2], const v4 (&ah)[NT2], v4 X, float u12, float u22, const v4& uh, const v4& uz,
                    const v4& ur, const v4& rh, const v4& hh, int g, int n) {
    if (g == 1) X[0] = 1.0f;  // row 4: the bias column
    const v4 U2 = v4{u12, u22, 0.f, 0.f};  // lanes g > 0 carry zeros (gX is zero there)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT2; ++i) {
      *reinterpret_cast<v4*>(U1i + n * PH + 16 * i + 4 * g) = U1[i];
      *reinterpret_cast<v4*>(AHi + n * PH + 16 * i + 4 * g) = ah[i];
    }
    *reinterpret_cast<v4*>(Xi + n * 16 + 4 * g) = X;
    *reinterpret_cast<v4*>(U2i + n * 16 + 4 * g) = U2;
    *reinterpret_cast<v4*>(UHi + n * 16 + 4 * g) = uh;
    *reinterpret_cast<v4*>(UZi + n * 16 + 4 * g) = uz;
    *reinterpret_cast<v4*>(URi + n * 16 + 4 * g) = ur;
    *reinterpret_cast<v4*>(RHi + n * 16 + 4 * g) = rh;
    *reinterpret_cast<v4*>(HHi + n * 16 + 4 * g) = hh;
    __syncthreads();
    const int m = n, kk = g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int o = (4 * c + kk) * 16 + m;
      const float xB = Xi[o], u2A = U2i[o], rhB = RHi[o], hhB = HHi[o];
      dHh = mfma4(UHi[o], rhB, dHh);
      dHz = mfma4(UZi[o], hhB, dHz);
      dHr = mfma4(URi[o], hhB, dHr);
#pragma unroll
      for (int i = 0; i < NT2; ++i) {
        dWa[i] = mfma4(U1i[(4 * c + kk) * PH + 16 * i + m], xB, dWa[i]);
        dWb[i] = mfma4(u2A, AHi[(4 * c + kk) * PH + 16 * i + m], dWb[i]);
      }
    }
    db2 = db2 + U2;
  }
  HODE_DEV void store(float* __restrict__ out, int lane) {
#pragma unroll
    for (int i = 0; i < NT2; ++i) {
      *reinterpret_cast<v4*>(out + ((size_t)i * 64 + lane) * 4) = dWa[i];
      *reinterpret_cast<v4*>(out + ((size_t)(NT2 + i) * 64 + lane) * 4) = dWb[i];
    }
    *reinterpret_cast<v4*>(out + ((size_t)(2 * NT2) * 64 + lane) * 4) = dHh;
    *reinterpret_cast<v4*>(out + ((size_t)(2 * NT2 + 1) * 64 + lane) * 4) = dHz;
    *reinterpret_cast<v4*>(out + ((size_t)(2 * NT2 + 2) * 64 + lane) * 4) = dHr;
    v4 sv;
#pragma unroll
    for (int r = 0; r < 4; ++r) sv[r] = row_sum(db2[r]);
    if ((lane & 15) == 0) *reinterpret_cast<v4*>(out + (2 * NT2 + 3) * 256 + 4 * (lane >> 4)) = sv;
  }
};

// fixed-order fold of the per-wave blocks into the flat weight gradient (RealW order); one wave per slot of a block
// (M = 16: every entry of the three GRU blocks is live; M < 16: row stride M, the padded rows and columns are not written)
template <int HT>
HODE_DEV void real_grad_fold(const float* __restrict__ partials, int n_waves, int H, const int M, float* __restrict__ gw) {
  constexpr int NT2 = 2 * HT, NP = RealGradAcc<HT>::NP;
  const int j = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int w = lane; w < n_waves; w += 64) s += partials[(size_t)w * NP + j];
  s = wave_sum(s);
  if (lane != 0) return;
  const int oW11 = 0, ob11 = 3 * H, ow12 = 4 * H, ob12 = 5 * H, oW21 = 5 * H + 1, ob21 = 7 * H + 1, ow22 = 8 * H + 1,
            ob22 = 9 * H + 1, oWhh = 9 * H + 2, oWhz = oWhh + M * M, oWhr = oWhz + M * M;
  if (j >= (2 * NT2 + 3) * 256) {
    const int o = j - (2 * NT2 + 3) * 256;
    if (o == 0) gw[ob12] += s;
    else if (o == 1) gw[ob22] += s;
    return;
  }
  const int tile = j / 256, l = (j % 256) / 4, r = j % 4;
  const int rw = 4 * (l >> 4) + r, col = l & 15;
  if (tile < NT2) {
    const bool first = tile < HT;
    const int hid = 16 * (first ? tile : tile - HT) + rw;
    if (hid >= H) return;
    if (first) {
      if (col < 3) gw[oW11 + 3 * hid + col] += s;
      else if (col == 4) gw[ob11 + hid] += s;
    } else {
      if (col < 2) gw[oW21 + 2 * hid + col] += s;
      else if (col == 4) gw[ob21 + hid] += s;
    }
  } else if (tile < 2 * NT2) {
    const int i = tile - NT2;
    const bool first = i < HT;
    const int hid = 16 * (first ? i : i - HT) + col;
    if (hid >= H) return;
    if (first && rw == 0) gw[ow12 + hid] += s;
    else if (!first && rw == 1) gw[ow22 + hid] += s;
  } else {
    const int which = tile - 2 * NT2;
    if (rw >= M || col >= M) return;
    gw[(which == 0 ? oWhh : (which == 1 ? oWhz : oWhr)) + rw * M + col] += s;
  }
}

// ------------------------------------------------------------------------------------ one solver step, shared pieces
// What real_mf_body (the chained solve) and csrc/real_step/ (the one-step-ahead solve) both run: the guarded state I/O of a
// tile, the dose of a stage, the stage arithmetic of one solver step forward, its recomputation for the adjoint and the
// cotangent chain through the stages.
constexpr int real_stages(int method) { return method == HODE_METHOD_EULER ? 1 : (method == HODE_METHOD_MIDPOINT ? 2 : 4); }

template <class Tile>
HODE_DEV void real_load_state(const Tile& tile, int g, const float* src, v4& X, v4& Hs) {  // src -> one patient's D floats
  X = v4{0.f, 0.f, 0.f, 0.f};
  if constexpr (Tile::kRagged) {
    const int M = tile.m();
    if (g == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) X[r] = src[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Hs[r] = 4 * g + r < M ? src[4 + 4 * g + r] : 0.f;
  } else {
    if (g == 0) X = *reinterpret_cast<const v4*>(src);
    Hs = *reinterpret_cast<const v4*>(src + 4 + 4 * g);
  }
}
template <class Tile>
HODE_DEV void real_store_state(const Tile& tile, int g, float* dst, const v4& X, const v4& Hs) {  // the caller checks `live`
  if constexpr (Tile::kRagged) {
    const int M = tile.m();
    if (g == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[r] = X[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < M) dst[4 + 4 * g + r] = Hs[r];
  } else {
    if (g == 0) *reinterpret_cast<v4*>(dst) = X;
    *reinterpret_cast<v4*>(dst + 4 + 4 * g) = Hs;
  }
}
template <class Stage>
HODE_DEV void real_set_dose(const RealArgs& a, int p, float kel, bool g0, Stage& s, float t) {
  s.dv = 0.f;
  s.ddk = 0.f;
  if (g0) {
    const DoseK d = real_dose(a, p, t, kel);
    s.dv = d.v;
    s.ddk = d.dk;
  }
}

// (X, Hs) at st.t0 -> (X, Hs) at st.t1; `s` is the caller's stage scratch, set_dose(stage, t) fills a stage's dose
template <int METHOD, class Net, class SetDose>
HODE_DEV void real_step_fwd(const Net& nn, typename Net::Stage& s, const RStageTimes& st, v4& X, v4& Hs, SetDose&& set_dose) {
  constexpr float c13 = (float)(1.0 / 3.0);
  const float dt = st.dt;
  v4 k1H;
  s.X = X; s.Hs = Hs; set_dose(s, st.t_first);
  nn.rhs(s, k1H);
  const v4 k1X = s.KX;
  if constexpr (METHOD == HODE_METHOD_EULER) {
    X = X + dt * k1X; Hs = Hs + dt * k1H;
  } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {
    v4 k2H;
    s.X = X + (0.5f * dt) * k1X; s.Hs = Hs + (0.5f * dt) * k1H; set_dose(s, st.ta);
    nn.rhs(s, k2H);
    X = X + dt * s.KX; Hs = Hs + dt * k2H;
  } else {
    v4 k2H, k3H, k4H;
    s.X = X + (dt * k1X) * c13; s.Hs = Hs + (dt * k1H) * c13; set_dose(s, st.ta);
    nn.rhs(s, k2H);
    const v4 k2X = s.KX;
    s.X = X + dt * (k2X - k1X * c13); s.Hs = Hs + dt * (k2H - k1H * c13); set_dose(s, st.tb);
    nn.rhs(s, k3H);
    const v4 k3X = s.KX;
    s.X = X + dt * ((k1X - k2X) + k3X); s.Hs = Hs + dt * ((k1H - k2H) + k3H); set_dose(s, st.t_last);
    nn.rhs(s, k4H);
    X = X + ((k1X + 3.0f * (k2X + k3X)) + s.KX) * (dt * 0.125f);
    Hs = Hs + ((k1H + 3.0f * (k2H + k3H)) + k4H) * (dt * 0.125f);
  }
}

// The stages of the step from (X, Hs) over `st`, kept for the VJPs: s[q] and kH[q] of stage q (arrays of real_stages(METHOD)
// entries).  A macro, not a function: as an inlined function the same statements compile to another instruction schedule in
// the chained kernels, whose device code is held fixed (profiles/real_step_device_code_diff.txt).
constexpr float kRealThird = (float)(1.0 / 3.0);
#define HODE_REAL_STEP_STAGES(METHOD, nn, s, kH, st, X, Hs, set_dose)                                                        \
  s[0].X = X; s[0].Hs = Hs; set_dose(s[0], st.t_first);                                                                      \
  nn.rhs(s[0], kH[0]);                                                                                                       \
  if constexpr (METHOD == HODE_METHOD_MIDPOINT) {                                                                            \
    s[1].X = X + (0.5f * st.dt) * s[0].KX; s[1].Hs = Hs + (0.5f * st.dt) * kH[0]; set_dose(s[1], st.ta);                     \
    nn.rhs(s[1], kH[1]);                                                                                                     \
  } else if constexpr (METHOD == HODE_METHOD_RK4_38) {                                                                       \
    s[1].X = X + (st.dt * s[0].KX) * kRealThird; s[1].Hs = Hs + (st.dt * kH[0]) * kRealThird; set_dose(s[1], st.ta);         \
    nn.rhs(s[1], kH[1]);                                                                                                     \
    s[2].X = X + st.dt * (s[1].KX - s[0].KX * kRealThird); s[2].Hs = Hs + st.dt * (kH[1] - kH[0] * kRealThird);              \
    set_dose(s[2], st.tb);                                                                                                   \
    nn.rhs(s[2], kH[2]);                                                                                                     \
    s[3].X = X + st.dt * ((s[0].KX - s[1].KX) + s[2].KX); s[3].Hs = Hs + st.dt * ((kH[0] - kH[1]) + kH[2]);                  \
    set_dose(s[3], st.t_last);                                                                                               \
    nn.rhs(s[3], kH[3]);                                                                                                     \
  }

// (lamX, lamH) at the end of the step of length dt -> at its start; vjp(q, gX, gH, aX, aH) is the VJP of stage q.  Declares aX
// and aH in the enclosing scope.  A macro for the reason given above.
#define HODE_REAL_STEP_CHAIN(METHOD, dt, lamX, lamH, vjp)                                                                     \
  v4 aX, aH;                                                                                                                  \
  if constexpr (METHOD == HODE_METHOD_EULER) {                                                                                \
    vjp(0, dt * lamX, dt * lamH, aX, aH);                                                                                     \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
  } else if constexpr (METHOD == HODE_METHOD_MIDPOINT) {                                                                      \
    vjp(1, dt * lamX, dt * lamH, aX, aH);                                                                                     \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
    const v4 gX = (0.5f * dt) * aX, gH = (0.5f * dt) * aH;                                                                    \
    vjp(0, gX, gH, aX, aH);                                                                                                   \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
  } else {                                                                                                                    \
    const float w1 = dt * 0.125f, w3 = dt * 0.375f;                                                                           \
    vjp(3, w1 * lamX, w1 * lamH, aX, aH);                                                                                     \
    v4 daX = dt * aX, daH = dt * aH;                                                                                          \
    v4 g1X = w1 * lamX + daX, g1H = w1 * lamH + daH;                                                                          \
    v4 g2X = w3 * lamX - daX, g2H = w3 * lamH - daH;                                                                          \
    const v4 gX = w3 * lamX + daX, gH = w3 * lamH + daH;                                                                      \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
    vjp(2, gX, gH, aX, aH);                                                                                                   \
    daX = dt * aX; daH = dt * aH;                                                                                             \
    g2X = g2X + daX; g2H = g2H + daH;                                                                                         \
    g1X = g1X - kRealThird * daX; g1H = g1H - kRealThird * daH;                                                               \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
    vjp(1, g2X, g2H, aX, aH);                                                                                                 \
    g1X = g1X + kRealThird * (dt * aX); g1H = g1H + kRealThird * (dt * aH);                                                   \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
    vjp(0, g1X, g1H, aX, aH);                                                                                                 \
    lamX = lamX + aX; lamH = lamH + aH;                                                                                       \
  }

// ONCHIP (backward): weight gradients accumulated by the wave (RealGradAcc), one partial block per wave in a.tape;
// otherwise the GEMM operands are taped for the caller (contract of the lane-per-patient kernels).
// `tile` says how the M = D - 4 GRU states sit in the 16-row H tile: RealTileFull (M = 16, rows of 20 floats, float4 I/O) or
// RealTileRagged (runtime M <= 16: rows >= M are zero and stay zero -- u = tanh(0) = 0, dH = (1 - z)(u - H) = 0 -- and every
// load and store of a state row is element-wise and guarded, so that nothing outside the D floats of a patient is touched).
// `lds` is the RealGradAcc image of the on-chip backward (RealGradAcc<HT>::kLdsFloats floats; unused otherwise).
// `dose` is the on-chip backward's hook for the gradient of the dose table (real_dose/hode_real_dose_ht.hip).  A hook with
// kGrad set is called before the sweep (begin), after the acc.add of every stage VJP (tap) and after the sweep, before
// grad_y0 is stored (finish); this one does nothing, and the kernels without a hook compile as if there were none.
struct NoRealDoseGrad {
  static constexpr bool kGrad = false;
};
template <int HT, int METHOD, bool BWD, bool ONCHIP, class Tile, class DOSE = NoRealDoseGrad>
HODE_DEV void real_mf_body(const RealArgs& a, const Tile tile, float* lds, DOSE dose = DOSE{}) {
  static_assert(!DOSE::kGrad || (BWD && ONCHIP), "the dose hook is the on-chip backward's");
  typedef RealMf<HT, Tile> Net;
  typedef typename Net::Stage Stage;
  constexpr int NT2 = 2 * HT;
  const int M = tile.m(), D = M + 4;
  constexpr int NS = real_stages(METHOD);
  const int lane = threadIdx.x;
  Net nn;
  nn.load(a, tile, lane);
  const int g = nn.g;
  const bool g0 = g == 0;
  const int pr = blockIdx.x * 16 + nn.n;
  const bool live = pr < a.B;
  const int p = live ? pr : a.B - 1;
  const size_t B = a.B;
  const size_t row = B * D;
  const RealTape tl{a.H, M};
  const size_t tstride = (size_t)tl.rows() * B;
  RealGradAcc<HT> acc;
  if constexpr (BWD && ONCHIP) acc.init(lds);
  if (g0) real_dose_table(a, p, nn.kel);  // each lane reads back only its own column

  auto load_state = [&](const float* src, v4& X, v4& Hs) { real_load_state(tile, g, src, X, Hs); };
  auto store_state = [&](float* dst, const v4& X, const v4& Hs) {
    if (live) real_store_state(tile, g, dst, X, Hs);
  };
  auto set_dose = [&](Stage& s, float t) { real_set_dose(a, p, nn.kel, g0, s, t); };

  if constexpr (!BWD) {
    v4 X, Hs;
    load_state(a.y0 + (size_t)p * D, X, Hs);
    store_state(a.h + (size_t)p * D, X, Hs);
    Stage s;
    for (int n = 0; n + 1 < a.T; ++n) {
      const RStageTimes st(a.t, n, a.perturb, METHOD);
      real_step_fwd<METHOD>(nn, s, st, X, Hs, set_dose);
      store_state(a.h + (size_t)(n + 1) * row + (size_t)p * D, X, Hs);
    }
  } else {
    const float lv = live ? 1.0f : 0.0f;
    float dth[3] = {0.f, 0.f, 0.f};
    v4 lamX, lamH;
    load_state(a.grad_h + (size_t)(a.T - 1) * row + (size_t)p * D, lamX, lamH);
    lamX = lv * lamX; lamH = lv * lamH;
    if constexpr (DOSE::kGrad) dose.begin(a, p, g0 && live, nn.kel);

    auto tape_tile = [&](float* tp, int first_row, int nrows, const v4& v) {  // rows 4g + r of a 16-row vector
      if (!live) return;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rw = 4 * g + r;
        if (rw < nrows) tp[(size_t)(first_row + rw) * B] = v[r];
      }
    };
    auto tape_hidden = [&](float* tp, int first_row, const v4* v) {  // HT tiles, rows < hidden_dim
      if (!live) return;
#pragma unroll
      for (int i = 0; i < HT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rw = 16 * i + 4 * g + r;
          if (rw < a.H) tp[(size_t)(first_row + rw) * B] = v[i][r];
        }
    };

    for (int n = a.T - 2; n >= 0; --n) {
      const RStageTimes st(a.t, n, a.perturb, METHOD);
      float* tp0 = a.tape + (size_t)n * NS * tstride + p;
      v4 X, Hs;
      load_state(a.h + (size_t)n * row + (size_t)p * D, X, Hs);
      Stage s[NS];
      v4 kH[NS];
      HODE_REAL_STEP_STAGES(METHOD, nn, s, kH, st, X, Hs, set_dose)
      auto vjp = [&](int q, const v4& gX, const v4& gH, v4& aX, v4& aH) {
        v4 U1[NT2], ur, uz, uh;
        float u12, u22;
        nn.vjp(s[q], gX, gH, aX, aH, U1, u12, u22, ur, uz, uh, dth);
        if constexpr (ONCHIP) {
          acc.add(U1, s[q].ah, s[q].X, u12, u22, uh, uz, ur, s[q].RH, s[q].Hs, g, nn.n);
          if constexpr (DOSE::kGrad) dose.tap(st, q, gX[3]);
          return;
        }
        float* tp = tp0 + (size_t)q * tstride;
        tape_tile(tp, tl.y3(), 3, s[q].X);
        tape_hidden(tp, tl.a11(), s[q].ah);
        tape_hidden(tp, tl.u11(), U1);
        tape_hidden(tp, tl.a21(), s[q].ah + HT);
        tape_hidden(tp, tl.u21(), U1 + HT);
        if (live && g0) {
          tp[(size_t)tl.u12() * B] = u12;
          tp[(size_t)tl.u22() * B] = u22;
        }
        tape_tile(tp, tl.hh(), M, s[q].Hs);
        tape_tile(tp, tl.rh(), M, s[q].RH);
        tape_tile(tp, tl.ur(), M, ur);
        tape_tile(tp, tl.uz(), M, uz);
        tape_tile(tp, tl.uh(), M, uh);
      };
      HODE_REAL_STEP_CHAIN(METHOD, st.dt, lamX, lamH, vjp)
      v4 ghX, ghH;
      load_state(a.grad_h + (size_t)n * row + (size_t)p * D, ghX, ghH);
      lamX = lamX + lv * ghX; lamH = lamH + lv * ghH;
    }
    if constexpr (DOSE::kGrad) dose.finish();
    store_state(a.grad_y0 + (size_t)p * D, lamX, lamH);
    // only lanes g == 0 of live patients carry scalar-gradient terms (X, gX are zero elsewhere; lv zeroes dead patients)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = wave_sum(g0 ? dth[j] : 0.f);
      if (lane == 0) a.partials[(size_t)blockIdx.x * 3 + j] = v;
    }
    if constexpr (ONCHIP) acc.store(a.tape + (size_t)blockIdx.x * RealGradAcc<HT>::NP, lane);
  }
}

}  // namespace hode
