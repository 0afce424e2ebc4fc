// Masked single-layer LSTM over an observation window on the matrix cores (fp32 MFMA), gfx950.
//
// Replaces the T single-step nn.LSTM calls of EncoderLSTM.forward (reference model.py:420-422; EncoderLSTMReal
// :226-229) and fuses the cat([x, a]) * cat([mask, 1]) that feeds them (model.py:415-421).  CPU restatement:
// oracle/encoder.py::lstm_cell.  Gate order i, f, g, o; gates = x W_ih^T + b_ih + h W_hh^T + b_hh.
//
// Design.  A workgroup (4 waves) owns a tile of BT = 16*NT patients for the WHOLE window:
// h and c never leave the chip.  Per step the gate pre-activations G^T[4H x BT] = Wcat[4H x K] * act^T[K x BT]
// (K = I + H) are accumulated with v_mfma_f32_16x16x4_f32 -- exact fp32, the matrix pipe's rate for this dtype.
//   * Wcat is the A operand.  Its rows are permuted so that one 16-row MFMA tile = 4 hidden units x 4 gates; in the
//     16x16 accumulator layout (row = 4*(lane>>4) + reg, col = lane&15) a lane then holds all four gates of ONE
//     (unit, patient) pair in its 4 registers: the cell update needs no cross-lane traffic at all.
//     Wave w owns hidden units [w*H/4, (w+1)*H/4); its quarter of Wcat is streamed from L2 every step as
//     pre-packed fragments (one global_load_dwordx4 per lane = 4 k-quads of one tile; 1 KiB per wave-instruction).
//   * act^T (B operand) lives in LDS k-major ([k][patient], leading dimension == 16 mod 32 so the 4x16 fragment
//     read is bank-conflict free), double buffered: x_t*mask_t for the next step is fetched from HBM (coalesced,
//     contiguous tile) while the current step's MFMAs run; h_t is written by the cell update.
// Algorithmic bytes per patient: 2*4*T*obs (x, mask) + 4*T*(I-obs) read, 8H written; with save_tape additionally
// 20*T*H written (activated gates + cell state per step, in the lane order the backward kernel reads them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/hode.h"
#include "hode_common.hpp"
#include "hode_host.hpp"

namespace hode {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LstmArgs {
  const float* __restrict__ x;
  const float* __restrict__ a;
  const float* __restrict__ mask;
  const float* __restrict__ wp;     // packed Wcat fragments [4][KQ4][TPW][64][4]; operand row I + Hp is the bias
  float* __restrict__ h_out;
  float* __restrict__ c_out;
  float* __restrict__ tape;         // [T][nblk][Hp/16 (unit tile = wave * TPW + tile of the wave)][NT][5][64] or nullptr
  int T, B, OBS, AD, I, H, Hp, Kq, KQ4, LD, reverse;
  unsigned long long* dbg;  // HODE_LSTM_STAMPS builds only: [T][8] s_memtime stamps of wave 0 of block 0
};

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope release over ALL address
// spaces, i.e. s_waitcnt vmcnt(0): every wave would sit out the HBM write burst of the step (tape stores in the forward,
// dG / h_prev rows in the BPTT -- 32 MB per step over the chip, written by all workgroups at the same moment) before the
// matrix pipe starts again.  Nothing in these kernels reads back what they store, so the stores may drain under the next
// step's MFMAs.
HODE_DEV void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

HODE_DEV float sigmoid_gate(float x) {
  // 1 / (1 + exp(-x)) on v_exp + v_rcp.  ABSOLUTE error: bound 1.9e-7, measured 1.0e-7 (tests/test_hip_helpers.py); in ulp
  // the error grows with |x| for x < 0 (the fp32 log2(e) and the rounded product: bound (5 + 1.23 |x|) ulp; measured 2.24 ulp
  // for |x| < 1, 9.04 ulp for |x| < 8, 61.9 ulp up to 87.3).  exp overflow -> rcp(inf) = 0, underflow -> 1; a result below 2^-126 is flushed to 0.
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// NW waves of TPW 16-row tiles each (NW * TPW * 16 = padded H).  Hp = 160 runs as 8 waves x 5 tiles: two waves per
// SIMD, every register in the 256-entry VGPR file -- with 4 x 10 the 120 accumulators went to the AGPR half and came
// back through v_accvgpr moves every step, the compiler spilled, and nothing covered a non-MFMA instruction.
// PAD: the hidden size is not a compiled one (H < Hp): the cell update zeroes h of the padded units H .. Hp - 1 by a select
// (hode_lstm_fwd_body.hpp says why).  A template parameter, so that the kernels of H == Hp (every shipped encoder) are the
// code they were: as a select on every store lstm_fwd_kernel ran 1.7 % longer at the benchmark's H = 160 (3.57 against
// 3.52 ms), as a pass of its own behind the update loop 3.2 %, as two copies of the body under a kernel-uniform branch 2.8 %.
// VEC4: obs_dim % 4 == 0 (x tile fetched in 16-byte groups).  A compile-time switch: as a run-time branch the flat
// path's per-element divisions are hoisted out of the step loop and pinned ~60 registers in every shipped shape.
//
// POLICY says what leaves the chip.  LstmFinalState: the state after the last step, h_out[B][H] (the encoder).
// LstmSequence: the hidden state of EVERY step, h_out[T][B][H] -- row t holds the state after consuming input row t, in
// either walking direction -- for a sequence-to-sequence LSTM (libhode_lstm_seq.so, include/hode_lstm_seq.h).  The rows
// are stored from the lanes' registers in the cell update: lane (g, pc) holds unit 4 tile + g of patient 16 c + pc, so
// the four lanes of a patient column write 16 contiguous bytes; nothing waits for these stores, they drain under the next
// step's MFMAs like the tape's.  (Read back along u, the k-major activation buffer puts a wave on two banks.)
//
// The body is csrc/hode_lstm_fwd_body.hpp (the BPTT's: hode_lstm_bwd_body.hpp), one text that each kernel definition
// includes under its `using POLICY = ...`.  Textual on purpose: as a __device__ template called from the two kernels the
// compiler scheduled every lstm_fwd_kernel instantiation differently from the build before the split (same flags, 0 of 8
// forward kernels of the TPW = 1 unit byte-identical); included, every kernel of libhode.so is byte-identical
// (profiles/lstm_seq_device_code_diff.txt), so its measured timings carry over.
struct LstmFinalState { static constexpr bool kAllSteps = false; };
struct LstmSequence { static constexpr bool kAllSteps = true; };

template <int NT, int TPW, int NW, bool VEC4, bool PAD>
__global__ __launch_bounds__(64 * NW) void lstm_fwd_kernel(LstmArgs p) {
  using POLICY = LstmFinalState;
#include "hode_lstm_fwd_body.hpp"
}

#ifdef HODE_LSTM_SEQ_UNIT
// libhode_lstm_seq.so only: p.h_out is [T][B][H]
template <int NT, int TPW, int NW, bool VEC4, bool PAD>
__global__ __launch_bounds__(64 * NW) void lstm_seq_fwd_kernel(LstmArgs p) {
  using POLICY = LstmSequence;
#include "hode_lstm_fwd_body.hpp"
}
#endif


// ---------------------------------------------------------------------------------------------------- backward
// Back-propagation through time of the recurrence.  Per step (walked in the reverse of the forward processing order)
//   dh = carry (+ grad_h_out at the last processed step);  tc = tanh(c_t)
//   d_o = dh tc o(1-o);  dc = carry_c + dh o (1 - tc^2);  d_i = dc g i(1-i);  d_f = dc c_prev f(1-f);  d_g = dc i (1-g^2)
//   carry_c = dc f;  carry_h[u'] = sum_rho W_hh[rho][u'] dG[rho]     <- the only contraction: fp32 MFMA
// The gate cotangents dG leave the kernel as grad_gates[T][B][4H] and the entering hidden state as h_prev[T][B][H]
// (both row-major, written coalesced through an LDS transpose); the weight gradients are then three plain GEMMs
// over K = T*B (dG^T x, dG^T h_prev, column sums), which the host wrapper hands to the BLAS library.
//
// MFMA mapping: out[u' (16 per tile) x patient] += W_hh^T[u' x rho] dG^T[rho x patient].  K (rho = gate rows) is
// split over the waves: wave w contracts over the gate rows of ITS units, i.e. exactly the dG values it has just
// produced.  With rho ordered (tile, gate, unit-in-tile) the B-operand fragment of k-quad (tile, gate) -- lane
// (k = lane>>4, j = lane&15) -- IS the register that lane already holds from the element-wise step: no staging.
// The four partial [H x BT] results are exchanged through LDS slabs and summed in a fixed order.
struct LstmBwdArgs {
  const float* __restrict__ tape;      // forward tape [T][nblk][4][TPW][NT][5][64]
  const float* __restrict__ whp;       // packed W_hh^T fragments [4][TPW(tau)][4 (gate row)][ceil(TPW/4)][64][4 (mt)]
  const float* __restrict__ grad_h_out;  // [B][H]; all-steps policy (lstm_seq_bwd_kernel): [T][B][H]
  float* __restrict__ grad_gates;      // [T][B][4H]
  float* __restrict__ h_prev;          // GEMM operand [T][B][W]: (OBS columns left to the caller: x*mask) | action columns
                                       // (AD) | hidden state entering the step (H) | 1.0 | zero padding to W
  const float* __restrict__ a;         // [T][B][AD] or nullptr
  int T, B, H, Hp, LD, reverse, AD, OBS, W;
  unsigned long long* dbg;  // HODE_LSTM_STAMPS builds only: [T][8] s_memtime stamps of wave 0 of block 0
};


#ifndef HODE_BPTT_BODY_HOOK
#define HODE_BPTT_BODY_HOOK 1
#endif
#ifndef HODE_BPTT_BURST
#define HODE_BPTT_BURST 1   // 1: element-wise burst, then the MFMAs with only loads between them; 0: 1 MFMA : 1-2 VALU interleave (3 % slower, tools/micro/mfma_valu_overlap.hip)
#endif
// FLAT: H == 16 TPW (no padded hidden units): the store phase copies whole dG rows (see there); a template parameter so
// that only one of the two store loops -- and its hoisted addresses -- exists in an instantiation
//
// POLICY (see the forward).  LstmSequence: every step has a cotangent of its own, dh = carry + grad_h_out[t]: the carry
// starts from the row of the last processed step, and after the slab fold of a step the row of the step processed NEXT in
// this walk is added.  That row is requested one patient column at a time between the slab writes and parked in LDS until
// the fold (hode_lstm_bwd_body.hpp says why there and not earlier: the tile loop leaves no registers); no load is consumed
// by the next instruction, which would be an HBM round trip per step.
template <int NT, int TPW, bool FLAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void lstm_bwd_kernel(LstmBwdArgs p) {
  using POLICY = LstmFinalState;
#include "hode_lstm_bwd_body.hpp"
}

#ifdef HODE_LSTM_SEQ_UNIT
// libhode_lstm_seq.so only: p.grad_h_out is [T][B][H]
template <int NT, int TPW, bool FLAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void lstm_seq_bwd_kernel(LstmBwdArgs p) {
  using POLICY = LstmSequence;
#include "hode_lstm_bwd_body.hpp"
}
#endif

// ---------------------------------------------------------------------------------------------------- launch geometry
struct LstmGeom {
  int Hp, TPW, NT, BT, nblk, Kq, KQ4, LD;
  int fTPW, fNW;   // the forward kernel's tiles per wave x waves (fTPW * fNW == TPW * 4)
  size_t wp_floats, tape_floats, whp_floats, lds_bytes, lds_bwd_bytes;
};

// Per-size entry points, one translation unit per TPW (csrc/hode_lstm_tpw.hip compiled with -DHODE_LSTM_TPW=<n>, so the
// hidden sizes build in parallel): padded H = 16 TPW.
#define HODE_LSTM_DECL(n)                                                                  \
  int lstm_fwd_tpw##n(const LstmGeom& G, const LstmArgs& a, hipStream_t s);               \
  int lstm_bwd_tpw##n(const LstmGeom& G, const LstmBwdArgs& a, hipStream_t s);
HODE_LSTM_DECL(1) HODE_LSTM_DECL(2) HODE_LSTM_DECL(3) HODE_LSTM_DECL(4) HODE_LSTM_DECL(5) HODE_LSTM_DECL(6) HODE_LSTM_DECL(8)
HODE_LSTM_DECL(10)
#undef HODE_LSTM_DECL

}  // namespace hode
