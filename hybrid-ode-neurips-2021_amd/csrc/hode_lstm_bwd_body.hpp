// The body of the LSTM BPTT kernels (hode_lstm_kernels.hpp), included once per kernel definition: lstm_bwd_kernel with
// `using POLICY = LstmFinalState`, lstm_seq_bwd_kernel with LstmSequence.  In scope where it is included: the template
// arguments NT, TPW, FLAT, the kernel argument `LstmBwdArgs p` and POLICY.  Not a header of its own: no include guard.
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int BT = 16 * NT;
  constexpr int Hp = 16 * TPW;
  constexpr int LDG = 4 * Hp + 4;   // row pitch of the dG transpose tile (pad: 2-way instead of 16-way conflicts)
  constexpr int LDH = Hp + 4;
  const int tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63;
  const int g = l >> 4, pc = l & 15;
  const int b0 = blockIdx.x * BT;
  const int nvalid = min(BT, p.B - b0);
  constexpr int LD = BT + ((BT % 32 == 0) ? 16 : 0);   // == p.LD (lstm_geom); compile-time: slab offsets become immediates
  float* dgt = lds;                      // [BT][LDG]   (time-shared with the partial slabs [4][Hp][LD])
  float* slab = lds;
  float* hT = lds + (size_t)BT * LDG;    // [BT][LDH]
  const int unit0 = __builtin_amdgcn_readfirstlane(w) * TPW * 4 + g;   // the lane's unit in tile 0 of its wave
  float* dg_lane = dgt + pc * LDG + unit0;
  float* hT_lane = hT + pc * LDH + unit0;
  float* slab_w = slab + (__builtin_amdgcn_readfirstlane(w) * Hp + 4 * g) * LD + pc;   // partial of wave w, rows 4g.., column pc
  const float* slab_r = slab + unit0 * LD + pc;
  const int H = p.H;

  float carry_h[TPW][NT], carry_c[TPW][NT];
#pragma unroll
  for (int tt = 0; tt < TPW; ++tt) {
    const int u = (w * TPW + tt) * 4 + g;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int b = 16 * c + pc;
      if constexpr (POLICY::kAllSteps) {
        const size_t t_last = p.reverse ? 0 : p.T - 1;   // time index of the first backward step
        carry_h[tt][c] = (u < H && b < nvalid) ? p.grad_h_out[(t_last * p.B + b0 + b) * H + u] : 0.f;
      } else {
        carry_h[tt][c] = (u < H && b < nvalid) ? p.grad_h_out[(size_t)(b0 + b) * H + u] : 0.f;
      }
      carry_c[tt][c] = 0.f;
    }
  }
  // wave-uniform bases (SGPRs) + one 32-bit lane offset: with per-lane 64-bit pointers the compiler hoists one address
  // pair per fragment out of the step loop (100 pairs for TPW = 10) and spills them
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const size_t tape_step = (size_t)gridDim.x * 4 * TPW * NT * 5 * 64;
  const size_t tape_blk = ((size_t)blockIdx.x * 4 + wu) * TPW * NT * 5 * 64;
  constexpr int MG = (TPW + 3) / 4;   // 16-byte weight groups per (tile, gate row)
  const f32x4* whb = reinterpret_cast<const f32x4*>(p.whp) + (size_t)wu * TPW * 4 * MG * 64;

  // Operands of one (step, unit tile): the step's activated gates and cell state and the previous step's cell state
  // and output gate for NT patient columns (TapeOps), and the TPW weight fragments the tile's MFMAs read.
  //
  // Software pipeline over the unit tiles of a step (fully unrolled, register sets alternate by renaming):
  //   body(tt) = [tape loads of tile tt+2] [weight loads of tile tt+1] [element-wise step of tile tt+1] [MFMAs of tile tt]
  // The element-wise step of the NEXT tile and the matrix products of THIS one are independent and sit in one basic
  // block, interleaved one VALU group per MFMA: with one wave per SIMD nothing else fills the matrix pipe while the
  // wave does VALU work (26 us per step for 16 us of MFMA time when each tile ran element-wise -> MFMAs in sequence).
  // A load consumed by the next instruction costs an HBM / L2 round trip per tile, hence the two-tile tape distance.
  struct TapeOps { float gi[NT], gf[NT], gg[NT], go[NT], cn[NT], cp[NT], op[NT]; };
  // All tape and weight loads are BUFFER loads: 4-SGPR resource (rebuilt per step with scalar instructions) + one lane
  // offset register + scalar / immediate offsets.  With global loads the compiler kept one 64-bit VGPR address per 4 KiB
  // window (19 pairs) and, behind the pointer laundering that stops it hoisting 100 fragment addresses, fell back to
  // FLAT loads for the weights (they count on lgkmcnt as well as vmcnt: a wait for an LDS write became a wait for L2).
  auto rsrc_of = [](const void* ptr) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, 0x7fffffff, 0x00020000);  // raw, dword format
  };
  auto ldf = [&](__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, l * 4, byte_off, 0));
  };
  auto step_ptrs = [&](int s, const float*& tc, const float*& tpv) {
    const int t = p.reverse ? p.T - 1 - s : s;
    const int t_prev = p.reverse ? t + 1 : t - 1;  // time index processed one step earlier in the forward sweep
    tc = p.tape + (size_t)t * tape_step + tape_blk;
    tpv = (s > 0) ? p.tape + (size_t)t_prev * tape_step + tape_blk : tc;  // s == 0: dummy reads, masked by has_prev
  };
  auto load_tape_col = [&](TapeOps& o, __amdgpu_buffer_rsrc_t rc, __amdgpu_buffer_rsrc_t rp, int tt, int c) {
    const int q5 = (tt * NT + c) * 5 * 64 * 4;   // byte offset of the (tile, column) record: [gi | gf | gg | go | c][64]
    o.gi[c] = ldf(rc, q5); o.gf[c] = ldf(rc, q5 + 256); o.gg[c] = ldf(rc, q5 + 512); o.go[c] = ldf(rc, q5 + 768);
    o.cn[c] = ldf(rc, q5 + 1024);
    o.cp[c] = ldf(rp, q5 + 1024); o.op[c] = ldf(rp, q5 + 768);
  };
  auto load_tape = [&](TapeOps& o, __amdgpu_buffer_rsrc_t rc, __amdgpu_buffer_rsrc_t rp, int tt) {
#pragma unroll
    for (int c = 0; c < NT; ++c) load_tape_col(o, rc, rp, tt, c);
  };
  const __amdgpu_buffer_rsrc_t wrs = rsrc_of(whb);
  // weights of row block R = 4 * tile + gate row
  auto load_w = [&](f32x4 (&wf)[MG], int R) {
#pragma unroll
    for (int j = 0; j < MG; ++j)
      wf[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, l * 16, (R * MG + j) * 64 * 16, 0));
  };
  TapeOps ops[2];          // tile tt lives in ops[tt & 1]: during body(tt) the sets hold tiles tt+1 (consumed) and tt+2 (in flight)
  f32x4 wfr[3][MG];        // row block R = 4 tt + r in wfr[R % 3], loaded two blocks (60 NT/3 MFMAs) ahead
  float dgr[2][NT][4];     // tile tt's gate cotangents (the MFMA B operands) in dgr[tt & 1]
  {
    const float *tc0, *tpv0;
    step_ptrs(p.T - 1, tc0, tpv0);
    load_tape(ops[0], rsrc_of(tc0), rsrc_of(tpv0), 0);
    load_tape(ops[1], rsrc_of(tc0), rsrc_of(tpv0), TPW > 1 ? 1 : 0);
    load_w(wfr[0], 0);
    load_w(wfr[1], 1);
  }

#ifdef HODE_LSTM_STAMPS
#define HODE_LSTAMP(i) if (p.dbg && blockIdx.x == 0 && tid == 0) { __builtin_amdgcn_s_waitcnt(0); p.dbg[(size_t)s * 8 + (i)] = __builtin_amdgcn_s_memtime(); }
#else
#define HODE_LSTAMP(i)
#endif
  const int nA0 = nvalid * p.AD;
  const int act_b = p.AD > 0 ? tid / max(p.AD, 1) : 0, act_u = tid - act_b * p.AD;
  float a_nx = 0.f;
  if (p.a && nA0 <= 256 && tid < nA0) {
    const int t0 = p.reverse ? 0 : p.T - 1;   // time index of the first backward step (s = T - 1)
    a_nx = p.a[((size_t)t0 * p.B + b0) * p.AD + tid];
  }
  for (int s = p.T - 1; s >= 0; --s) {
    const int t = p.reverse ? p.T - 1 - s : s;
    HODE_LSTAMP(0)
    const float *tc, *tpv, *tc_n, *tpv_n;
    step_ptrs(s, tc, tpv);
    step_ptrs(s > 0 ? s - 1 : 0, tc_n, tpv_n);  // next step's first tiles (s == 0: a harmless repeat)
    const float has_prev = s > 0 ? 1.0f : 0.0f;
    const __amdgpu_buffer_rsrc_t rs_c = rsrc_of(tc), rs_p = rsrc_of(tpv), rs_cn = rsrc_of(tc_n), rs_pn = rsrc_of(tpv_n);

    f32x4 acc[TPW][NT];
#pragma unroll
    for (int mt = 0; mt < TPW; ++mt)
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The columns of the GEMM operand row that do not depend on the recurrence -- the action columns (a copy of an input),
    // the constant 1 of the bias column, the zero padding -- are written HERE, ahead of the tile loop: inside the store
    // phase each patient's action copy was a dependent global load -> store (12 serial HBM round trips per wave and step,
    // 5.8 us of a 36.6 us step; tools/lstm_stamp_probe.py).
    {
      const int W = p.W, I = p.OBS + p.AD;
      float* hdst = p.h_prev + ((size_t)t * p.B + b0) * W;
      const float* asrc = p.a ? p.a + ((size_t)t * p.B + b0) * p.AD : nullptr;
      const int nA = nvalid * p.AD, nP = nvalid * (W - I - H);
      if (nA <= 256) {
        // one action value per thread, loaded ONE STEP AHEAD (a_nx): a load consumed by the next store stalls its wave for an
        // HBM round trip at the head of the step, and the whole workgroup waits for that wave at the end of the tile loop
        if (tid < nA) hdst[(size_t)act_b * W + p.OBS + act_u] = a_nx;
        if (s > 0 && tid < nA) {
          const int t_n = p.reverse ? p.T - s : s - 1;   // time index of backward step s - 1
          a_nx = p.a[((size_t)t_n * p.B + b0) * p.AD + tid];
        }
      } else {
        for (int e = tid; e < nA; e += 256) {
          const int b = e / p.AD, u = e - b * p.AD;
          hdst[(size_t)b * W + p.OBS + u] = asrc[e];
        }
      }
      for (int e = tid; e < nP; e += 256) {
        const int b = e / (W - I - H), u = e - b * (W - I - H);
        hdst[(size_t)b * W + I + H + u] = u == 0 ? 1.0f : 0.0f;
      }
    }

    // element-wise step of tile tt: gate cotangents -> dgr[tt & 1] (+ the transposed copies for the row-major stores)
    auto elementwise = [&](int tt, const TapeOps& o, float (&dg)[NT][4]) {
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        const float gi = o.gi[c], gf = o.gf[c], gg = o.gg[c], go = o.go[c], cn = o.cn[c];
        const float c_prev = has_prev * o.cp[c];
        const float h_prev = has_prev * (o.op[c] * tanh_f32(c_prev));
        const float tcn = tanh_f32(cn);
        const float dh = carry_h[tt][c];
        const float dc = __builtin_fmaf(dh * go, __builtin_fmaf(-tcn, tcn, 1.0f), carry_c[tt][c]);
        dg[c][0] = dc * gg * gi * (1.0f - gi);
        dg[c][1] = dc * c_prev * gf * (1.0f - gf);
        dg[c][2] = dc * gi * __builtin_fmaf(-gg, gg, 1.0f);
        dg[c][3] = dh * tcn * go * (1.0f - go);
        carry_c[tt][c] = dc * gf;
        // lane base + compile-time offset: (patient 16c + pc, unit (w TPW + tt) 4 + g).  Written as one index
        // expression the compiler hoisted one address per (tile, column, gate) out of the step loop and spilled them.
#pragma unroll
        for (int r = 0; r < 4; ++r) dg_lane[16 * c * LDG + r * Hp + 4 * tt] = dg[c][r];
        hT_lane[16 * c * LDH + 4 * tt] = h_prev;
      }
    };
    // body(tt): row block r of the tile = TPW * NT MFMAs.  The tape operands of tile tt + 2 are requested in the first
    // MFMAs of the body (they are needed from the start of the next body: one body = 1.6 us of latency cover), the
    // weights of row block R + 2 at the start of row block R; the group barriers below pin that issue order (left to
    // itself the scheduler sinks every load next to its use, and an in-order vmcnt wait on the newest load waits for all).
    auto body = [&](int tt) {
#if defined(HODE_LSTM_STAMPS) || HODE_BPTT_BODY_HOOK
      // In product builds p.dbg is null and this is a never-taken branch -- KEPT ON PURPOSE: it ends the basic block at every
      // unit tile.  Without it the ten bodies of a step are one block and the kernel is 0.47 ms (15 %) slower at the bench
      // shape (same-call A/B of the two builds, tools/lstm_time_probe.py): the scheduler's / waitcnt pass's choices over a
      // 3 000-instruction block undo part of the issue order pinned below.
      if (p.dbg && blockIdx.x == 0 && tid == 0) p.dbg[(size_t)(p.T + s) * 16 + tt] = __builtin_amdgcn_s_memtime();  // no wait
#endif
      TapeOps& o_nx = ops[tt & 1];
      const bool same_step = tt + 2 < TPW;
      const int tile_nx = same_step ? tt + 2 : min(tt + 2 - TPW, TPW - 1);
      load_w(wfr[(4 * tt + 2) % 3], (4 * tt + 2) % (4 * TPW));
      if (same_step) load_tape(o_nx, rs_c, rs_p, tile_nx);
      else load_tape(o_nx, rs_cn, rs_pn, tile_nx);
      if (tt + 1 < TPW) elementwise(tt + 1, ops[(tt + 1) & 1], dgr[(tt + 1) & 1]);
      if (HODE_BPTT_BURST) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = 4 * tt + r;
        if (r > 0) load_w(wfr[(R + 2) % 3], (R + 2) % (4 * TPW));   // past the step's last block: the next step's first two
#pragma unroll
        for (int mt = 0; mt < TPW; ++mt)
#pragma unroll
          for (int c = 0; c < NT; ++c)
            acc[mt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wfr[R % 3][mt >> 2][mt & 3], dgr[tt & 1][c][r], acc[mt][c], 0, 0, 0);
      }
      // issue pipeline of the block: per MFMA one or two VALU of the next tile's element-wise step, the loads in the
      // first MFMAs of each row block, one LDS write every 8 MFMAs
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        constexpr int MF = TPW * NT;
        const int n_loads = HODE_BPTT_BURST ? (r == 0 ? 0 : MG) : MG + (r == 0 ? 7 * NT : 0);
#pragma unroll
        for (int i = 0; i < MF; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                              // 1 MFMA
          if (i < n_loads) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);             // 1 VMEM read
          if (tt + 1 < TPW && !HODE_BPTT_BURST) {
            if (i & 1) __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);                 // 1 VALU
            else __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                       // 2 VALU
            if ((i & 7) == 7) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);          // 1 LDS write
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    elementwise(0, ops[0], dgr[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) body(tt);
    // canonical register sets for the next step: its tile 0 -> ops[0], its tile 1 -> ops[1], its row blocks 0, 1 ->
    // wfr[0], wfr[1]
    if constexpr ((TPW & 1) && TPW > 1) {   // TPW == 1: the only body loads the next step's tile 0 straight into ops[0]
      const TapeOps t0 = ops[1], t1 = ops[0];
      ops[0] = t0; ops[1] = t1;
    }
    if constexpr ((4 * TPW) % 3 != 0) {
      f32x4 n0[MG], n1[MG];
#pragma unroll
      for (int j = 0; j < MG; ++j) { n0[j] = wfr[(4 * TPW) % 3][j]; n1[j] = wfr[(4 * TPW + 1) % 3][j]; }
#pragma unroll
      for (int j = 0; j < MG; ++j) { wfr[0][j] = n0[j]; wfr[1][j] = n1[j]; }
    }
    HODE_LSTAMP(1)
    lds_barrier();
    HODE_LSTAMP(2)
    // coalesced row-major stores of this step's dG and h_prev tiles.  Wave w stores patients w, w+4, ...; the loops run
    // over (patient, gate, unit) explicitly -- a flat index would need two integer divisions per element, which made
    // this transposition the longest phase of the step (120 iterations x ~70 instructions per thread).
    {
      float* gdst = p.grad_gates + ((size_t)t * p.B + b0) * 4 * H;
      const int W = p.W, I = p.OBS + p.AD;
      float* hdst = p.h_prev + ((size_t)t * p.B + b0) * W;
      const float* asrc = p.a ? p.a + ((size_t)t * p.B + b0) * p.AD : nullptr;
      // The LDS reads of a patient's rows are all issued before the first store (and two patients are in flight): with one
      // ds_read -> wait -> global_store chain per 16 bytes this phase was LDS-LATENCY bound -- 84 dependent round trips per
      // wave and step, 8.6 us of a 36.6 us step (tools/lstm_stamp_probe.py) -- not bandwidth bound.
      const bool vec = (H & 3) == 0;
      const bool lane_g = 4 * l < H;           // H <= 160: one 16-byte chunk per lane and gate row covers a row
      if constexpr (FLAT) {
        // H a multiple of 16 (every shipped encoder): a patient's dG row is 4H contiguous floats in LDS and in HBM -- a flat
        // copy in 16-byte chunks over ALL 64 lanes (ceil(H/64) instructions instead of 4 with 4H/16 <= 40 lanes busy), software
        // pipelined: the LDS reads of the wave's next patient are in flight while this patient's stores issue
        constexpr int NC = (Hp + 63) / 64;       // 16-byte chunks of the dG row per lane
        constexpr int NHC = (Hp + 63) / 64;      // floats of the h_prev row per lane
        struct Row { f32x4 v[NC]; float h[NHC]; };
        auto ld = [&](int b, Row& r) {
          const float* drow = dgt + (size_t)b * LDG;
          const float* hrow = hT + (size_t)b * LDH;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int f = l + 64 * c;
            r.v[c] = f < Hp ? *reinterpret_cast<const f32x4*>(drow + 4 * f) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int k = 0; k < NHC; ++k) r.h[k] = (l + 64 * k < H) ? hrow[l + 64 * k] : 0.f;
        };
        auto st = [&](int b, const Row& r) {
          float* grow = gdst + (size_t)b * 4 * H;
          float* hd = hdst + (size_t)b * W + I;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int f = l + 64 * c;
            if (f < Hp) *reinterpret_cast<f32x4*>(grow + 4 * f) = r.v[c];
          }
#pragma unroll
          for (int k = 0; k < NHC; ++k)
            if (l + 64 * k < H) hd[l + 64 * k] = r.h[k];
        };
        Row ra, rb;
        int b = w;
        if (b < nvalid) ld(b, ra);
        for (; b < nvalid; b += 8) {
          if (b + 4 < nvalid) ld(b + 4, rb);
          __builtin_amdgcn_sched_barrier(0);   // the next patient's reads stay ahead of this patient's stores
          st(b, ra);
          if (b + 4 < nvalid) {
            if (b + 8 < nvalid) ld(b + 8, ra);
            __builtin_amdgcn_sched_barrier(0);
            st(b + 4, rb);
          }
        }
      } else
      for (int b = w; b < nvalid; b += 8) {
        const int b2 = b + 4;
        const bool two = b2 < nvalid;
        const float* drow = dgt + (size_t)b * LDG;
        const float* drow2 = dgt + (size_t)(two ? b2 : b) * LDG;
        const float* hrow = hT + (size_t)b * LDH;
        const float* hrow2 = hT + (size_t)(two ? b2 : b) * LDH;
        f32x4 v[4], v2[4];
        float hv[3], hv2[3];
        if (vec) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[r] = lane_g ? *reinterpret_cast<const f32x4*>(drow + r * Hp + 4 * l) : f32x4{0.f, 0.f, 0.f, 0.f};
            v2[r] = lane_g ? *reinterpret_cast<const f32x4*>(drow2 + r * Hp + 4 * l) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          hv[k] = (l + 64 * k < H) ? hrow[l + 64 * k] : 0.f;
          hv2[k] = (l + 64 * k < H) ? hrow2[l + 64 * k] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the reads above the stores
        auto put = [&](int bb, const float* dr, const f32x4 (&vv)[4], const float (&hh)[3]) {
          float* grow = gdst + (size_t)bb * 4 * H;
          if (vec) {
            if (lane_g) {
#pragma unroll
              for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(grow + r * H + 4 * l) = vv[r];
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              for (int u = l; u < H; u += 64) grow[r * H + u] = dr[r * Hp + u];
          }
          float* hd = hdst + (size_t)bb * W;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (l + 64 * k < H) hd[I + l + 64 * k] = hh[k];
        };
        put(b, drow, v, hv);
        if (two) put(b2, drow2, v2, hv2);
      }
    }
    HODE_LSTAMP(3)
    lds_barrier();
    HODE_LSTAMP(4)
    // exchange the K-split partial products: slab[w][u'][patient]
    float* park_lane = nullptr;   // all-steps policy only
    if constexpr (!POLICY::kAllSteps) {
#pragma unroll
    for (int mt = 0; mt < TPW; ++mt)
#pragma unroll
      for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          slab_w[(16 * mt + rr) * LD + 16 * c] = acc[mt][c][rr];
    } else {
      auto slab_put = [&](int mt) {   // the loop above, one output tile at a time
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            slab_w[(16 * mt + rr) * LD + 16 * c] = acc[mt][c][rr];
      };
      // All-steps policy: the cotangent row of backward step s - 1, added after this step's slab fold.  The loop runs at the
      // limit of the register file (TPW = 10, NT = 3: 6 of 512 left), so the row never sits in TPW * NT registers: one
      // patient column (TPW values) at a time is requested, a share of the slab writes covers its round trip, and it is
      // parked RAW in the BT * LDH floats that lstm_geom allocates past max(dG tile, slabs) -- the h_prev transpose tile
      // where the slabs end below it, the floats behind the slabs where they cover it (NT = 2); free from the store phase to
      // the next step's element-wise pass -- where the lane reads it back itself at the fold (no barrier involved).
      // Nothing consumes a loaded value before it is parked: a padded unit is zeroed at the fold, not here.
      // Addressing: one buffer resource PER PATIENT COLUMN over the column's valid patients (base = row t_n, patient
      // b0 + 16 c; max(0, nvalid - 16 c) * H * 4 bytes) and the whole offset, lane part + 16 tt, in the VGPR offset, the
      // operand the hardware range-checks (the scalar offset operand takes no part in that check): a patient past the batch
      // and a padded unit of the column's last patient are out of range and read 0, never memory behind the tensor; a padded
      // unit of any other patient reads the next patient's row, which the fold's select discards.
      const int sn = s > 0 ? s - 1 : 0;             // s == 0: a harmless repeat, never consumed
      const int t_n = p.reverse ? p.T - 1 - sn : sn;
      const float* grow = p.grad_h_out + ((size_t)t_n * p.B + b0) * H;   // wave-uniform
      const int lane_off = (pc * H + unit0) * 4;
      constexpr int kPark = BT * LDG > 4 * Hp * LD ? BT * LDG : 4 * Hp * LD;   // lstm_geom: the allocation is kPark + BT * LDH floats
      park_lane = lds + kPark + pc * LDH + unit0;
      float ghc[2][TPW];
      auto gh_load = [&](float (&dst)[TPW], int c) {
        const int rows = max(nvalid - 16 * c, 0);
        const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grow + (size_t)16 * c * H), 0,
                                                                              rows * H * 4, 0x00020000);
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt)
          dst[tt] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, lane_off + 16 * tt, 0, 0));
      };
      auto gh_park = [&](const float (&src)[TPW], int c) {
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) park_lane[16 * c * LDH + 4 * tt] = src[tt];
      };
      gh_load(ghc[0], 0);
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = c * TPW / NT; mt < (c + 1) * TPW / NT; ++mt) slab_put(mt);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < NT) gh_load(ghc[(c + 1) & 1], c + 1);
        gh_park(ghc[c & 1], c);
      }
    }
    HODE_LSTAMP(5)
    lds_barrier();
    HODE_LSTAMP(6)
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) {
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        const float* sp = slab_r + 4 * tt * LD + 16 * c;
        carry_h[tt][c] = ((sp[0] + sp[Hp * LD]) + sp[2 * Hp * LD]) + sp[3 * Hp * LD];
        if constexpr (POLICY::kAllSteps) {
          const float gh = park_lane[16 * c * LDH + 4 * tt];
          carry_h[tt][c] += (FLAT || unit0 + 4 * tt < H) ? gh : 0.f;   // a padded unit's slot holds the next patient's value
        }
      }
    }
    HODE_LSTAMP(7)
    lds_barrier();
  }
#undef HODE_LSTAMP
