// The body of the LSTM window kernels (hode_lstm_kernels.hpp), included once per kernel definition: lstm_fwd_kernel with
// `using POLICY = LstmFinalState`, lstm_seq_fwd_kernel with LstmSequence.  In scope where it is included: the template
// arguments NT, TPW, NW, VEC4, PAD, the kernel argument `LstmArgs p` and POLICY; PAD: the hidden size is not a compiled
// one, units H .. Hp - 1 are padding.  Not a header of its own: no include guard.
  constexpr int NTHR = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int BT = 16 * NT;
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;  // w in an SGPR: per-wave bases stay scalar
  const int g = l >> 4, pc = l & 15;
  const int b0 = blockIdx.x * BT;
  const int nvalid = min(BT, p.B - b0);
  // compile-time leading dimension (== p.LD, lstm_geom): LDS offsets of the unrolled tile loops become instruction
  // immediates instead of one hoisted address register per (tile, patient column, buffer)
  constexpr int LD = BT + ((BT % 32 == 0) ? 16 : 0);
  const int Krows = 4 * p.Kq;                  // rows of one activation buffer (zero padded past I + Hp)
  float* act0 = lds;
  float* act1 = lds + (size_t)Krows * LD;

  // zero both activation buffers (h_{-1} = 0, padding rows/columns stay 0 forever); row I + Hp is the bias row: ones
  const int one_row = p.I + p.Hp;
  for (int e = tid; e < 2 * Krows * LD; e += NTHR) {
    const int r = (e / LD) % Krows;
    lds[e] = r == one_row ? 1.f : 0.f;
  }

  float cst[TPW][NT];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int c = 0; c < NT; ++c) cst[t][c] = 0.f;

  // x tile staging: the tile of one step is BT*OBS contiguous floats (patients are contiguous in [T][B][OBS]).
  // OBS % 4 == 0 (every shipped shape): a thread owns 16-byte groups (patient b = idx % BT, group idx / BT) -- consecutive
  // lanes are consecutive PATIENTS, so the k-major LDS writes are conflict free (the flat element order wrote a wave's
  // 64 values into 2 banks) and no run-time division is needed; the 16-byte loads walk every cache line four times
  // within the step, which L1 / L2 absorb.  Otherwise: flat element order, one division per element.
  // The loads are UNCONDITIONAL (slots past the tile read element 0 and are zeroed when staged) and x * mask is formed
  // when the tile is staged, not when it is fetched: a guarded load followed by the product is one basic block with a
  // vmcnt(0) per 16-byte group -- five serialised HBM round trips (6 us) in front of every step's first MFMA.
  constexpr int XPT = NW == 8 ? 12 : 20;  // staged floats per thread (XPT * NTHR covers BT*OBS <= 5120; multiple of 4)
  const int n_x = nvalid * p.OBS;
  constexpr bool vec4 = VEC4;
  const int Q4 = p.OBS >> 2;
  const bool has_mask = p.mask != nullptr;
  float xs[XPT], ms[XPT];
  auto fetch_x = [&](int t) {
    const size_t base = ((size_t)t * p.B + b0) * p.OBS;
    const float* xb = p.x + base;
    const float* mb = has_mask ? p.mask + base : xb;   // no mask: the second load repeats the first (L1 hit), never used
    if constexpr (vec4) {
#pragma unroll
      for (int j = 0; j < XPT / 4; ++j) {
        const int idx = tid + NTHR * j;
        const int b = idx % BT, i4 = idx / BT;
        const int off = (i4 < Q4 && b < nvalid) ? b * p.OBS + 4 * i4 : 0;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + off);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mb + off);
        xs[4 * j] = v[0]; xs[4 * j + 1] = v[1]; xs[4 * j + 2] = v[2]; xs[4 * j + 3] = v[3];
        ms[4 * j] = m[0]; ms[4 * j + 1] = m[1]; ms[4 * j + 2] = m[2]; ms[4 * j + 3] = m[3];
      }
    } else {
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        const int e = tid + NTHR * j;
        const int off = e < n_x ? e : 0;
        xs[j] = xb[off];
        ms[j] = mb[off];
      }
    }
  };
  auto stage_x = [&](float* dst, int t) {
    if constexpr (vec4) {
#pragma unroll
      for (int j = 0; j < XPT / 4; ++j) {
        const int idx = tid + NTHR * j;
        const int b = idx % BT, i4 = idx / BT;
        if (i4 < Q4) {
          const bool live = b < nvalid;  // zeros for patients past the batch
#pragma unroll
          for (int c = 0; c < 4; ++c)
            dst[(4 * i4 + c) * LD + b] = live ? (has_mask ? xs[4 * j + c] * ms[4 * j + c] : xs[4 * j + c]) : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        const int e = tid + NTHR * j;
        if (e < n_x) {
          const int b = e / p.OBS, i = e - b * p.OBS;
          dst[i * LD + b] = has_mask ? xs[j] * ms[j] : xs[j];
        }
      }
    }
    // action columns (never masked): AD * nvalid values
    for (int e = tid; e < nvalid * p.AD; e += NTHR) {
      const int b = e / p.AD, i = e - b * p.AD;
      dst[(p.OBS + i) * LD + b] = p.a[((size_t)t * p.B + b0 + b) * p.AD + i];
    }
  };

  const int t_first = p.reverse ? p.T - 1 : 0;
  fetch_x(t_first);
  __syncthreads();  // zero fill done
  stage_x(act0, t_first);
  __syncthreads();

  const f32x4* wbase = reinterpret_cast<const f32x4*>(p.wp) + (size_t)w * p.KQ4 * TPW * 64;  // wave-uniform; lane index added per load
  // weight fragment registers live across steps: the first group of step s+1 is requested as soon as step s's MFMA loop
  // ends, so its L2 round trip runs under the cell update, the x staging and the barrier
  f32x4 wa[TPW], wb[TPW];
#pragma unroll
  for (int tt = 0; tt < TPW; ++tt) wa[tt] = wbase[tt * 64 + l];

#ifdef HODE_LSTM_STAMPS
#define HODE_FSTAMP(i) if (p.dbg && blockIdx.x == 0 && tid == 0) { __builtin_amdgcn_s_waitcnt(0); p.dbg[(size_t)s * 8 + (i)] = __builtin_amdgcn_s_memtime(); }
// no-wait stamps inside the MFMA section: slot [T + s][16]
#define HODE_GSTAMP(i) if (p.dbg && blockIdx.x == 0 && tid == 0) p.dbg[(size_t)(p.T + s) * 16 + (i)] = __builtin_amdgcn_s_memtime();
#else
#define HODE_FSTAMP(i)
#define HODE_GSTAMP(i)
#endif
  for (int s = 0; s < p.T; ++s) {
    const int t = p.reverse ? p.T - 1 - s : s;
    HODE_FSTAMP(0)
    float* cur = (s & 1) ? act1 : act0;
    float* nxt = (s & 1) ? act0 : act1;
    const bool more = s + 1 < p.T;
    const int t_next = p.reverse ? t - 1 : t + 1;
    if (more) fetch_x(t_next);  // HBM loads in flight under the MFMA loop

    f32x4 acc[TPW][NT];
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt)
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[tt][c] = f32x4{0.f, 0.f, 0.f, 0.f};  // the bias arrives through the ones row

    // software-pipelined weight fragments: group q+1 is loaded while group q feeds the matrix pipe.  The loop over
    // full groups (4 k-quads each) is branch-free; the partial last group is peeled -- with a conditional per k-quad
    // inside the loop the waitcnt pass falls back to vmcnt(0) at every quad, i.e. it waits for the prefetch it has just
    // issued (one L2 round trip per group, 16 per step).
    // B fragments (one LDS row per patient column) are read one k-quad ahead: read-then-use in front of every 30-MFMA
    // block would expose the LDS latency 61 times per step
    auto load_group0 = [&](f32x4 (&wf)[TPW]) {
#pragma unroll
      for (int tt = 0; tt < TPW; ++tt) wf[tt] = wbase[tt * 64 + l];
    };
    // Nothing in the loop copies a register: weight fragments alternate between wa / wb over PAIRS of groups and the B
    // fragments between bf / bn over pairs of k-quads -- with one wave per SIMD nothing else covers an instruction
    // that is not an MFMA, and the 40 + 12 moves, the 10 loads and their addresses cost 500 cycles per group (13 %)
    // when they sat between the MFMA blocks.  The prefetch loads are pinned one in front of every 3 MFMAs of the
    // group's first k-quad, where they issue while the matrix pipe is busy.
    float bf[NT], bn[NT];
    const int last_quad = p.Kq - 1;
    auto read_b = [&](float (&dst)[NT], int quad) {
      const float* rowp = cur + (size_t)(4 * min(quad, last_quad) + g) * LD + pc;
#pragma unroll
      for (int c = 0; c < NT; ++c) dst[c] = rowp[16 * c];
    };
    read_b(bf, 0);
    // one full group: 4 k-quads out of wf, B fragments bf -> bn -> bf -> bn -> bf; wn <- group qn during k-quad 0
    auto group4 = [&](const f32x4 (&wf)[TPW], f32x4 (&wn)[TPW], int q, int qn) {
      const f32x4* wq = wbase + (size_t)qn * TPW * 64;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float (&bc)[NT] = (kk & 1) ? bn : bf;
        float (&bx)[NT] = (kk & 1) ? bf : bn;
        read_b(bx, 4 * q + kk + 1);
        __builtin_amdgcn_sched_barrier(0);  // keep the read HERE: the scheduler would sink it next to its use
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) {
          if (kk == 0) wn[tt] = wq[tt * 64 + l];
#pragma unroll
          for (int c = 0; c < NT; ++c)
            acc[tt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[tt][kk], bc[c], acc[tt][c], 0, 0, 0);
        }
        if (kk == 0) {
#pragma unroll
          for (int tt = 0; tt < TPW; ++tt) {
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // one weight load ...
            __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);  // ... per NT MFMAs
          }
        }
      }
    };
    // the partial last group (its fragments are zero padded): once per step, moves do not matter here
    auto group_tail = [&](const f32x4 (&wf)[TPW], int q, int n) {
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        if (kk < n) {
          read_b(bn, 4 * q + kk + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int tt = 0; tt < TPW; ++tt)
#pragma unroll
            for (int c = 0; c < NT; ++c)
              acc[tt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[tt][kk], bf[c], acc[tt][c], 0, 0, 0);
#pragma unroll
          for (int c = 0; c < NT; ++c) bf[c] = bn[c];
        }
      }
    };
    const int n_full = p.Kq >> 2;        // groups with all 4 k-quads
    const int tail = p.Kq & 3;           // k-quads of the last, partial group
    const int n_groups = n_full + (tail ? 1 : 0);
    int q = 0;
    HODE_GSTAMP(10)
    for (; q + 2 <= n_full; q += 2) {
      HODE_GSTAMP(q >> 1)
      group4(wa, wb, q, q + 1);
      group4(wb, wa, q + 1, min(q + 2, n_groups - 1));  // clamped: the last prefetch may be a repeat, never out of bounds
    }
    HODE_GSTAMP(8)
    // wa holds group q; the step's last prefetch goes to group 0 of the next step (weights do not change in the launch)
    if (n_full & 1) {
      group4(wa, wb, q, tail ? n_full : 0);
      if (tail) {
        group_tail(wb, n_full, tail);
        load_group0(wa);
      } else {
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) wa[tt] = wb[tt];
      }
    } else {
      if (tail) group_tail(wa, n_full, tail);
      load_group0(wa);
    }
    HODE_GSTAMP(9)
    HODE_FSTAMP(1)

    // cell update: lane (g, pc) holds gates i,f,g,o of unit u = (w*TPW + tt)*4 + g for patient 16c + pc
    float* nxt_lane = nxt + (p.I + w * TPW * 4 + g) * LD + pc;   // lane base; tile / column offsets are immediates
    float* tp = p.tape ? p.tape + (((size_t)t * gridDim.x + blockIdx.x) * NW + w) * TPW * NT * 5 * 64 : nullptr;  // wave-uniform
    // all-steps policy: row t of h_out, this workgroup's patients (wave-uniform) + the lane's (patient pc, unit 4 w TPW + g)
    float* hs_lane = nullptr;
    if constexpr (POLICY::kAllSteps) hs_lane = p.h_out + ((size_t)t * p.B + b0) * p.H + (pc * p.H + w * TPW * 4 + g);
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) {
      const int u = (w * TPW + tt) * 4 + g;
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        const float gi = sigmoid_gate(acc[tt][c][0]);
        const float gf = sigmoid_gate(acc[tt][c][1]);
        const float gg = tanh_f32(acc[tt][c][2]);
        const float go = sigmoid_gate(acc[tt][c][3]);
        const float cn = __builtin_fmaf(gf, cst[tt][c], gi * gg);
        const float hn = go * tanh_f32(cn);
        cst[tt][c] = cn;
        // PAD (H < Hp): a padded unit (u >= H: zero weights, zero bias) stores an exact zero, by a select.  Its
        // pre-activations are 0 * act, which is NaN, not 0, for a patient whose measurement or action is infinite, and the
        // next step would multiply that h by the zero-padded W_hh column -- 0 * NaN -- into every real unit of the patient,
        // where the gates of the real units only saturate (sigmoid -> 0 / 1, tanh -> +-1) and h stays finite
        nxt_lane[4 * tt * LD + 16 * c] = (PAD && u >= p.H) ? 0.f : hn;
        if constexpr (POLICY::kAllSteps) {
          if (u < p.H && 16 * c + pc < nvalid) hs_lane[16 * c * p.H + 4 * tt] = hn;   // padded units, patients past the batch: never written
        }
        if (tp) {
          float* q5 = tp + (tt * NT + c) * 5 * 64;
          q5[l] = gi; q5[64 + l] = gf; q5[128 + l] = gg; q5[192 + l] = go; q5[256 + l] = cn;
        }
      }
      // one tile's NT patient columns at a time: interleaving all TPW * NT exp / rcp chains costs more registers than
      // the file has next to the accumulators (the other wave of the SIMD covers the latency instead)
      __builtin_amdgcn_sched_barrier(0);
    }
    HODE_FSTAMP(2)
    if (more) stage_x(nxt, t_next);
    HODE_FSTAMP(3)
    lds_barrier();
    HODE_FSTAMP(4)
  }
#undef HODE_FSTAMP
#undef HODE_GSTAMP

  // final state: h_T is what the last step left in its output buffer (each lane reads back its own values); with the
  // all-steps policy h_T already is the last processed row of h_out
  const float* fin = (p.T & 1) ? act1 : act0;
#pragma unroll
  for (int tt = 0; tt < TPW; ++tt) {
    const int u = (w * TPW + tt) * 4 + g;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int b = 16 * c + pc;
      if (u < p.H && b < nvalid) {
        if constexpr (!POLICY::kAllSteps) p.h_out[(size_t)(b0 + b) * p.H + u] = fin[(size_t)(p.I + u) * LD + b];
        p.c_out[(size_t)(b0 + b) * p.H + u] = cst[tt][c];
      }
    }
  }
