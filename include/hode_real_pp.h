/* C ABI of libhode_real_pp.so: Dormand-Prince 5(4) with PER-PATIENT step control for the real-data hybrid rhs
 * HODE_RHS_ROCHE_REAL (reference model.py:570-657), forward and discrete adjoint, gfx950.
 *
 * Every patient carries its own controller: Hairer's first step (order 4) from an RMS norm over its own D components, an
 * attempt, accept (ratio <= 1) or reject, the step factor of torchdiffeq's dopri5.  NO STEP CROSSES AN OUTPUT TIME: with j
 * the next output index, an attempt from t0 has the length dt_used = min(dt, t[j] - t0), a clipped attempt ends at t[j]
 * exactly, and h[j] is the endpoint of the accepted step that reaches t[j] -- there is no dense output.  After an attempt,
 * accepted or not, dt <- dt_used * factor(ratio).  The clock (t0, dt) is fp64, the stage times fp32; the two stages with
 * c = 1 are evaluated at the left limit nextafter_down(t1); FSAL.
 *
 * Layout: 16 patients per wave on the matrix cores (the device code of csrc/hode_real_mf.hpp with the ragged tile,
 * M = latent_dim - 4 at run time).  The 16 patients of a tile attempt together, each with its own t0, dt and accept flag;
 * the whole forward is ONE launch.  The backward is a second launch over the per-patient tapes: the discrete adjoint of
 * the accepted steps with every step size a constant (dt_0 included), stages recomputed from the taped state, weight
 * gradients accumulated on chip and folded in a fixed order (no atomics on gradients: repeats are bit-identical).
 *
 * Tape, per accepted step n of patient p (cell n * B + p): t0 and dt_used as doubles, the output index the step reached
 * or -1, and the D floats of the state at the step's start.
 *
 * Conventions as in hode.h, whose constants are used: device pointers, fp32, h[T][B][D]; return 0 ok, <0 an argument error
 * (HODE_E_*), >0 a hipError_t from a launch, text in hode_real_pp_last_error_string(); an argument error launches nothing.
 * The library never allocates, never synchronises and never reads anything back.
 *
 * Status: patient_status[p] is 0 or an OR of HODE_STATUS_NONFINITE / _DT_UNDERFLOW / _MAX_STEPS; status[0] is the OR over
 * the patients (the caller zeroes it).  A failing patient stops; the other patients of its tile finish.
 *
 * Domain: latent_dim 5 .. 20, hidden_dim 1 .. 64, batch >= 1, n_times >= 1, n_action_times >= 1, any increasing grid,
 * rtol > 0, atol >= 0, max_steps >= 1, flags 0 or HODE_FLAG_NO_TAPE (forward only). */
#ifndef HODE_REAL_PP_H_
#define HODE_REAL_PP_H_

#include <stddef.h>
#include <stdint.h>

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_REAL_PP_ABI_VERSION 1

typedef struct hode_real_pp_desc {
  uint32_t struct_size;    /* = sizeof(hode_real_pp_desc) */
  int32_t batch;           /* B */
  int32_t latent_dim;      /* D = 5 .. 20 */
  int32_t hidden_dim;      /* H = 1 .. 64 */
  int32_t n_times;         /* T */
  int32_t n_action_times;  /* Ta >= 1 rows of the dose table */
  int32_t max_steps;       /* accepted steps per patient = rows of the tape */
  int32_t max_attempts;    /* attempts per patient; 0 = 8 max_steps + 1024 */
  int32_t flags;           /* 0 or HODE_FLAG_NO_TAPE */
  double rtol, atol;

  const float* t;          /* [T] increasing */
  const float* y0;         /* [B][D] */
  const float* act;        /* [Ta][B] dose table */
  const float* theta;      /* [3]: k_immunity, kel, kel2 */
  const float* wflat;      /* [9 H + 2 + 3 (D-4)^2] all weights in creation order */
  float* h;                /* out (forward) / in (backward) [T][B][D] */

  int32_t* status;         /* [1] OR over the patients; zeroed by the caller */
  int32_t* n_accepted;     /* [B] out (forward) / in (backward) */
  int32_t* n_rejected;     /* [B] out (forward) */
  int32_t* patient_status; /* [B] out (forward) */

  const float* grad_h;     /* backward: [T][B][D] */
  float* grad_y0;          /* backward: out [B][D] */
  float* grad_wflat;       /* backward: acc, shape of wflat */
  float* grad_theta;       /* backward: acc [3] */

  void* workspace;         /* >= hode_real_pp_workspace_bytes(desc), 16-byte aligned; the forward's is the backward's */
  size_t workspace_bytes;
} hode_real_pp_desc;

int hode_real_pp_version(void);
const char* hode_real_pp_last_error_string(void);

/* bytes of workspace for this descriptor (0 for a descriptor outside the domain):
 * [ per-wave weight-gradient blocks | per-wave rows of the three scalars | tape_t | tape_dt | tape_j | tape_y | dose table ];
 * with HODE_FLAG_NO_TAPE the four tapes are empty */
size_t hode_real_pp_workspace_bytes(const hode_real_pp_desc* d);

/* the whole forward solve, one launch on `stream` */
int hode_real_pp_fwd(const hode_real_pp_desc* d, void* stream);

/* the sweep over the forward's tapes and the fixed-order folds of the weight-gradient blocks and the three scalars */
int hode_real_pp_bwd(const hode_real_pp_desc* d, void* stream);

/* byte offsets of tape_t, tape_dt, tape_j, tape_y inside the workspace (tests read the tapes back) */
int hode_real_pp_tape_offsets(const hode_real_pp_desc* d, size_t* out4);

#ifdef __cplusplus
}
#endif

#endif
