/* C ABI of libhode_dopri5_pp.so: the adaptive Dormand-Prince 5(4) solve of the hybrid Roche rhs with PER-PATIENT step
 * control, forward in one launch and the discrete adjoint in a second one, gfx950.
 *
 * hode_dopri5_fwd (hode.h) restates torchdiffeq's controller as it is: one RMS error norm over all B*D elements and one dt
 * for the whole batch, hence one launch per attempted step.  Here every patient carries a controller of its own -- Hairer's
 * initial step, the error ratio (RMS over the patient's D components against atol + rtol max(|y0|, |y1|)), accept / reject,
 * the step-size factor, the quartic dense output and the accepted-step tape -- which is torchdiffeq run on each patient as
 * a batch of one.  A patient's trajectory depends on nobody else's, so a lane runs its patient's whole solve in registers.
 *
 * The one place where this differs from "torchdiffeq on a batch of one": the backward treats EVERY step size as a constant,
 * dt_0 included (the semantics of HODE_FLAG_DETACH_FIRST_STEP of hode_dopri5_bwd); the derivative of Hairer's initial step
 * is not formed.
 *
 * Conventions as in hode.h, whose constants are used: device pointers, fp32, h[T][B][D]; return 0 ok, <0 an argument error
 * (HODE_E_*), >0 a hipError_t from a launch, text in hode_dopri5_pp_last_error_string(); an argument error launches
 * nothing.  The library never allocates, never synchronises and never reads anything back: numerical failure is reported
 * per patient in patient_status[B] (HODE_STATUS_* bits) and OR-ed into the one word *status, both zeroed by the caller.
 * A patient whose status is set stops; the others finish.  Every loop of the kernels has a bound that does not depend on
 * data: max_steps accepted steps and max_attempts attempts per patient (exceeding either sets HODE_STATUS_MAX_STEPS).
 *
 * Domain: rhs_kind HODE_RHS_ROCHE / HODE_RHS_ROCHE_ABLATE, latent_dim in {4, 6, 8, 12}, batch >= 1, n_times >= 1,
 * n_dose >= 1.  Parameter gradients are reduced per wave and folded in a fixed order: repeats are bit-identical. */
#ifndef HODE_DOPRI5_PP_H_
#define HODE_DOPRI5_PP_H_

#include <stddef.h>
#include <stdint.h>

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_DOPRI5_PP_ABI_VERSION 1

typedef struct hode_dopri5_pp_desc {
  uint32_t struct_size;    /* = sizeof(hode_dopri5_pp_desc) */
  int32_t rhs_kind;        /* HODE_RHS_ROCHE or HODE_RHS_ROCHE_ABLATE */
  int32_t batch;           /* B */
  int32_t latent_dim;      /* D in {4, 6, 8, 12} */
  int32_t n_times;         /* T */
  int32_t n_dose;          /* K >= 1 doses per patient */
  int32_t need_theta_grad; /* backward: also accumulate grad_theta */
  int32_t max_steps;       /* accepted steps per patient = rows of the tape */
  int32_t max_attempts;    /* attempts per patient; 0 = 8 * max_steps + 1024 */
  int32_t flags;           /* 0 or HODE_FLAG_NO_TAPE (forward only: no tape is written, the workspace holds no tape) */
  double rtol, atol;

  const float* t;          /* [T] strictly increasing */
  const float* y0;         /* [B][D] */
  const float* dosage;     /* [B] */
  const float* dose_times; /* [B][K] */
  const float* theta;      /* [HODE_N_THETA] */
  const float* w1;         /* [D-4][D] (NULL when D == 4) */
  const float* b1;         /* [D-4] */
  float* h;                /* forward out: [T][B][D], h[0] = y0 */
  int32_t* status;         /* [1], zeroed by the caller: OR of every patient's status */
  int32_t* n_accepted;     /* [B] forward out / backward in: accepted steps of each patient */
  int32_t* n_rejected;     /* [B] forward out */
  int32_t* patient_status; /* [B] forward out: HODE_STATUS_* bits of each patient */

  const float* grad_h;     /* backward in: [T][B][D] */
  float* grad_y0;          /* backward out: [B][D] */
  float* grad_w1;          /* acc, shape of w1 */
  float* grad_b1;          /* acc */
  float* grad_theta;       /* acc [HODE_N_THETA] (with need_theta_grad) */

  void* workspace;         /* >= hode_dopri5_pp_workspace_bytes(desc); the forward's tape, handed untouched to the backward */
  size_t workspace_bytes;
} hode_dopri5_pp_desc;

int hode_dopri5_pp_version(void);
const char* hode_dopri5_pp_last_error_string(void);

/* bytes of workspace for this descriptor (0 for a descriptor outside the domain).  With the tape:
 * [ per-wave gradient partials | tape_t [max_steps][B] double | tape_dt [max_steps][B] double |
 *   tape_j [max_steps][B] int32 pair | tape_y [max_steps][B][D] float ]; with HODE_FLAG_NO_TAPE the partials alone. */
size_t hode_dopri5_pp_workspace_bytes(const hode_dopri5_pp_desc* d);

/* one launch: every patient's whole adaptive solve */
int hode_dopri5_pp_fwd(const hode_dopri5_pp_desc* d, void* stream);

/* the sweep over the per-patient tapes and the fixed-order fold of the parameter-gradient partials */
int hode_dopri5_pp_bwd(const hode_dopri5_pp_desc* d, void* stream);

/* byte offsets inside the workspace: out5 = {partials, tape_t, tape_dt, tape_j, tape_y}; entry (n, p) of a tape array is
 * at index n * B + p.  Tests and diagnostics. */
int hode_dopri5_pp_tape_offsets(const hode_dopri5_pp_desc* d, size_t* out5);

#ifdef __cplusplus
}
#endif

#endif
