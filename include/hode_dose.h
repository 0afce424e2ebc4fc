/* C ABI of libhode_dose.so: the discrete adjoint of the fixed-grid solve (euler / midpoint / 3/8-rule rk4) of the hybrid
 * Roche rhs that ALSO produces the gradient with respect to every patient's dosage, gfx950.
 *
 * hode_rk_bwd (hode.h) gives grad_y0, grad_w1, grad_b1 and grad_theta and nothing for the treatment.  The reference
 * differentiates through it: RocheODE.set_action takes dosage = max over time of the action, dose_at_time multiplies by it,
 * and torchdiffeq's plain odeint is ordinary autograd.  Here the same sweep carries one more per-lane accumulator.  With g
 * the cotangent handed to the rhs' VJP at a stage evaluated at time ts,
 *
 *     grad_dosage[p] += g[3] * kel * s_p(ts),     s_p(t) = sum_k 1[t >= tau_k] exp(kel (tau_k - t)),
 *
 * the dose schedule at unit dosage.  s_p does not depend on the dosage, so a patient whose dosage is 0 has a well-defined
 * gradient.  Under HODE_RHS_ROCHE_ABLATE the dose does not enter the rhs and grad_dosage is exactly 0.
 *
 * Layout: one lane per patient, 64-lane workgroups, the stages recomputed from h[n] (no tape).  grad_dosage[p] is written by
 * patient p's own lane; the parameter gradients are reduced per wave and folded in a fixed order.  No atomics: repeats are
 * bit-identical.
 *
 * Conventions as in hode.h, whose constants are used: device pointers, fp32, h[T][B][D]; return 0 ok, <0 an argument error
 * (HODE_E_*), >0 a hipError_t from a launch, text in hode_dose_last_error_string(); an argument error launches nothing.
 * The library never allocates, never synchronises and never reads anything back.
 *
 * Domain: rhs_kind HODE_RHS_ROCHE / HODE_RHS_ROCHE_ABLATE, latent_dim in {4, 6, 8, 12}, method HODE_METHOD_EULER /
 * HODE_METHOD_MIDPOINT / HODE_METHOD_RK4_38, batch >= 1, n_times >= 1, n_dose >= 1, any increasing grid, perturb 0 / 1. */
#ifndef HODE_DOSE_H_
#define HODE_DOSE_H_

#include <stddef.h>
#include <stdint.h>

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_DOSE_ABI_VERSION 1

typedef struct hode_dose_desc {
  uint32_t struct_size;    /* = sizeof(hode_dose_desc) */
  int32_t rhs_kind;        /* HODE_RHS_ROCHE or HODE_RHS_ROCHE_ABLATE */
  int32_t method;          /* HODE_METHOD_EULER / _MIDPOINT / _RK4_38 */
  int32_t perturb;         /* the forward's: first / last stage time moved one ulp inside the step */
  int32_t batch;           /* B */
  int32_t latent_dim;      /* D in {4, 6, 8, 12} */
  int32_t n_times;         /* T */
  int32_t n_dose;          /* K >= 1 doses per patient */
  int32_t need_theta_grad; /* also accumulate grad_theta */
  int32_t flags;           /* 0 */

  const float* t;          /* [T] increasing */
  const float* h;          /* the forward's output [T][B][D] (h[0] = y0) */
  const float* dosage;     /* [B] */
  const float* dose_times; /* [B][K] */
  const float* theta;      /* [HODE_N_THETA] */
  const float* w1;         /* [D-4][D] (NULL when D == 4) */
  const float* b1;         /* [D-4] */
  const float* grad_h;     /* [T][B][D] */

  float* grad_y0;          /* out [B][D] */
  float* grad_dosage;      /* out [B] */
  float* grad_w1;          /* acc, shape of w1 */
  float* grad_b1;          /* acc */
  float* grad_theta;       /* acc [HODE_N_THETA] (with need_theta_grad) */
  int32_t* status;         /* [1] or NULL, zeroed by the caller: HODE_STATUS_NONFINITE when a gradient of a patient is not finite */

  void* workspace;         /* >= hode_dose_workspace_bytes(desc): the per-wave gradient partials */
  size_t workspace_bytes;
} hode_dose_desc;

int hode_dose_version(void);
const char* hode_dose_last_error_string(void);

/* bytes of workspace for this descriptor (0 for a descriptor outside the domain): [waves][partials] floats */
size_t hode_dose_workspace_bytes(const hode_dose_desc* d);

/* the sweep and the fixed-order fold of the parameter-gradient partials, on `stream` */
int hode_dose_bwd(const hode_dose_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif
