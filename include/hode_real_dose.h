/* C ABI of libhode_real_dose.so: the discrete adjoint of the fixed-grid solve (euler / midpoint / 3/8-rule rk4) of the
 * real-data hybrid rhs HODE_RHS_ROCHE_REAL (reference model.py:570-657) that ALSO produces the gradient with respect to the
 * table of hourly doses act[Ta][B], gfx950.  Backward only: the forward is hode_rk_fwd of libhode.so / libhode_real_dims.so.
 *
 * The kernels evaluate Dose(t) = exp(kel (n - t)) S_n with n = min(Ta, floor(t)), S_n = act[n-1] + E S_{n-1}, E = exp(-kel),
 * S_0 = 0 (Dose = 0 for n < 1), and the dose enters the rhs in KX[3] = kel Dose(ts) - kel2 X[3] alone.  With gX the
 * cotangent handed to the VJP of a stage evaluated at time ts,
 *
 *     tap:      n = min(Ta, floor(ts)) >= 1:  S^_n += gX[3] kel exp(kel (n - ts))
 *     scan:     n = Ta .. 1:  grad_act[n-1] = S^_n,  S^_{n-1} += E S^_n.
 *
 * The reverse sweep meets the stage times in non-increasing order, so the n of successive taps never increases and the lane
 * that carries a patient's X fuses the scan into the sweep with two registers.  Every element of grad_act is written exactly
 * once, by its own patient's lane: no atomics, no memset, no workspace beyond hode_real_dims_rk_bwd's; repeats are
 * bit-identical.  Rows at or after the last stage time are exactly 0.
 *
 * Layout: 16 patients per wave on the matrix cores (the device code of csrc/hode_real_mf.hpp with the ragged tile,
 * M = latent_dim - 4 at run time), stages recomputed from h[n], weight gradients accumulated on chip and folded in a fixed
 * order.
 *
 * Conventions as in hode.h, whose constants are used: device pointers, fp32, h[T][B][D]; return 0 ok, <0 an argument error
 * (HODE_E_*), >0 a hipError_t from a launch, text in hode_real_dose_last_error_string(); an argument error launches nothing.
 * The library never allocates, never synchronises and never reads anything back.
 *
 * Domain: latent_dim 5 .. 20, hidden_dim 1 .. 64, method HODE_METHOD_EULER / _MIDPOINT / _RK4_38, batch >= 1, n_times >= 1,
 * n_action_times >= 1, any increasing grid, perturb 0 / 1, flags 0. */
#ifndef HODE_REAL_DOSE_H_
#define HODE_REAL_DOSE_H_

#include <stddef.h>
#include <stdint.h>

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_REAL_DOSE_ABI_VERSION 1

typedef struct hode_real_dose_desc {
  uint32_t struct_size;    /* = sizeof(hode_real_dose_desc) */
  int32_t method;          /* HODE_METHOD_EULER / _MIDPOINT / _RK4_38 */
  int32_t perturb;         /* the forward's: first / last stage time moved one ulp inside the step */
  int32_t batch;           /* B */
  int32_t latent_dim;      /* D = 5 .. 20 */
  int32_t hidden_dim;      /* H = 1 .. 64 */
  int32_t n_times;         /* T */
  int32_t n_action_times;  /* Ta >= 1 rows of the dose table */
  int32_t flags;           /* 0 */

  const float* t;          /* [T] increasing */
  const float* h;          /* the forward's output [T][B][D] (h[0] = y0) */
  const float* act;        /* [Ta][B] dose table */
  const float* theta;      /* [3]: k_immunity, kel, kel2 */
  const float* wflat;      /* [9 H + 2 + 3 (D-4)^2] all weights in creation order */
  const float* grad_h;     /* [T][B][D] */

  float* grad_y0;          /* out [B][D] */
  float* grad_act;         /* out [Ta][B], every element written */
  float* grad_wflat;       /* acc, shape of wflat */
  float* grad_theta;       /* acc [3] */

  void* workspace;         /* >= hode_real_dose_workspace_bytes(desc), 16-byte aligned */
  size_t workspace_bytes;
} hode_real_dose_desc;

int hode_real_dose_version(void);
const char* hode_real_dose_last_error_string(void);

/* bytes of workspace for this descriptor (0 for a descriptor outside the domain):
 * [ per-wave weight-gradient blocks | per-wave rows of the three scalars | dose table ] */
size_t hode_real_dose_workspace_bytes(const hode_real_dose_desc* d);

/* the sweep and the fixed-order folds of the weight-gradient blocks and the three scalars, on `stream` */
int hode_real_dose_bwd(const hode_real_dose_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif
