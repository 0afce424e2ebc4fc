/* C ABI of libhode_real_step.so: the ONE-STEP-AHEAD ("step") solve of the real-data hybrid rhs HODE_RHS_ROCHE_REAL
 * (reference DecoderReal.forward with a 3-D init, model.py:838-856) on the matrix cores, gfx950.  N independent intervals
 * per patient, each integrated from a start state of its own over S solver steps; forward and discrete adjoint in one
 * launch per direction (plus the dose-table prelude and the folds).  The device code is csrc/hode_real_mf.hpp with the
 * ragged tile, the one libhode.so and libhode_real_dims.so instantiate for the chained solve.
 *
 * The entries take hode_solve_desc of hode.h.  Fields that keep their meaning: struct_size, rhs_kind, method, perturb,
 * batch (B), latent_dim (D), hidden_dim, n_action_times (Ta), lanes_per_patient, dosage [Ta][B], theta, w1, grad_w1,
 * grad_theta, flags, workspace, workspace_bytes.  Fields read differently HERE:
 *     n_times    N, the number of intervals (>= 1)
 *     n_dose     S, the solver steps per interval (1 .. 8), the same for every interval
 *     max_steps  C, the consecutive intervals one wave owns; 0 = the library chooses
 *                (hode_real_step_intervals_per_wave), values above N mean N
 *     t          [N][S + 1]  the solver grid of every interval, its end point included; row i strictly increasing
 *     y0         [N][B][D]   the start state of every interval
 *     h          [N + 1][B][D] out: h[0] = 0 (the reference's padding row), h[i + 1] = the end state of interval i
 *     grad_h     [N + 1][B][D] cotangent of h (row 0 is not read)
 *     grad_y0    out [N][B][D]: row i = the VJP of interval i on grad_h[i + 1]
 * Domain: rhs_kind HODE_RHS_ROCHE_REAL, latent_dim 5 .. 20, hidden_dim 1 .. 64, lanes_per_patient 0 or 16, method euler /
 * midpoint / rk4, perturb 0 / 1, flags 0; the backward requires grad_w1 (the flat weight gradient, accumulated into) --
 * there is no operand-tape mode.  The backward recomputes the sub-step states of an interval (S > 1) into its own
 * workspace; nothing of the forward's workspace is needed again.  Anything else returns HODE_E_* of hode.h with a message
 * in hode_real_step_last_error_string(); > 0 is a hipError_t from a launch. */
#ifndef HODE_REAL_STEP_H_
#define HODE_REAL_STEP_H_

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_REAL_STEP_ABI_VERSION 1

int hode_real_step_version(void);
const char* hode_real_step_last_error_string(void);
/* which: HODE_WS_RK_FWD / HODE_WS_RK_BWD; 0 outside the domain */
size_t hode_real_step_workspace_bytes(const hode_solve_desc* desc, int which);
/* C as the launches of `desc` would use it (max_steps honoured; otherwise the run length with the least work per SIMD: the
 * grid of ceil(B / 16) x ceil(N / C) waves runs one wave per SIMD in rounds of 1 024); 0 outside the domain */
int hode_real_step_intervals_per_wave(const hode_solve_desc* desc);
int hode_real_step_rk_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_real_step_rk_bwd(const hode_solve_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_REAL_STEP_H_ */
