/* C ABI of libhode_neural_odd.so: the NeuralODE rhs dy/dt = tanh(W2 tanh(W1 [y, Dose(t)] + b1) + b2) (reference
 * model.py:969-1026) at the ODD latent dimensions 5, 7, ..., 15 on the matrix-core kernels, gfx950.  libhode.so serves
 * the even ones (4 .. 14); both are instantiated from the same kernel templates (csrc/hode_neural_mf_kernels.hpp,
 * csrc/hode_neural_dopri5_kernels.hpp) and take the SAME descriptor, hode_solve_desc of hode.h, with the same meaning
 * of every field, the same workspace protocol and the same tape format.
 *
 * Every entry has the signature and the contract of its hode_* namesake in hode.h.  Domain:
 *     rhs_kind == HODE_RHS_NEURAL, latent_dim in {5, 7, 9, 11, 13, 15}, hidden_dim == 10 * latent_dim,
 *     lanes_per_patient 0 or 16 (there is no lane-per-patient layout here),
 *     hode_neural_odd_rk_*: method euler / midpoint / rk4, perturb 0 / 1; the backward needs grad_w1 .. grad_b2 (the
 *         weight gradients are accumulated on chip; there is no operand-tape mode),
 *     hode_neural_odd_dopri5_*: flags HODE_FLAG_NO_TAPE (forward) and HODE_FLAG_DETACH_FIRST_STEP (backward).
 * Anything else returns HODE_E_UNSUPPORTED / HODE_E_NULL / HODE_E_SIZE (codes of hode.h) with a message that names the
 * value in hode_neural_odd_last_error_string(); > 0 is a hipError_t from a launch. */
#ifndef HODE_NEURAL_ODD_H_
#define HODE_NEURAL_ODD_H_

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_NEURAL_ODD_ABI_VERSION 1

int hode_neural_odd_version(void);
const char* hode_neural_odd_last_error_string(void);
/* which: HODE_WS_RK_FWD / _RK_BWD / _DOPRI5_FWD / _DOPRI5_BWD; 0 outside the domain */
size_t hode_neural_odd_workspace_bytes(const hode_solve_desc* desc, int which);
int hode_neural_odd_rk_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_neural_odd_rk_bwd(const hode_solve_desc* desc, void* hip_stream);
int hode_neural_odd_dopri5_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_neural_odd_dopri5_bwd(const hode_solve_desc* desc, void* hip_stream);
/* out5: byte offsets of the initial-step record, tape_t, tape_dt, tape_j, tape_y inside the dopri5 workspace */
int hode_neural_odd_dopri5_tape_offsets(const hode_solve_desc* desc, size_t* out5);

#ifdef __cplusplus
}
#endif
#endif /* HODE_NEURAL_ODD_H_ */
