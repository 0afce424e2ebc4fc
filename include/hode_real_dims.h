/* C ABI of libhode_real_dims.so: the real-data hybrid rhs HODE_RHS_ROCHE_REAL (two small MLPs + GRU-ODE block, reference
 * model.py:570-657) on the matrix-core fixed-grid kernels at the latent sizes 5 .. 20, gfx950.  libhode.so serves 4 and 20;
 * both are built from the same device code (csrc/hode_real_mf.hpp) and take the SAME descriptor, hode_solve_desc of
 * hode.h, with the same meaning of every field and the same workspace protocol.  Size 20 is accepted here only so that
 * this library's ragged-tile kernels can be held against libhode.so's.
 *
 * Every entry has the signature and the contract of its hode_* namesake in hode.h.  Domain:
 *     rhs_kind HODE_RHS_ROCHE_REAL, latent_dim 5 .. 20, hidden_dim 1 .. 64,
 *     lanes_per_patient 0 or 16 (the matrix-core layout; there is no one-patient-per-lane kernel here),
 *     method euler / midpoint / rk4, perturb 0 / 1, flags 0,
 *     backward: grad_w1 (the flat weight gradient, accumulated into) is required -- there is no operand-tape mode.
 * Anything else returns HODE_E_UNSUPPORTED / HODE_E_NULL / HODE_E_SIZE / ... (codes of hode.h) with a message that names
 * the value and the sizes in hode_real_dims_last_error_string(); > 0 is a hipError_t from a launch. */
#ifndef HODE_REAL_DIMS_H_
#define HODE_REAL_DIMS_H_

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_REAL_DIMS_ABI_VERSION 1

int hode_real_dims_version(void);
const char* hode_real_dims_last_error_string(void);
/* which: HODE_WS_RK_FWD / HODE_WS_RK_BWD; 0 outside the domain */
size_t hode_real_dims_workspace_bytes(const hode_solve_desc* desc, int which);
int hode_real_dims_rk_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_real_dims_rk_bwd(const hode_solve_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_REAL_DIMS_H_ */
