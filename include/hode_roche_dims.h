/* C ABI of libhode_roche_dims.so: the hybrid "Roche" rhs (expert block + tanh(W y + b), reference model.py:446-555) at
 * the latent sizes 5, 7, 9, 10, 11, 13, 14, 15, 16 on the fixed-grid and dopri5 kernels, gfx950.  libhode.so serves 4, 6,
 * 8, 12, 20 (dopri5: 4, 6, 8, 12); both are instantiated from the same kernel templates (csrc/hode_rk_kernels.hpp,
 * csrc/hode_dopri5_kernels.hpp) and take the SAME descriptor, hode_solve_desc of hode.h, with the same meaning of every
 * field, the same workspace protocol and the same tape format.
 *
 * Every entry has the signature and the contract of its hode_* namesake in hode.h.  Domain:
 *     rhs_kind HODE_RHS_ROCHE or HODE_RHS_ROCHE_ABLATE, latent_dim one of the sizes above,
 *     lanes_per_patient 0 (the default of the size), 1 (one patient per lane) or 4 (a patient per quad: the ragged quad
 *         layout where (latent_dim - 4) % 4 != 0; dopri5 has the quad layout at 16 only and runs one patient per lane
 *         elsewhere); there is no MFMA (16) or split (48) layout here,
 *     hode_roche_dims_rk_*: method euler / midpoint / rk4, perturb 0 / 1; flags HODE_FLAG_OVERWRITE_GRADS and
 *         HODE_FLAG_SKIP_FOLD (backward) -- no layout here keeps a stage tape, so HODE_WS_RK_FWD is 0,
 *     hode_roche_dims_dopri5_*: as hode_dopri5_* for the Roche kinds.
 * Anything else returns HODE_E_UNSUPPORTED / HODE_E_NULL / HODE_E_SIZE / ... (codes of hode.h) with a message that names
 * the value and the sizes in hode_roche_dims_last_error_string(); > 0 is a hipError_t from a launch. */
#ifndef HODE_ROCHE_DIMS_H_
#define HODE_ROCHE_DIMS_H_

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_ROCHE_DIMS_ABI_VERSION 1

int hode_roche_dims_version(void);
const char* hode_roche_dims_last_error_string(void);
/* which: HODE_WS_RK_FWD / _RK_BWD / _DOPRI5_FWD / _DOPRI5_BWD; 0 outside the domain */
size_t hode_roche_dims_workspace_bytes(const hode_solve_desc* desc, int which);
int hode_roche_dims_rk_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_roche_dims_rk_bwd(const hode_solve_desc* desc, void* hip_stream);
int hode_roche_dims_dopri5_fwd(const hode_solve_desc* desc, void* hip_stream);
int hode_roche_dims_dopri5_bwd(const hode_solve_desc* desc, void* hip_stream);
/* out5: byte offsets of the initial-step record, tape_t, tape_dt, tape_j, tape_y inside the dopri5 workspace */
int hode_roche_dims_dopri5_tape_offsets(const hode_solve_desc* desc, size_t* out5);

#ifdef __cplusplus
}
#endif
#endif /* HODE_ROCHE_DIMS_H_ */
