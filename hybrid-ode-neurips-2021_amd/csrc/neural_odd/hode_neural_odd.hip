// C-ABI entry points of libhode_neural_odd.so (include/hode_neural_odd.h): the NeuralODE rhs at the odd latent dimensions
// 5 .. 15 -- argument checks, the per-dimension table, the library's own error text.  The kernels are the templates
// libhode.so instantiates at the even dimensions (hode_neural_odd_dim.hip); this library exists because libhode.so's set of
// kernel symbols is pinned, not because the code differs.  At D = 15 [y, Dose] fills the 16-row input tile exactly and the
// layer-1 bias gradient takes NeuralGradAcc's path without the ones row (../hode_neural_mf.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once
#include "../hode_host.hpp"
#include "../hode_neural_args.hpp"
#include "hode_neural_odd.hpp"

namespace {

using hode::fail;
using hode::NeuralOddDim;

const NeuralOddDim* dim_entry(int latent_dim) {
  switch (latent_dim) {
#define HODE_NEURAL_ODD_CASE(n) case n: return hode::neural_odd_d##n();
    HODE_NEURAL_ODD_DIMS(HODE_NEURAL_ODD_CASE)
#undef HODE_NEURAL_ODD_CASE
  }
  return nullptr;
}

// what every entry checks first; *out is the table row of the latent dimension
int check_domain(const hode_solve_desc* d, const NeuralOddDim** out) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(hode_solve_desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(hode_solve_desc));
  if (d->rhs_kind != HODE_RHS_NEURAL)
    return fail(HODE_E_UNSUPPORTED, "neural odd: rhs_kind %d is not served here (have HODE_RHS_NEURAL = %d)", d->rhs_kind, HODE_RHS_NEURAL);
  *out = dim_entry(d->latent_dim);
  if (!*out)
    return fail(HODE_E_UNSUPPORTED, "neural odd: latent_dim %d has no compiled kernel (have 5, 7, 9, 11, 13, 15; libhode.so has 4, 6, 8, 10, 12, 14)",
                d->latent_dim);
  if (d->hidden_dim != 10 * d->latent_dim)
    return fail(HODE_E_UNSUPPORTED, "neural odd: hidden_dim %d != 10 * latent_dim (reference model.py:991-996)", d->hidden_dim);
  if (d->lanes_per_patient != 0 && d->lanes_per_patient != 16)
    return fail(HODE_E_UNSUPPORTED, "neural odd: lanes_per_patient %d (have 0 and 16: the matrix-core layout only)", d->lanes_per_patient);
  return 0;
}

int check_pointers(const hode_solve_desc* d, bool bwd) {
  if (d->batch <= 0 || d->n_times <= 0 || d->n_dose < 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d n_dose=%d", d->batch, d->n_times, d->n_dose);
  if (!d->t || !d->y0 || !d->dosage || !d->h || !d->w1 || !d->b1 || !d->w2 || !d->b2 || (d->n_dose > 0 && !d->dose_times))
    return fail(HODE_E_NULL, "t / y0 / dosage / dose_times / h / w1 / b1 / w2 / b2 must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0)) return fail(HODE_E_NULL, "grad_h / grad_y0 required by the backward");
  if (bwd && !d->grad_w1)
    return fail(HODE_E_UNSUPPORTED, "neural odd: grad_w1 is NULL -- the operand-tape mode is not built here, the backward accumulates the weight gradients on chip");
  if (bwd && (!d->grad_b1 || !d->grad_w2 || !d->grad_b2)) return fail(HODE_E_NULL, "grad_b1 / grad_w2 / grad_b2 are required next to grad_w1");
  if ((uintptr_t)d->workspace & 15) return fail(HODE_E_ALIGN, "workspace must be 16-byte aligned");
  return 0;
}

int check_rk(const hode_solve_desc* d, bool bwd, const NeuralOddDim** e) {
  if (int err = check_domain(d, e)) return err;
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "neural odd: unknown fixed-grid method %d", d->method);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "neural odd: flags %d have no meaning for the fixed-grid solve", d->flags);
  if (int err = check_pointers(d, bwd)) return err;
  const size_t need = bwd ? (*e)->rk_partial_bytes(d) : 0;
  if (need && (!d->workspace || d->workspace_bytes < need))
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  return 0;
}

int check_dopri5(const hode_solve_desc* d, bool bwd, const NeuralOddDim** e) {
  if (int err = check_domain(d, e)) return err;
  const int known = bwd ? HODE_FLAG_DETACH_FIRST_STEP : HODE_FLAG_NO_TAPE;
  if (bwd && (d->flags & HODE_FLAG_NO_TAPE))
    return fail(HODE_E_UNSUPPORTED, "the forward ran with HODE_FLAG_NO_TAPE (flags %d): there is no tape to sweep", d->flags);
  if (d->flags & ~known) return fail(HODE_E_UNSUPPORTED, "neural odd: flags %d (dopri5 %s honours %d only)", d->flags, bwd ? "backward" : "forward", known);
  if (d->max_steps <= 0) return fail(HODE_E_SIZE, "bad sizes: max_steps=%d", d->max_steps);
  if (!(d->rtol > 0) || !(d->atol >= 0)) return fail(HODE_E_SIZE, "rtol must be > 0 and atol >= 0");
  if (int err = check_pointers(d, bwd)) return err;
  if (!d->host_n_accepted) return fail(HODE_E_NULL, "host_n_accepted is required (fwd: out, bwd: in)");
  return 0;  // the workspace size is checked by the launcher, which lays it out
}

hode::NeuralArgs rk_args(const hode_solve_desc* d) {
  hode::NeuralArgs a{};
  a.t = d->t; a.y0 = d->y0; a.dosage = d->dosage; a.dose_times = d->dose_times; a.w1 = d->w1; a.b1 = d->b1; a.b2 = d->b2;
  a.w2 = d->w2; a.w2t = nullptr;
  a.h = d->h; a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.a1t = (float*)d->workspace;  // the on-chip backward's per-wave partials
  a.B = d->batch; a.T = d->n_times; a.K = d->n_dose; a.perturb = d->perturb;
  return a;
}

}  // namespace

extern "C" int hode_neural_odd_version(void) { return HODE_NEURAL_ODD_ABI_VERSION; }

extern "C" const char* hode_neural_odd_last_error_string(void) { return hode::g_err; }

extern "C" size_t hode_neural_odd_workspace_bytes(const hode_solve_desc* d, int which) {
  const NeuralOddDim* e = nullptr;
  if (check_domain(d, &e)) return 0;
  switch (which) {
    case HODE_WS_RK_BWD: return d->grad_w1 ? e->rk_partial_bytes(d) : 0;
    case HODE_WS_DOPRI5_FWD:
    case HODE_WS_DOPRI5_BWD: return e->dopri5_workspace_bytes(d);
    default: return 0;  // HODE_WS_RK_FWD: the forward needs none
  }
}

extern "C" int hode_neural_odd_rk_fwd(const hode_solve_desc* d, void* stream) {
  const NeuralOddDim* e = nullptr;
  if (int err = check_rk(d, false, &e)) return err;
  return e->rk(d, rk_args(d), false, (hipStream_t)stream);
}

extern "C" int hode_neural_odd_rk_bwd(const hode_solve_desc* d, void* stream) {
  const NeuralOddDim* e = nullptr;
  if (int err = check_rk(d, true, &e)) return err;
  return e->rk(d, rk_args(d), true, (hipStream_t)stream);
}

extern "C" int hode_neural_odd_dopri5_fwd(const hode_solve_desc* d, void* stream) {
  const NeuralOddDim* e = nullptr;
  if (int err = check_dopri5(d, false, &e)) return err;
  return e->dopri5(d, false, (hipStream_t)stream);
}

extern "C" int hode_neural_odd_dopri5_bwd(const hode_solve_desc* d, void* stream) {
  const NeuralOddDim* e = nullptr;
  if (int err = check_dopri5(d, true, &e)) return err;
  return e->dopri5(d, true, (hipStream_t)stream);
}

extern "C" int hode_neural_odd_dopri5_tape_offsets(const hode_solve_desc* d, size_t* out5) {
  const NeuralOddDim* e = nullptr;
  if (!out5) return fail(HODE_E_NULL, "out5 is NULL");
  if (int err = check_domain(d, &e)) return err;
  e->dopri5_tape_offsets(d, out5);
  return 0;
}
