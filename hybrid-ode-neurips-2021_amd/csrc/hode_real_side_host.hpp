// Host code of the side libraries of the real-data hybrid rhs on the matrix cores -- libhode_real_dims.so (real_dims/),
// libhode_real_step.so (real_step/) and libhode_real_dose.so (real_dose/) -- kept once: the hidden-tile counts, the checks
// their entries share, the workspace layout, the fill of RealArgs and the dispatch on the hidden-tile count with the fold
// of the three scalars.  A library is described by data (RealSide); what only one of them checks or lays out stays in its
// own file.  Everything here is inline or a template: the per-hidden-tile units include it too (through their library's
// *.hpp) for HODE_REAL_SIDE_HTS and real_side_partial_floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "hode_host.hpp"
#include "hode_real_args.hpp"

// the hidden-tile counts HT a side library compiles a unit for (hidden_dim <= 16 HT)
#define HODE_REAL_SIDE_HTS(X) X(1) X(2) X(3) X(4)

namespace hode {

// floats of one wave's block of weight-gradient partials (RealGradAcc<HT>::NP; the units assert the equality)
constexpr size_t real_side_partial_floats(int ht) { return (size_t)(4 * ht + 3) * 256 + 16; }

// one side library: the prefix of its refusals, its sizes as they state them, the sizes themselves, and what its
// refusals add to the shared words
struct RealSide {
  const char* name;
  const char* have;
  int min_latent, max_latent, max_hidden;
  const char *latent_note = "", *hidden_note = "", *lanes_note = "", *method_note = "", *n_times_note = "", *sizes_note = "";
};

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }
inline int real_side_hidden_tiles(int hidden_dim) { return (hidden_dim + 15) / 16; }
inline size_t real_side_blocks(int batch) { return ((size_t)batch + 15) / 16; }  // of 16 patients: a wave's

// the descriptor itself, the rhs kind where the descriptor has one, and the two sizes
template <class Desc>
int real_side_check_domain(const RealSide& L, const Desc* d) {
  if (!d) return fail(HODE_E_NULL, "descriptor is NULL");
  if (d->struct_size != sizeof(Desc))
    return fail(HODE_E_SIZE, "struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(Desc));
  if constexpr (std::is_same<Desc, hode_solve_desc>::value) {
    if (d->rhs_kind != HODE_RHS_ROCHE_REAL)
      return fail(HODE_E_UNSUPPORTED, "%s: rhs_kind %d is not served here (have HODE_RHS_ROCHE_REAL = %d at %s)", L.name, d->rhs_kind,
                  HODE_RHS_ROCHE_REAL, L.have);
  }
  if (d->latent_dim < L.min_latent || d->latent_dim > L.max_latent)
    return fail(HODE_E_UNSUPPORTED, "%s: latent_dim %d has no compiled kernel (have %s%s)", L.name, d->latent_dim, L.have, L.latent_note);
  if (d->hidden_dim < 1 || d->hidden_dim > L.max_hidden)
    return fail(HODE_E_UNSUPPORTED, "%s: hidden_dim %d has no compiled kernel (have %s%s)", L.name, d->hidden_dim, L.have, L.hidden_note);
  return 0;
}

inline int real_side_check_lanes(const RealSide& L, const hode_solve_desc* d) {
  if (d->lanes_per_patient != 0 && d->lanes_per_patient != 16)
    return fail(HODE_E_UNSUPPORTED, "%s: lanes_per_patient %d (have 0 and 16 at %s: the matrix-core layout only%s)", L.name,
                d->lanes_per_patient, L.have, L.lanes_note);
  return 0;
}

template <class Desc>
int real_side_check_method(const RealSide& L, const Desc* d) {
  if (d->method < HODE_METHOD_EULER || d->method > HODE_METHOD_RK4_38)
    return fail(HODE_E_UNSUPPORTED, "%s: unknown fixed-grid method %d%s", L.name, d->method, L.method_note);
  if (d->flags) return fail(HODE_E_UNSUPPORTED, "%s: flags %d have no meaning for this solve", L.name, d->flags);
  return 0;
}

template <class Desc>
int real_side_check_sizes(const RealSide& L, const Desc* d) {
  if (d->batch <= 0 || d->n_times <= 0 || d->n_action_times <= 0)
    return fail(HODE_E_SIZE, "bad sizes: batch=%d n_times=%d%s n_action_times=%d%s", d->batch, d->n_times, L.n_times_note,
                d->n_action_times, L.sizes_note);
  return 0;
}

inline int real_side_check_pointers(const hode_solve_desc* d, bool bwd) {
  if (!d->t || !d->y0 || !d->dosage || !d->theta || !d->w1 || !d->h)
    return fail(HODE_E_NULL, "t / y0 / dosage (dose table) / theta / w1 (flat weights) / h must be non-NULL");
  if (bwd && (!d->grad_h || !d->grad_y0 || !d->grad_theta)) return fail(HODE_E_NULL, "grad_h / grad_y0 / grad_theta required");
  return 0;
}

template <class Desc>
int real_side_check_workspace(const Desc* d, size_t need) {
  if (!d->workspace || d->workspace_bytes < need)
    return fail(HODE_E_WORKSPACE, "workspace %zu B < required %zu B", d->workspace_bytes, need);
  if ((uintptr_t)d->workspace & 15) return fail(HODE_E_ALIGN, "workspace must be 16-byte aligned");
  return 0;
}

struct RealSideLayout {
  size_t grads, partials, extra, dose, total;
};
// [ per-wave weight-gradient blocks (bwd) | per-wave rows of the three scalars (bwd) | `extra` bytes (bwd) | dose table ]
template <class Desc>
RealSideLayout real_side_layout(const Desc* d, bool bwd, size_t n_waves, size_t extra = 0) {
  RealSideLayout L{0, 0, 0, 0, 0};
  size_t off = 0;
  if (bwd) {
    L.grads = off; off = al256(off + n_waves * real_side_partial_floats(real_side_hidden_tiles(d->hidden_dim)) * sizeof(float));
    L.partials = off; off = al256(off + n_waves * 3 * sizeof(float));
    L.extra = off; off = al256(off + extra);
  }
  L.dose = off; off = al256(off + (size_t)2 * ((size_t)d->n_action_times + 1) * (size_t)d->batch * sizeof(float));
  L.total = off;
  return L;
}

// the kernels' arguments; the four pointers are the ones the two descriptor types name differently
template <class Desc>
RealArgs real_side_args(const Desc* d, const float* y0, const float* act, const float* wflat, float* h, const RealSideLayout& L,
                        bool bwd) {
  char* ws = (char*)d->workspace;
  RealArgs a{};
  a.t = d->t; a.y0 = y0; a.act = act; a.theta = d->theta; a.wflat = wflat; a.h = h;
  a.grad_h = d->grad_h; a.grad_y0 = d->grad_y0;
  a.tape = bwd ? (float*)(ws + L.grads) : nullptr;
  a.partials = bwd ? (float*)(ws + L.partials) : nullptr;
  a.dose_tab = (float*)(ws + L.dose);
  a.B = d->batch; a.T = d->n_times; a.Ta = d->n_action_times; a.H = d->hidden_dim; a.perturb = d->perturb;
  return a;
}

// launch[hidden tiles - 1](args ...), one launcher per HODE_REAL_SIDE_HTS; then, for a backward (`grad_theta` given), the
// fixed-order fold of the three scalars' per-wave rows
template <class Launch, class... Args>
int real_side_launch(Launch* const (&launch)[4], const RealArgs& a, size_t n_waves, float* grad_theta, hipStream_t s,
                     const Args&... args) {
  const int e = launch[real_side_hidden_tiles(a.H) - 1](args...);
  if (e || !grad_theta) return e;
  return launch_fold_partials(a.partials, (int)n_waves, 3, 0, 0, nullptr, nullptr, grad_theta, 1, s);
}

}  // namespace hode
