// Host side of the adaptive (dopri5) forward that the Roche solver (hode_dopri5.hip) and the NeuralODE solver
// (hode_neural_dopri5_kernels.hpp) share: how the workspace is carved, how many attempts go out between two reads of the
// controller record, and the attempt loop with what follows it.  Host code only; nothing here knows which solver calls it.
// The functions have internal linkage: they are helpers of the unit that includes them, not names of its library.
// The kernels take different argument structs (DpArgs / NdpArgs), so filling those stays with each solver.
#pragma once
#include <hip/hip_runtime.h>

#include "hode_dopri5_kernels.hpp"

namespace hode {

constexpr size_t kInitOffset = 128;  // DpInit sits behind the two DpCtrl records
static_assert(2 * sizeof(DpCtrl) <= kInitOffset, "controller records overlap the init record");
static_assert(sizeof(DpInit) == sizeof(hode_dopri5_init_record), "DpInit is the ABI's hode_dopri5_init_record");

// ---------------------------------------------------------------------------------------------------- workspace
struct AdaptiveLayout {
  size_t ctrl, partials, slots, kbuf, tape_t, tape_dt, tape_j, tape_y, grad_partials, total;
};

// Byte offsets of the fields, each on a 256-byte boundary.  `BD` = batch * latent_dim; `slot_bytes` is the persistent
// attempt loop's exchange array (Roche only; 0 adds no offset, every step being aligned already); `grad_floats_per_wave`
// is the length of one wave's block of gradient partials.
static inline AdaptiveLayout adaptive_layout(int n_waves, size_t BD, int max_steps, bool no_tape, size_t slot_bytes,
                                             size_t grad_floats_per_wave) {
  const auto align = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t S = (size_t)(max_steps > 0 ? max_steps : 1);
  AdaptiveLayout L;
  size_t off = 0;
  L.ctrl = off; off = align(off + kInitOffset + sizeof(DpInit));  // two controller records + the DpInit record
  L.partials = off; off = align(off + (size_t)4 * n_waves * sizeof(float));
  L.slots = off; off = align(off + slot_bytes);
  L.kbuf = off; off = align(off + 7 * BD * sizeof(float));
  L.tape_t = off; off = align(off + S * sizeof(double));
  L.tape_dt = off; off = align(off + S * sizeof(double));
  L.tape_j = off; off = align(off + 2 * S * sizeof(int));
  L.tape_y = off; off = align(off + (no_tape ? 2 : S + 1) * BD * sizeof(float));
  L.grad_partials = off; off = align(off + (size_t)n_waves * grad_floats_per_wave * sizeof(float));
  L.total = off;
  return L;
}

// what hode_dopri5_tape_offsets reports: the init record and the four tape arrays
static inline void adaptive_tape_offsets(const AdaptiveLayout& L, size_t* out5) {
  out5[0] = L.ctrl + kInitOffset;
  out5[1] = L.tape_t;
  out5[2] = L.tape_dt;
  out5[3] = L.tape_j;
  out5[4] = L.tape_y;
}

// ------------------------------------------------------------------------------------------------- chunk policy
// Attempts enqueued between two reads of the controller record.  Every read is a host round trip during which the GPU
// idles (~70 us measured: 29-30 ms per solve with a fixed chunk of 32, 26.7 ms with 128 at 4 200 attempts), every attempt
// enqueued past the end costs an early-exit launch (~1.3 us).  The chunk therefore starts small (`first`), doubles while
// nothing is known, and then follows an estimate of what is left: attempts so far scaled by the output-grid progress
// j_next / T, kept within [min, max].
struct ChunkPolicy {
  int first, min, max;
};

static inline int next_chunk(const ChunkPolicy& p, int chunk, long long attempts, int j_next, int n_times) {
  const double done = n_times > 1 ? (double)(j_next - 1) / (double)(n_times - 1) : 1.0;
  if (done <= 0.0) return chunk * 2 > p.max ? p.max : chunk * 2;
  const double left = (double)attempts * (1.0 - done) / done;
  long long c = (long long)(0.75 * left);
  if (c < p.min) c = p.min;
  if (c > p.max) c = p.max;
  return (int)c;
}

// ------------------------------------------------------------------------------------------------- attempt loop
// every attempt either accepts (<= max_steps of those) or shrinks dt by >= 5x towards underflow: a generous bound
static inline long long adaptive_max_attempts(const hode_solve_desc* d) { return 64LL * ((long long)d->max_steps + 64); }

// Runs attempts until the controller reports `done`: enqueue(i) launches attempt number i on `s` and returns 0 or an error
// code (its own per-launch check, if it has one); hipGetLastError is looked at once per chunk, under the name `launch_what`.
// `ctrl` is the device's pair of controller records, double-buffered by attempt parity; *host receives the last one read.
template <class Enqueue>
static int adaptive_attempts(const hode_solve_desc* d, const DpCtrl* ctrl, const ChunkPolicy& policy, const char* launch_what,
                             hipStream_t s, Enqueue&& enqueue, DpCtrl* host) {
  int attempt = 0, chunk = policy.first;
  const long long max_attempts = adaptive_max_attempts(d);
  for (;;) {
    for (int i = 0; i < chunk; ++i)
      if (int e = enqueue(attempt++)) return e;
    if (int e = hip_fail(hipGetLastError(), launch_what)) return e;
    // the ONE host synchronisation of the path: the number of adaptive steps is data dependent
    if (int e = hip_fail(hipMemcpyAsync(host, ctrl + (attempt & 1), sizeof(DpCtrl), hipMemcpyDeviceToHost, s), "controller read-back"))
      return e;
    if (int e = hip_fail(hipStreamSynchronize(s), "controller read-back sync")) return e;
    if (host->done) return 0;
    if (attempt > max_attempts) {
      host->status |= HODE_STATUS_MAX_STEPS;
      return 0;
    }
    chunk = next_chunk(policy, chunk, attempt, host->j_next, d->n_times);
  }
}

// what follows the loop: the step counts to the caller's host memory, a non-zero status to its device word
static inline int adaptive_report(const hode_solve_desc* d, const DpCtrl& host, hipStream_t s) {
  *d->host_n_accepted = host.n_acc;
  if (d->host_n_rejected) *d->host_n_rejected = host.n_rej;
  if (d->status && host.status) {
    if (int e = hip_fail(hipMemcpyAsync(d->status, &host.status, sizeof(int), hipMemcpyHostToDevice, s), "status write")) return e;
    if (int e = hip_fail(hipStreamSynchronize(s), "status write sync")) return e;
  }
  return 0;
}

}  // namespace hode
