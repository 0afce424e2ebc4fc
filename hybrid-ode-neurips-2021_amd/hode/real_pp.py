"""dopri5 with PER-PATIENT step control for the real-data hybrid rhs (``hode_real_pp_fwd`` / ``hode_real_pp_bwd``,
libhode_real_pp.so): every patient carries its own controller -- Hairer's first step, an RMS error norm over its own D
components, accept / reject, an accepted-step tape of its own -- and NO STEP CROSSES AN OUTPUT TIME: an attempt is clipped
to the next output time, so every ``h[j]`` is the endpoint of an accepted step and there is no dense output.  This is what
``DecoderReal``'s own default (``method="dopri5"`` with ``options["step_t"] = t``) means for a batch of one.  The whole forward
is ONE launch (16 patients per wave on the matrix cores, attempting together, each with its own step length), the backward
a second one over the per-patient tapes: the discrete adjoint of the accepted steps with every step size a constant,
``dt_0`` included.  At B > 1 the trajectories differ from a batch-global controller's, by design.

Out of its domain, each refused with a message: latent size 4 (the expert-only model) and sizes above 20, hidden sizes
above 64, CPU tensors, the one-step-ahead solve, gradients for ``t`` and for the dose table.

Two plain launch functions; the ``torch.autograd.Function`` that joins them lives next to the module it serves, in the
package-root ``model.py`` (``RocheODEReal.step_control = "patient"``)."""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _real_pp_lib as PL
from .patient_dopri5 import _status_error
from .solver import _f32c, _i32c, _require_gpu, _stream

#: the last forward: per-patient device tensors "n_accepted", "n_rejected", "status" (B,) int32, and the host values
#: "no_tape", "max_steps", "workspace_bytes"
last_stats = {}


def check_domain(latent_dim, hidden_dim):
    """Raise HodeConfigError outside the kernels' domain, before a library is loaded or anything is launched."""
    if not PL.MIN_LATENT <= int(latent_dim) <= PL.MAX_LATENT:
        raise L.HodeConfigError("hode.real_pp: per-patient step control is compiled for %s (got latent dimension %d); "
                                "there is no torch-eager path in the product" % (PL.sizes_text(), latent_dim))
    if not 1 <= int(hidden_dim) <= PL.MAX_HIDDEN:
        raise L.HodeConfigError("hode.real_pp: per-patient step control is compiled for %s (got hidden dimension %d); "
                                "there is no torch-eager path in the product" % (PL.sizes_text(), hidden_dim))


def _check_shapes(y0, theta, wflat, t, act, hidden):
    B, D = y0.shape
    M = D - 4
    if t.dim() != 1 or act.dim() != 2 or act.shape[1] != B or theta.numel() != 3 or wflat.numel() != 9 * hidden + 2 + 3 * M * M:
        raise L.HodeConfigError("hode.real_pp: y0 (B, D), t (T,), act (Ta, B), theta (3,) and wflat (%d,) expected (got %s, %s, "
                                "%s, %s, %s)" % (9 * hidden + 2 + 3 * M * M, tuple(y0.shape), tuple(t.shape), tuple(act.shape),
                                                 tuple(theta.shape), tuple(wflat.shape)))


def real_patient_dopri5_forward(y0, theta, wflat, t, act, hidden, rtol=1e-7, atol=1e-8, max_steps=0, max_attempts=0,
                                no_tape=False):
    """The forward launch.  y0 (B, D); theta (3,) = (k_immunity, kel, kel2); wflat all weights in creation order; t (T,);
    act (Ta, B) the table of hourly doses.  Returns ``(h (T, B, D), tape_ws, stats)``: ``tape_ws`` is the int32 workspace
    tensor that holds the per-patient tapes for ``real_patient_dopri5_backward`` (without a tape when ``no_tape``: pass that
    when nothing needs a gradient -- the caller samples grad mode), ``stats`` is ``last_stats``.

    ``max_steps`` (accepted steps per patient = rows of the tape, default ``16 T + 64``) is multiplied by 4 and the solve
    repeated while only MAX_STEPS is set, and refused once the tape no longer fits the device; ``max_attempts`` bounds the
    attempts of a patient (default ``8 max_steps + 1024``).  A failing status raises HodeError (a RuntimeError) with the texts
    of ``hode.patient_dopri5`` plus the index of the first failing patient; the other patients have finished."""
    _require_gpu(y0, theta, wflat, t, act)
    B, D = y0.shape
    hidden = int(hidden)
    check_domain(D, hidden)
    _check_shapes(y0, theta, wflat, t, act, hidden)
    lib = PL.lib()
    y0c, thc, wc, tc, ac = _f32c(y0), _f32c(theta), _f32c(wflat), _f32c(t), _f32c(act)
    T = tc.numel()
    h = torch.empty((T, B, D), device=y0c.device, dtype=torch.float32)
    steps = int(max_steps) if max_steps else 16 * T + 64
    while True:
        status = torch.zeros(1, device=y0c.device, dtype=torch.int32)
        nacc = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        nrej = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        pst = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        d = PL.new_desc()
        d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times = B, D, hidden, tc.numel(), ac.shape[0]
        d.t, d.y0, d.act, d.theta, d.wflat = tc.data_ptr(), y0c.data_ptr(), ac.data_ptr(), thc.data_ptr(), wc.data_ptr()
        d.rtol, d.atol = float(rtol), float(atol)
        d.h, d.status = h.data_ptr(), status.data_ptr()
        d.n_accepted, d.n_rejected, d.patient_status = nacc.data_ptr(), nrej.data_ptr(), pst.data_ptr()
        d.max_steps, d.max_attempts = steps, int(max_attempts)
        d.flags = L.FLAG_NO_TAPE if no_tape else 0
        nbytes = lib.hode_real_pp_workspace_bytes(d)
        free, _ = torch.cuda.mem_get_info(y0c.device)
        if nbytes > free + torch.cuda.memory_reserved(y0c.device) - torch.cuda.memory_allocated(y0c.device):
            raise L.HodeError("hode dopri5 (per-patient step control, real-data rhs): tapes of %d accepted steps need %.1f GB, "
                              "the device has %.1f GB free (max_num_steps exceeded)" % (steps, nbytes / 1e9, free / 1e9))
        ws = torch.empty(max(nbytes, 4) // 4, device=y0c.device, dtype=torch.int32)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        with torch.cuda.device(y0c.device):
            PL.check(lib.hode_real_pp_fwd(d, _stream()), "hode_real_pp_fwd")
        st = int(status.item())
        if st == L.STATUS_MAX_STEPS and not no_tape and steps < (1 << 20) \
                and (not max_attempts or int(nacc.max().item()) >= steps):
            del ws
            steps *= 4  # a tape too small: retry with a larger one (refused above once it no longer fits the device)
            continue
        break
    last_stats.clear()
    last_stats.update(n_accepted=nacc, n_rejected=nrej, status=pst, no_tape=bool(no_tape), max_steps=steps,
                      workspace_bytes=int(nbytes))
    if st:
        first = int(torch.nonzero(pst)[0, 0].item())
        raise L.HodeError("hode dopri5 (per-patient step control, real-data rhs): %s (first failing patient: %d)"
                          % (_status_error(st) or "max_num_steps exceeded", first))
    return h, ws, last_stats


def real_patient_dopri5_backward(y0, theta, wflat, t, act, hidden, h, tape_ws, n_accepted, max_steps, grad_h, rtol=1e-7,
                                 atol=1e-8):
    """The backward launch for the inputs of a ``real_patient_dopri5_forward`` call, the ``h`` and ``tape_ws`` it returned
    and its ``stats["n_accepted"]`` / ``stats["max_steps"]``.  Returns ``(grad_y0, grad_theta[3], grad_wflat)``; the
    parameter gradients are reduced per wave and folded in a fixed order (bit-identical repeats)."""
    _require_gpu(y0, theta, wflat, t, act, h, tape_ws, n_accepted, grad_h)
    B, D = y0.shape
    hidden = int(hidden)
    check_domain(D, hidden)
    _check_shapes(y0, theta, wflat, t, act, hidden)
    lib = PL.lib()
    y0c, thc, wc, tc, ac = _f32c(y0), _f32c(theta), _f32c(wflat), _f32c(t), _f32c(act)
    hc, gh = _f32c(h), _f32c(grad_h)
    ws, nacc = _i32c(tape_ws, "tape_ws"), _i32c(n_accepted, "n_accepted")
    T = tc.numel()
    if gh.shape != (T, B, D) or hc.shape != (T, B, D) or nacc.shape != (B,):
        raise L.HodeConfigError("hode.real_pp: h and grad_h (T, B, D) and n_accepted (B,) expected")
    gy0 = torch.empty((B, D), device=y0c.device, dtype=torch.float32)
    gth = torch.zeros(3, device=y0c.device, dtype=torch.float32)
    gw = torch.zeros_like(wc)
    scratch = torch.zeros(B, device=y0c.device, dtype=torch.int32)  # status word, rejected counts, patient status: unused here
    d = PL.new_desc()
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times = B, D, hidden, tc.numel(), ac.shape[0]
    d.t, d.y0, d.act, d.theta, d.wflat = tc.data_ptr(), y0c.data_ptr(), ac.data_ptr(), thc.data_ptr(), wc.data_ptr()
    d.rtol, d.atol = float(rtol), float(atol)
    d.h, d.status = hc.data_ptr(), scratch.data_ptr()
    d.n_accepted = nacc.data_ptr()
    d.n_rejected = d.patient_status = scratch.data_ptr()
    d.max_steps = int(max_steps)
    d.grad_h, d.grad_y0, d.grad_wflat, d.grad_theta = gh.data_ptr(), gy0.data_ptr(), gw.data_ptr(), gth.data_ptr()
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    with torch.cuda.device(y0c.device):
        PL.check(lib.hode_real_pp_bwd(d, _stream()), "hode_real_pp_bwd")
    return gy0, gth, gw


def read_tape(tape_ws, batch, latent_dim, hidden, n_action_times, max_steps, n_accepted):
    """Tests only: the per-patient accepted-step tapes out of a forward's workspace, at the offsets
    ``hode_real_pp_tape_offsets`` reports -- a list over patients of ``{"t", "dt"}`` (float64 lists), ``"j"`` (the output
    index each step reached, or -1) and ``"y"`` (the state at each step's start, float32 rows)."""
    import numpy as np
    d = PL.new_desc()
    d.batch, d.latent_dim, d.hidden_dim, d.n_times = int(batch), int(latent_dim), int(hidden), 1
    d.n_action_times, d.max_steps = int(n_action_times), int(max_steps)
    off = (C.c_size_t * 4)()
    PL.check(PL.lib().hode_real_pp_tape_offsets(d, off), "hode_real_pp_tape_offsets")
    raw = tape_ws.cpu().numpy().view(np.uint8)
    cells = int(max_steps) * int(batch)
    t = raw[off[0]:off[0] + 8 * cells].view(np.float64).reshape(max_steps, batch)
    dt = raw[off[1]:off[1] + 8 * cells].view(np.float64).reshape(max_steps, batch)
    j = raw[off[2]:off[2] + 4 * cells].view(np.int32).reshape(max_steps, batch)
    y = raw[off[3]:off[3] + 4 * cells * latent_dim].view(np.float32).reshape(max_steps, batch, latent_dim)
    counts = n_accepted.cpu().tolist()
    return [{"t": t[:n, p].tolist(), "dt": dt[:n, p].tolist(), "j": j[:n, p].tolist(), "y": y[:n, p].copy()}
            for p, n in enumerate(counts)]
