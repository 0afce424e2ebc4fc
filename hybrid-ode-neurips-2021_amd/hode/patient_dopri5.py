"""dopri5 with PER-PATIENT step control for the hybrid Roche rhs (``hode_dopri5_pp_fwd`` / ``hode_dopri5_pp_bwd``,
libhode_dopri5_pp.so): every patient carries its own controller -- Hairer's first step, an RMS error norm over its own D
components, accept / reject, dense output, an accepted-step tape of its own -- which is ``torchdiffeq.odeint`` run on each
patient as a batch of one.  The whole forward is ONE launch (a lane per patient, the attempt loop in registers), the
backward a second one over the per-patient tapes.  ``hode.adaptive.roche_dopri5`` keeps torchdiffeq's batch-global
controller (one norm over B*D, one dt for everybody, one launch per attempt) and stays the default.

The one difference from "torchdiffeq on a batch of one": the backward treats every step size as a constant, dt_0 included
(``detach_first_step=True`` of ``roche_dopri5``); the derivative of Hairer's initial step is not formed.

Two plain launch functions; the ``torch.autograd.Function`` that joins them lives next to the module it serves, in the
package-root ``model.py`` (``RocheODE.step_control = "patient"``)."""

from __future__ import annotations

import ctypes as C

import torch

from . import _dopri5_pp_lib as PL
from . import _lib as L
from .solver import _f32c, _i32c, _ptr, _require_gpu, _stream

#: the last forward: per-patient device tensors "n_accepted", "n_rejected", "status" (B,) int32, and the host values
#: "no_tape", "max_steps", "workspace_bytes"
last_stats = {}


def check_domain(latent_dim, n_dose=1):
    """Raise HodeConfigError outside the kernels' domain, before a library is loaded or anything is launched."""
    if int(latent_dim) not in PL.DIMS:
        raise L.HodeConfigError("hode.patient_dopri5: per-patient step control is compiled for %s (got latent dimension %d); "
                                "there is no torch-eager path in the product" % (PL.sizes_text(), latent_dim))
    if int(n_dose) < 1:
        raise L.HodeConfigError("hode.patient_dopri5: at least one dose per patient is needed (got %d); have %s"
                                % (n_dose, PL.sizes_text()))


def _status_error(status):
    msgs = []
    if status & L.STATUS_NONFINITE:
        msgs.append("non-finite values in state `y`")
    if status & L.STATUS_DT_UNDERFLOW:
        msgs.append("underflow in dt")
    return "; ".join(msgs)


def patient_dopri5_forward(y0, theta, w, b, t, dosage, dose_times, rtol=1e-7, atol=1e-9, ablate=False, max_steps=0,
                           max_attempts=0, no_tape=False):
    """The forward launch.  y0 (B, D); theta the packed [16] vector; w (D-4, D), b (D-4,) or None when D == 4; t (T,);
    dosage (B,); dose_times (B, K).  Returns ``(h (T, B, D), tape_ws, stats)``: ``tape_ws`` is the int32 workspace tensor
    that holds the per-patient tapes for ``patient_dopri5_backward`` (without a tape when ``no_tape``: pass that when nothing
    needs a gradient -- the caller samples grad mode, as ``roche_dopri5`` does), ``stats`` is ``last_stats``.

    ``max_steps`` (accepted steps per patient = rows of the tape, default ``16 T + 64``) is multiplied by 4 and the solve
    repeated while only MAX_STEPS is set, and refused once the tape no longer fits the device; ``max_attempts`` bounds the
    attempts of a patient (default ``8 max_steps + 1024``).  A failing status raises HodeError (a RuntimeError) with the texts
    of the batch-global path plus the index of the first failing patient."""
    _require_gpu(y0, theta, t, dosage, dose_times, w, b)
    if dose_times.dim() != 2:
        dose_times = dose_times.reshape(y0.shape[0], -1)
    B, D = y0.shape
    T = t.numel()
    check_domain(D, dose_times.shape[1])
    lib = PL.lib()
    y0c, thc, tc, dosc, dtc = _f32c(y0), _f32c(theta), _f32c(t), _f32c(dosage), _f32c(dose_times)
    wc = _f32c(w) if w is not None else None
    bc = _f32c(b) if b is not None else None
    h = torch.empty((T, B, D), device=y0c.device, dtype=torch.float32)
    steps = int(max_steps) if max_steps else 16 * T + 64
    while True:
        status = torch.zeros(1, device=y0c.device, dtype=torch.int32)
        nacc = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        nrej = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        pst = torch.zeros(B, device=y0c.device, dtype=torch.int32)
        d = PL.new_desc()
        d.rhs_kind = L.RHS_ROCHE_ABLATE if ablate else L.RHS_ROCHE
        d.batch, d.latent_dim, d.n_times, d.n_dose = B, D, T, dtc.shape[1]
        d.t, d.y0, d.dosage, d.dose_times, d.theta = tc.data_ptr(), y0c.data_ptr(), dosc.data_ptr(), dtc.data_ptr(), thc.data_ptr()
        d.w1, d.b1 = _ptr(wc), _ptr(bc)
        d.rtol, d.atol = float(rtol), float(atol)
        d.h, d.status = h.data_ptr(), status.data_ptr()
        d.n_accepted, d.n_rejected, d.patient_status = nacc.data_ptr(), nrej.data_ptr(), pst.data_ptr()
        d.max_steps, d.max_attempts = steps, int(max_attempts)
        d.flags = L.FLAG_NO_TAPE if no_tape else 0
        nbytes = lib.hode_dopri5_pp_workspace_bytes(d)
        free, _ = torch.cuda.mem_get_info(y0c.device)
        if nbytes > free + torch.cuda.memory_reserved(y0c.device) - torch.cuda.memory_allocated(y0c.device):
            raise L.HodeError("hode dopri5 (per-patient step control): tapes of %d accepted steps need %.1f GB, the device "
                              "has %.1f GB free (max_num_steps exceeded)" % (steps, nbytes / 1e9, free / 1e9))
        ws = torch.empty(nbytes // 4, device=y0c.device, dtype=torch.int32)
        d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
        with torch.cuda.device(y0c.device):
            PL.check(lib.hode_dopri5_pp_fwd(d, _stream()), "hode_dopri5_pp_fwd")
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
        raise L.HodeError("hode dopri5 (per-patient step control): %s (first failing patient: %d)"
                          % (_status_error(st) or "max_num_steps exceeded", first))
    return h, ws, last_stats


def patient_dopri5_backward(y0, theta, w, b, t, dosage, dose_times, h, tape_ws, n_accepted, max_steps, grad_h, rtol=1e-7,
                            atol=1e-9, ablate=False, need_theta=True):
    """The backward launch for the inputs of a ``patient_dopri5_forward`` call, the ``h`` and ``tape_ws`` it returned and
    its ``stats["n_accepted"]`` / ``stats["max_steps"]``.  Returns ``(grad_y0, grad_theta or None, grad_w, grad_b)``; the
    parameter gradients are reduced per wave and folded in a fixed order (bit-identical repeats)."""
    _require_gpu(y0, theta, t, dosage, dose_times, w, b, h, tape_ws, n_accepted, grad_h)
    if dose_times.dim() != 2:
        dose_times = dose_times.reshape(y0.shape[0], -1)
    B, D = y0.shape
    T = t.numel()
    check_domain(D, dose_times.shape[1])
    lib = PL.lib()
    y0c, thc, tc, dosc, dtc = _f32c(y0), _f32c(theta), _f32c(t), _f32c(dosage), _f32c(dose_times)
    wc = _f32c(w) if w is not None else None
    bc = _f32c(b) if b is not None else None
    hc, gh = _f32c(h), _f32c(grad_h)
    ws, nacc = _i32c(tape_ws, "tape_ws"), _i32c(n_accepted, "n_accepted")
    if gh.shape != (T, B, D) or nacc.shape != (B,):
        raise L.HodeConfigError("hode.patient_dopri5: grad_h (T, B, D) and n_accepted (B,) expected")
    gy0 = torch.empty((B, D), device=y0c.device, dtype=torch.float32)
    gth = torch.zeros(L.N_THETA, device=y0c.device, dtype=torch.float32)
    gw = torch.zeros_like(wc) if wc is not None else None
    gb = torch.zeros_like(bc) if bc is not None else None
    scratch = torch.zeros((3, B), device=y0c.device, dtype=torch.int32)  # status word, rejected counts, patient status: unused here
    d = PL.new_desc()
    d.rhs_kind = L.RHS_ROCHE_ABLATE if ablate else L.RHS_ROCHE
    d.batch, d.latent_dim, d.n_times, d.n_dose = B, D, T, dtc.shape[1]
    d.t, d.y0, d.dosage, d.dose_times, d.theta = tc.data_ptr(), y0c.data_ptr(), dosc.data_ptr(), dtc.data_ptr(), thc.data_ptr()
    d.w1, d.b1 = _ptr(wc), _ptr(bc)
    d.rtol, d.atol = float(rtol), float(atol)
    d.h, d.status = hc.data_ptr(), scratch.data_ptr()
    d.n_accepted = nacc.data_ptr()
    d.n_rejected = d.patient_status = scratch.data_ptr()
    d.need_theta_grad = int(bool(need_theta))
    d.max_steps = int(max_steps)
    d.grad_h, d.grad_y0 = gh.data_ptr(), gy0.data_ptr()
    d.grad_w1, d.grad_b1, d.grad_theta = _ptr(gw), _ptr(gb), gth.data_ptr()
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    with torch.cuda.device(y0c.device):
        PL.check(lib.hode_dopri5_pp_bwd(d, _stream()), "hode_dopri5_pp_bwd")
    return gy0, (gth if need_theta else None), gw, gb


def read_tape(tape_ws, batch, latent_dim, max_steps, n_accepted):
    """Tests only: the per-patient accepted-step tapes out of a forward's workspace, at the offsets
    ``hode_dopri5_pp_tape_offsets`` reports -- a list over patients of ``{"t", "dt"}`` (float64 lists) and ``"j"`` (first /
    one-past-last output index per step)."""
    import numpy as np
    d = PL.new_desc()
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.max_steps = int(batch), int(latent_dim), 1, 1, int(max_steps)
    off = (C.c_size_t * 5)()
    PL.check(PL.lib().hode_dopri5_pp_tape_offsets(d, off), "hode_dopri5_pp_tape_offsets")
    raw = tape_ws.cpu().numpy().view(np.uint8)
    cells = int(max_steps) * int(batch)
    t = raw[off[1]:off[1] + 8 * cells].view(np.float64).reshape(max_steps, batch)
    dt = raw[off[2]:off[2] + 8 * cells].view(np.float64).reshape(max_steps, batch)
    j = raw[off[3]:off[3] + 8 * cells].view(np.int32).reshape(max_steps, batch, 2)
    counts = n_accepted.cpu().tolist()
    return [{"t": t[:n, p].tolist(), "dt": dt[:n, p].tolist(), "j": j[:n, p].tolist()} for p, n in enumerate(counts)]
