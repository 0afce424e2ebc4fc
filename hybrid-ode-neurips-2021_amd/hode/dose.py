"""Dose gradients of the fixed-grid hybrid solve (``hode_dose_bwd``, libhode_dose.so): the discrete adjoint of euler /
midpoint / 3/8-rule rk4 over the Roche rhs that, beside the gradients ``hode_rk_bwd`` gives (y0, theta, w, b), carries one
more per-lane accumulator and returns d loss / d dosage of every patient.  With ``g`` the cotangent handed to the rhs' VJP at
a stage evaluated at time ``ts``,

    gdosage[p] += g[3] * kel * s_p(ts),    s_p(t) = sum_k 1[t >= tau_k] exp(kel (tau_k - t)),

the dose schedule at unit dosage: it does not depend on the dosage, so a patient whose dosage is 0 has a well-defined
gradient; under ``ablate`` the dose does not enter the rhs and the gradient is exactly 0.  One lane per patient, stages
recomputed from ``h``, no atomics: repeats are bit-identical.

Out of its domain, each refused with a message: dopri5 (either step control), the quad and split layouts, latent sizes other
than 4, 6, 8, 12, the NeuralODE and real-data rhs, and gradients with respect to the dose times or ``t``.

One plain launch function; the ``torch.autograd.Function`` that joins it to the forward lives next to the module it serves,
in the package-root ``model.py`` (``RocheODE.dose_grad = True``)."""

from __future__ import annotations

import torch

from . import _dose_lib as DL
from . import _lib as L
from .solver import _f32c, _ptr, _require_gpu, _stream


def check_domain(latent_dim, n_dose=1):
    """Raise HodeConfigError outside the kernels' domain, before a library is loaded or anything is launched."""
    if int(latent_dim) not in DL.DIMS:
        raise L.HodeConfigError("hode.dose: dose gradients are compiled for %s (got latent dimension %d); "
                                "there is no torch-eager path in the product" % (DL.sizes_text(), latent_dim))
    if int(n_dose) < 1:
        raise L.HodeConfigError("hode.dose: at least one dose per patient is needed (got %d); have %s" % (n_dose, DL.sizes_text()))


def dose_backward(h, theta, w, b, t, dosage, dose_times, grad_h, method="rk4", ablate=False, perturb=False, need_theta=True):
    """The backward launch for a fixed-grid forward ``h = hode.roche_solve(y0, theta, w, b, t, dosage, dose_times, method,
    ablate, perturb)``: h (T, B, D); theta the packed [16] vector; w (D-4, D), b (D-4,) or None when D == 4; t (T,);
    dosage (B,); dose_times (B, K); grad_h (T, B, D).  Returns ``(grad_y0, grad_theta or None, grad_w, grad_b, grad_dosage)``;
    the parameter gradients are reduced per wave and folded in a fixed order, ``grad_dosage[p]`` is written by patient p's
    own lane."""
    if method not in L.METHODS:
        raise L.HodeConfigError("hode.dose: method %r is not a fixed-grid method; dose gradients serve %s" % (method, DL.sizes_text()))
    _require_gpu(h, theta, t, dosage, dose_times, w, b, grad_h)
    T, B, D = h.shape
    if dose_times.dim() != 2:
        dose_times = dose_times.reshape(B, -1)
    check_domain(D, dose_times.shape[1])
    lib = DL.lib()
    hc, thc, tc, dosc, dtc, gh = _f32c(h), _f32c(theta), _f32c(t), _f32c(dosage), _f32c(dose_times), _f32c(grad_h)
    wc = _f32c(w) if w is not None else None
    bc = _f32c(b) if b is not None else None
    if gh.shape != (T, B, D) or tc.numel() != T or dosc.shape != (B,):
        raise L.HodeConfigError("hode.dose: h and grad_h (T, B, D), t (T,) and dosage (B,) expected (got %s, %s, %s, %s)"
                                % (tuple(hc.shape), tuple(gh.shape), tuple(tc.shape), tuple(dosc.shape)))
    gy0 = torch.empty((B, D), device=hc.device, dtype=torch.float32)
    gdos = torch.empty(B, device=hc.device, dtype=torch.float32)
    gth = torch.zeros(L.N_THETA, device=hc.device, dtype=torch.float32)
    gw = torch.zeros_like(wc) if wc is not None else None
    gb = torch.zeros_like(bc) if bc is not None else None
    d = DL.new_desc()
    d.rhs_kind = L.RHS_ROCHE_ABLATE if ablate else L.RHS_ROCHE
    d.method, d.perturb = L.METHODS[method], int(bool(perturb))
    d.batch, d.latent_dim, d.n_times, d.n_dose = B, D, T, dtc.shape[1]
    d.need_theta_grad = int(bool(need_theta))
    d.t, d.h, d.dosage, d.dose_times, d.theta = tc.data_ptr(), hc.data_ptr(), dosc.data_ptr(), dtc.data_ptr(), thc.data_ptr()
    d.w1, d.b1 = _ptr(wc), _ptr(bc)
    d.grad_h, d.grad_y0, d.grad_dosage = gh.data_ptr(), gy0.data_ptr(), gdos.data_ptr()
    d.grad_w1, d.grad_b1, d.grad_theta = _ptr(gw), _ptr(gb), gth.data_ptr()
    nbytes = lib.hode_dose_workspace_bytes(d)
    ws = torch.empty(max(nbytes, 4) // 4, device=hc.device, dtype=torch.int32)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    with torch.cuda.device(hc.device):
        DL.check(lib.hode_dose_bwd(d, _stream()), "hode_dose_bwd")
    return gy0, (gth if need_theta else None), gw, gb, gdos
