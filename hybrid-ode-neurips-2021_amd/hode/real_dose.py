"""Dose-table gradients of the real-data hybrid solve (``hode_real_dose_bwd``, libhode_real_dose.so): the discrete adjoint of
euler / midpoint / 3/8-rule rk4 over the real-data hybrid rhs that, beside the gradients ``hode.real``'s backward gives (y0,
the three scalars, the flat weights), returns d loss / d act of the table of hourly doses ``act`` (Ta, B).

The kernels evaluate ``Dose(t) = exp(kel (n - t)) S_n`` with ``n = min(Ta, floor(t))`` and ``S_n = act[n-1] + exp(-kel)
S_{n-1}``.  With ``gX`` the cotangent handed to the rhs' VJP at a stage evaluated at time ``ts`` and ``n >= 1``,

    S^_n += gX[3] * kel * exp(kel (n - ts)),    then for n = Ta .. 1:  grad_act[n-1] = S^_n,  S^_{n-1} += exp(-kel) S^_n.

The reverse sweep meets the stage times in non-increasing order, so the lane that carries a patient fuses the scan into the
sweep: every element of ``grad_act`` is written once by its own patient's lane, no atomics, repeats are bit-identical, and
rows at or after the last stage time are exactly zero.  A dose of 0 has a well-defined gradient.

Out of its domain, each refused with a message: dopri5, latent size 4 (the expert-only model, one patient per lane in
libhode.so) and sizes above 20, hidden sizes above 64, the one-step-ahead solve, and gradients with respect to ``t``.

One plain launch function; the ``torch.autograd.Function`` that joins it to the forward lives next to the module it serves,
in the package-root ``model.py`` (``RocheODEReal.dose_grad = True``)."""

from __future__ import annotations

import torch

from . import _lib as L
from . import _real_dose_lib as DL
from .solver import _f32c, _require_gpu, _stream


def check_domain(latent_dim, hidden_dim):
    """Raise HodeConfigError outside the kernels' domain, before a library is loaded or anything is launched."""
    if not DL.MIN_LATENT <= int(latent_dim) <= DL.MAX_LATENT:
        raise L.HodeConfigError("hode.real_dose: dose-table gradients are compiled for %s (got latent dimension %d); "
                                "there is no torch-eager path in the product" % (DL.sizes_text(), latent_dim))
    if not 1 <= int(hidden_dim) <= DL.MAX_HIDDEN:
        raise L.HodeConfigError("hode.real_dose: dose-table gradients are compiled for %s (got hidden dimension %d); "
                                "there is no torch-eager path in the product" % (DL.sizes_text(), hidden_dim))


def real_dose_backward(h, theta, wflat, t, act, grad_h, hidden, method="midpoint", perturb=True):
    """The backward launch for a fixed-grid forward ``h = hode.real.real_solve(y0, theta, wflat, t, act, hidden, method,
    perturb)``: h (T, B, D); theta (3,) = (k_immunity, kel, kel2); wflat all weights in creation order; t (T,); act (Ta, B);
    grad_h (T, B, D).  Returns ``(grad_y0, grad_theta[3], grad_wflat, grad_act[Ta][B])``; the parameter gradients are reduced
    per wave and folded in a fixed order, column p of ``grad_act`` is written by patient p's own lane."""
    if method not in L.METHODS:
        raise L.HodeConfigError("hode.real_dose: method %r is not a fixed-grid method; dose-table gradients serve %s"
                                % (method, DL.sizes_text()))
    _require_gpu(h, theta, wflat, t, act, grad_h)
    T, B, D = h.shape
    hidden = int(hidden)
    check_domain(D, hidden)
    lib = DL.lib()
    hc, thc, wc, tc, ac, gh = _f32c(h), _f32c(theta), _f32c(wflat), _f32c(t), _f32c(act), _f32c(grad_h)
    M = D - 4
    if gh.shape != (T, B, D) or tc.numel() != T or ac.dim() != 2 or ac.shape[1] != B or thc.numel() != 3 \
            or wc.numel() != 9 * hidden + 2 + 3 * M * M:
        raise L.HodeConfigError("hode.real_dose: h and grad_h (T, B, D), t (T,), act (Ta, B), theta (3,) and wflat (%d,) expected "
                                "(got %s, %s, %s, %s, %s, %s)" % (9 * hidden + 2 + 3 * M * M, tuple(hc.shape), tuple(gh.shape),
                                                                  tuple(tc.shape), tuple(ac.shape), tuple(thc.shape), tuple(wc.shape)))
    gy0 = torch.empty((B, D), device=hc.device, dtype=torch.float32)
    gact = torch.empty(ac.shape, device=hc.device, dtype=torch.float32)
    gth = torch.zeros(3, device=hc.device, dtype=torch.float32)
    gw = torch.zeros_like(wc)
    d = DL.new_desc()
    d.method, d.perturb = L.METHODS[method], int(bool(perturb))
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times = B, D, hidden, T, ac.shape[0]
    d.t, d.h, d.act, d.theta, d.wflat = tc.data_ptr(), hc.data_ptr(), ac.data_ptr(), thc.data_ptr(), wc.data_ptr()
    d.grad_h, d.grad_y0, d.grad_act = gh.data_ptr(), gy0.data_ptr(), gact.data_ptr()
    d.grad_wflat, d.grad_theta = gw.data_ptr(), gth.data_ptr()
    nbytes = lib.hode_real_dose_workspace_bytes(d)
    ws = torch.empty(max(nbytes, 4) // 4, device=hc.device, dtype=torch.int32)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    with torch.cuda.device(hc.device):
        DL.check(lib.hode_real_dose_bwd(d, _stream()), "hode_real_dose_bwd")
    return gy0, gth, gw, gact
