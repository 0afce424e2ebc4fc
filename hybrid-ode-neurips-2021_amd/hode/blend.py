"""Scoring of the real-data two-model baselines on the GPU (libhode_blend.so): the per-step stacking fit of the
reference's ``experiments/run_real_ensemble.py:109-117`` (``nnls2_weights``: one launch instead of a torch -> numpy ->
``scipy.optimize.nnls`` round trip per forecast step) and the four-horizon masked squared error of a weighted blend,
the tail of ``run_real.py``, ``run_real_ensemble.py`` and ``run_real_residual.py`` (``horizon_sse``: every input read
once, all horizons accumulated as prefixes).  Evaluation only: no autograd."""

from __future__ import annotations

import torch

from . import _blend_lib as BL
from .solver import _f32c, _require_gpu, _stream


def _refuse(msg):
    raise BL.HodeConfigError("hode.blend: " + msg)


def _same_shape(ref, what, **tensors):
    for name, x in tensors.items():
        if x is not None and tuple(x.shape) != tuple(ref.shape):
            _refuse("%s shape %s != %s shape %s" % (name, tuple(x.shape), what, tuple(ref.shape)))


def nnls2_weights(x_e, x_m, truth):
    """Per forecast step ``i`` the non-negative ``(w_e[i], w_m[i])`` that minimise
    ``sum((w_e x_e[i] + w_m x_m[i] - truth[i]) ** 2)`` over the step's ``B * obs`` entries (no mask, as in the reference).
    ``x_e``, ``x_m``, ``truth``: (T', B, obs).  Returns two (T',) float32 tensors; an inactive weight is exactly 0."""
    if x_e.dim() != 3 or min(x_e.shape) < 1:
        _refuse("x_e must be (T', B, obs) with every dimension >= 1, got %s" % (tuple(x_e.shape),))
    _same_shape(x_e, "x_e", x_m=x_m, truth=truth)
    Tn, B, obs = x_e.shape
    if B * obs > 2 ** 31 - 1:
        _refuse("B * obs = %d exceeds 2^31 - 1" % (B * obs))
    _require_gpu(x_e, x_m, truth)
    lib = BL.lib()
    xec, xmc, tc = _f32c(x_e), _f32c(x_m), _f32c(truth)
    w = torch.empty((Tn, 2), device=x_e.device, dtype=torch.float32)
    d = BL.new_desc(BL.Nnls2Desc)
    d.n_steps, d.rows = Tn, B * obs
    d.step_stride_e = d.step_stride_m = d.step_stride_b = B * obs
    d.x_e, d.x_m, d.truth, d.w = xec.data_ptr(), xmc.data_ptr(), tc.data_ptr(), w.data_ptr()
    with torch.cuda.device(x_e.device):
        BL.check(lib.hode_blend_nnls2(d, _stream()), "hode_blend_nnls2")
    return w[:, 0], w[:, 1]


def _table(w, Tn, obs, like, what):
    """A mixing weight as the (T', obs) table the kernel reads: None stays None (one); a number, a (T',) table and a
    (T', 1, obs) tensor are broadcast."""
    if w is None:
        return None
    if not torch.is_tensor(w):
        return torch.full((Tn, obs), float(w), device=like.device, dtype=torch.float32)
    if w.dim() == 0:
        return w.to(torch.float32).expand(Tn, obs)
    if tuple(w.shape) == (Tn,):
        return w[:, None].expand(Tn, obs)
    if tuple(w.shape) == (Tn, 1, obs):
        return w[:, 0, :]
    if tuple(w.shape) != (Tn, obs):
        _refuse("%s shape %s is none of (%d,), (%d, %d), (%d, 1, %d)" % (what, tuple(w.shape), Tn, Tn, obs, Tn, obs))
    return w


def horizon_sse(x_e, truth, mask, horizons, x_m=None, weight_e=None, weight_m=None):
    """Masked squared error of the forecast ``weight_e * x_e + weight_m * x_m`` (``x_m`` None: ``weight_e * x_e`` alone)
    per patient, summed over the forecast steps ``t < n`` and the components, for every horizon end ``n`` of ``horizons``
    (forecast steps, non-decreasing, at most 8; each is clipped to T').  ``x_e``, ``x_m``, ``truth``, ``mask``:
    (T', B, obs).  A weight is None (one), a number, a (T',) table, a (T', obs) table or a (T', 1, obs) tensor.
    Returns ``(sse, cnt)``, each (H, B) float32: ``sse / cnt`` is a patient's mean squared error over a horizon (NaN for a
    patient without an observation there)."""
    if x_e.dim() != 3 or min(x_e.shape) < 1:
        _refuse("x_e must be (T', B, obs) with every dimension >= 1, got %s" % (tuple(x_e.shape),))
    _same_shape(x_e, "x_e", x_m=x_m, truth=truth, mask=mask)
    Tn, B, obs = x_e.shape
    ends = [int(n) for n in horizons]
    if not 1 <= obs <= BL.MAX_OBS:
        _refuse("obs %d outside 1..%d" % (obs, BL.MAX_OBS))
    if not 1 <= len(ends) <= BL.MAX_HORIZONS:
        _refuse("%d horizons, outside 1..%d" % (len(ends), BL.MAX_HORIZONS))
    if ends[0] < 1 or any(b < a for a, b in zip(ends, ends[1:])):
        _refuse("horizons %s must be >= 1 and non-decreasing" % (ends,))
    if Tn * B > 2 ** 31 - 1:
        _refuse("T' * B = %d exceeds 2^31 - 1" % (Tn * B))
    if x_m is None and weight_m is not None:
        _refuse("weight_m without x_m")
    g_e, g_m = _table(weight_e, Tn, obs, x_e, "weight_e"), _table(weight_m, Tn, obs, x_e, "weight_m")
    _require_gpu(x_e, x_m, truth, mask, g_e, g_m)
    lib = BL.lib()
    xec, tc, mc = _f32c(x_e), _f32c(truth), _f32c(mask)
    xmc = _f32c(x_m) if x_m is not None else None
    gec = _f32c(g_e) if g_e is not None else None
    gmc = _f32c(g_m) if g_m is not None else None
    sse = torch.empty((len(ends), B), device=x_e.device, dtype=torch.float32)
    cnt = torch.empty((len(ends), B), device=x_e.device, dtype=torch.float32)
    d = BL.new_desc(BL.HorizonDesc)
    d.n_times, d.batch, d.obs_dim, d.n_horizons = Tn, B, obs, len(ends)
    for h, n in enumerate(ends):
        d.horizons[h] = min(n, Tn)
    d.time_stride, d.patient_stride = B * obs, obs
    d.x_e, d.truth, d.mask = xec.data_ptr(), tc.data_ptr(), mc.data_ptr()
    d.x_m = 0 if xmc is None else xmc.data_ptr()
    d.w_e = 0 if gec is None else gec.data_ptr()
    d.w_m = 0 if gmc is None else gmc.data_ptr()
    d.sse, d.cnt = sse.data_ptr(), cnt.data_ptr()
    with torch.cuda.device(x_e.device):
        BL.check(lib.hode_blend_horizon_sse(d, _stream()), "hode_blend_horizon_sse")
    return sse, cnt
