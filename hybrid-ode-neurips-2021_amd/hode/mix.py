"""Ensemble CRPS of a weighted sum of two models' forecasts on the GPU (``hode_mix_crps``, libhode_mix.so): the metric
loop of the reference's ``training_utils.evaluate_ensemble`` / ``evaluate_ensemble_horizon`` (``training_utils.py:383-565``)
as one kernel over posterior samples that each model integrated in ONE solver launch.  Evaluation only: no autograd."""

from __future__ import annotations

import torch

from . import _mix_lib as M
from .solver import _f32c, _require_gpu, _stream

THREADS, MAX_ROWS, PACK_LDS, LDS_LIMIT, STATIC_LDS = 128, 8, 64 * 1024, 160 * 1024, 128 * 4


def lds_bytes(rows, n_members, latent_e, latent_m, obs):
    """Dynamic LDS of a workgroup that owns ``rows`` forecast rows (csrc/mix/hode_mix.hip: mix_lds_bytes)."""
    return 4 * (rows * n_members * (latent_e + latent_m) + (latent_e + latent_m) * obs + n_members * THREADS)


def rows_per_workgroup(n_members, latent_e, latent_m, obs):
    """How many (time, patient) rows share a 128-thread workgroup (csrc/mix/hode_mix.hip: mix_rows_per_workgroup)."""
    rows = min(THREADS // obs, MAX_ROWS)
    while rows > 1 and lds_bytes(rows, n_members, latent_e, latent_m, obs) + STATIC_LDS > PACK_LDS:
        rows -= 1
    return rows


def supported(n_members, latent_e, latent_m, obs):
    """The library's domain: every dimension in 1 .. 128 and the workgroup's LDS within 160 KiB."""
    if not all(1 <= v <= M.MAX_DIM for v in (n_members, latent_e, latent_m, obs)):
        return False
    rows = rows_per_workgroup(n_members, latent_e, latent_m, obs)
    return lds_bytes(rows, n_members, latent_e, latent_m, obs) + STATIC_LDS <= LDS_LIMIT


def _readout(r, what):
    """(weight, bias or None) of an ``nn.Linear``-like module or of a (weight, bias) pair."""
    if isinstance(r, (tuple, list)):
        if len(r) != 2:
            raise ValueError("hode.mixture_crps: %s must be a module with .weight / .bias or a (weight, bias) pair" % what)
        return r[0], r[1]
    return r.weight, getattr(r, "bias", None)


def _table(w, Tn, obs, like, what):
    """A mixing weight as the (T', obs) table the kernel reads: None stays None (one), a number is broadcast."""
    if w is None:
        return None
    if not torch.is_tensor(w):
        return torch.full((Tn, obs), float(w), device=like.device, dtype=torch.float32)
    if tuple(w.shape) != (Tn, obs):
        raise ValueError("hode.mixture_crps: %s shape %s != (%d, %d)" % (what, tuple(w.shape), Tn, obs))
    return w


def mixture_crps(h_e, h_m, truth, n_members, readout_e, readout_m, weight_e=None, weight_m=None, per_component=False):
    """CRPS of the M-member ensemble ``weight_e * readout_e(h_e) + weight_m * readout_m(h_m)`` against ``truth``
    (T', B, obs).

    ``h_e`` (T', M * B, De) and ``h_m`` (T', M * B, Dm) have the batch axis member-major (index m * B + b), exactly what a
    decoder returns for ``z.reshape(M * B, D)`` built from ``torch.stack`` of M draws; the two latent widths are
    independent.  ``readout_*`` is each model's ``output_function[0]`` (or a (weight (obs, D), bias (obs,) or None) pair);
    neither readout is materialised.  ``weight_*`` is None (one), a number, or a (T', obs) table.
    Returns the per-(time, patient) SUM over components (T', B), or the full (T', B, obs) field if ``per_component``.
    """
    _require_gpu(h_e, h_m, truth)
    lib = M.lib()
    Tn, MB, De = h_e.shape
    Dm = h_m.shape[-1]
    n = int(n_members)
    if n < 1 or MB % n:
        raise ValueError("hode.mixture_crps: batch axis %d is not a multiple of n_members %d" % (MB, n))
    B = MB // n
    obs = truth.shape[-1]
    if tuple(h_m.shape) != (Tn, MB, Dm):
        raise ValueError("hode.mixture_crps: h_m shape %s != (%d, %d, Dm)" % (tuple(h_m.shape), Tn, MB))
    if tuple(truth.shape) != (Tn, B, obs):
        raise ValueError("hode.mixture_crps: truth shape %s != (%d, %d, obs)" % (tuple(truth.shape), Tn, B))
    w_e, b_e = _readout(readout_e, "readout_e")
    w_m, b_m = _readout(readout_m, "readout_m")
    if tuple(w_e.shape) != (obs, De) or tuple(w_m.shape) != (obs, Dm):
        raise ValueError("hode.mixture_crps: readout weights %s / %s != (%d, %d) / (%d, %d)"
                         % (tuple(w_e.shape), tuple(w_m.shape), obs, De, obs, Dm))
    for b, what in ((b_e, "readout_e"), (b_m, "readout_m")):
        if b is not None and tuple(b.shape) != (obs,):
            raise ValueError("hode.mixture_crps: %s bias shape %s != (%d,)" % (what, tuple(b.shape), obs))
    g_e, g_m = _table(weight_e, Tn, obs, h_e, "weight_e"), _table(weight_m, Tn, obs, h_e, "weight_m")
    _require_gpu(w_e, b_e, w_m, b_m, g_e, g_m)
    if not supported(n, De, Dm, obs):
        raise M.HodeConfigError(
            "hode.mixture_crps: n_members %d, latent dims %d + %d, obs %d outside the kernel's domain (each 1..%d, "
            "workgroup LDS <= %d B)" % (n, De, Dm, obs, M.MAX_DIM, LDS_LIMIT))
    hec, hmc, tc = _f32c(h_e), _f32c(h_m), _f32c(truth)
    wec, wmc = _f32c(w_e), _f32c(w_m)
    bec = _f32c(b_e) if b_e is not None else None
    bmc = _f32c(b_m) if b_m is not None else None
    gec = _f32c(g_e) if g_e is not None else None
    gmc = _f32c(g_m) if g_m is not None else None
    d = M.new_desc()
    d.n_times, d.batch, d.n_members, d.obs_dim, d.latent_dim_e, d.latent_dim_m = Tn, B, n, obs, De, Dm
    d.time_stride_e, d.member_stride_e, d.patient_stride_e = MB * De, B * De, De
    d.time_stride_m, d.member_stride_m, d.patient_stride_m = MB * Dm, B * Dm, Dm
    d.h_e, d.h_m, d.truth = hec.data_ptr(), hmc.data_ptr(), tc.data_ptr()
    d.w_e, d.w_m = wec.data_ptr(), wmc.data_ptr()
    d.b_e = 0 if bec is None else bec.data_ptr()
    d.b_m = 0 if bmc is None else bmc.data_ptr()
    d.mix_e = 0 if gec is None else gec.data_ptr()
    d.mix_m = 0 if gmc is None else gmc.data_ptr()
    if per_component:
        out = torch.empty((Tn, B, obs), device=h_e.device, dtype=torch.float32)
        d.crps = out.data_ptr()
    else:
        out = torch.empty((Tn, B), device=h_e.device, dtype=torch.float32)
        d.crps_sum = out.data_ptr()
    with torch.cuda.device(h_e.device):
        M.check(lib.hode_mix_crps(d, _stream()), "hode_mix_crps")
    return out
