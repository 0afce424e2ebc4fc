"""The Sylvester-flow posterior with its Monte-Carlo KL (``hode_snf_fwd`` / ``hode_snf_bwd``, libhode_snf.so): the encoder's
raw heads in, the flow draws ``exp(z_K - 5)`` and the per-patient KL against the Exponential(100) prior out, one forward
and one backward launch.  The masks, the tanh diagonals, the Householder product, ``z0 = eps * sigma + mu``, the chain of
flows, the output layer and the KL all run inside the kernels; r1, r2 and Q never exist in device memory.  Two plain
launch functions; the ``torch.autograd.Function`` that joins them lives next to its caller, in the package-root
``flow.py``."""

from __future__ import annotations

import torch

from . import _snf_lib as NL
from ._lib import HodeConfigError
from .solver import _f32c, _ptr, _require_gpu, _stream

_SHAPES = ("hode.snf: shapes mu/log_var (B, D), full_d (B, K, D, D), diag1/diag2/bias (B, K, D), v (B, K, H, D) or None, "
           "noise (S, B, D) expected")


def check_domain(B, D, K, S, H, s_kl):
    """Raise HodeConfigError outside the kernels' domain (include/hode_snf.h); there is no fallback."""
    if B < 1:
        raise HodeConfigError("hode.snf: batch %d must be >= 1" % B)
    if not 1 <= D <= NL.MAX_LATENT:
        raise HodeConfigError("hode.snf: latent_dim %d outside 1..%d" % (D, NL.MAX_LATENT))
    if not 1 <= K <= NL.MAX_FLOWS:
        raise HodeConfigError("hode.snf: n_flows %d outside 1..%d" % (K, NL.MAX_FLOWS))
    if not 1 <= S <= NL.MAX_SAMPLES:
        raise HodeConfigError("hode.snf: n_samples %d outside 1..%d" % (S, NL.MAX_SAMPLES))
    if not 0 <= H <= NL.MAX_HOUSEHOLDER:
        raise HodeConfigError("hode.snf: n_householder %d outside 0..%d" % (H, NL.MAX_HOUSEHOLDER))
    if int(s_kl) != s_kl or not 0 <= s_kl < S:
        raise HodeConfigError("hode.snf: s_kl %r must be an integer in 0..n_samples-1 = %d" % (s_kl, S - 1))


def _shapes(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl):
    if noise.dim() != 3 or full_d.dim() != 4 or (v is not None and v.dim() != 4):
        raise HodeConfigError(_SHAPES)
    S, B, D = noise.shape
    K = full_d.shape[1]
    H = 0 if v is None else v.shape[2]
    if v is not None and H == 0:
        raise HodeConfigError("hode.snf: v with no Householder vectors; pass None for the triangular type")
    check_domain(B, D, K, S, H, s_kl)
    if mu.shape != (B, D) or log_var.shape != (B, D) or full_d.shape != (B, K, D, D) or diag1.shape != (B, K, D) \
            or diag2.shape != (B, K, D) or bias.shape != (B, K, D) or (v is not None and v.shape != (B, K, H, D)):
        raise HodeConfigError(_SHAPES)
    return S, B, D, K, H


def workspace_bytes(B, D, K, S):
    """Bytes of the workspace of one forward / backward pair: the states z_0 .. z_K of every draw and the backward's
    running cotangent, (K + 2) S B D floats rounded up to 256 bytes."""
    check_domain(B, D, K, S, 0, 0)
    d = NL.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples = B, D, K, S
    return int(NL.lib().hode_snf_workspace_bytes(d))


def snf_forward(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl=1, want_z=True):
    """The forward launch.  mu, log_var (B, D); full_d (B, K, D, D); diag1, diag2, bias (B, K, D); v (B, K, H, D) or None
    (the triangular type); noise (S, B, D).  Returns ``(z_out (S, B, D) or None, kl (B,), workspace)``: ``workspace`` is
    the float32 buffer ``snf_backward`` reads the states from."""
    _require_gpu(mu, log_var, full_d, diag1, diag2, bias, v, noise)
    lib = NL.lib()
    muc, lvc, fdc, d1c, d2c, bc, nc = _f32c(mu), _f32c(log_var), _f32c(full_d), _f32c(diag1), _f32c(diag2), _f32c(bias), _f32c(noise)
    vc = _f32c(v) if v is not None else None
    S, B, D, K, H = _shapes(muc, lvc, fdc, d1c, d2c, bc, vc, nc, s_kl)
    d = NL.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl, d.n_householder = B, D, K, S, int(s_kl), H
    d.mu, d.log_var, d.full_d, d.diag1, d.diag2 = muc.data_ptr(), lvc.data_ptr(), fdc.data_ptr(), d1c.data_ptr(), d2c.data_ptr()
    d.bias, d.v, d.noise = bc.data_ptr(), _ptr(vc), nc.data_ptr()
    z_out = torch.empty((S, B, D), device=muc.device, dtype=torch.float32) if want_z else None
    kl = torch.empty((B,), device=muc.device, dtype=torch.float32)
    ws = torch.empty((lib.hode_snf_workspace_bytes(d) // 4,), device=muc.device, dtype=torch.float32)
    d.z_out, d.kl, d.workspace, d.workspace_bytes = _ptr(z_out), kl.data_ptr(), ws.data_ptr(), ws.numel() * 4
    with torch.cuda.device(muc.device):
        NL.check(lib.hode_snf_fwd(d, _stream()), "hode_snf_fwd")
    return z_out, kl, ws


def snf_backward(mu, log_var, full_d, diag1, diag2, bias, v, noise, workspace, s_kl=1, grad_z=None, grad_kl=None):
    """The backward launch for the inputs of a ``snf_forward`` call and the ``workspace`` it returned.  Cotangents
    ``grad_z`` (S, B, D) and ``grad_kl`` (B,), each or None (zero).  Returns ``(grad_mu, grad_log_var, grad_full_d,
    grad_diag1, grad_diag2, grad_bias, grad_v or None)``; the sums over the S draws are formed in a fixed order
    (bit-identical repeats).  Only the cotangent part of the workspace is written: the call may be repeated."""
    _require_gpu(mu, log_var, full_d, diag1, diag2, bias, v, noise, workspace, grad_z, grad_kl)
    lib = NL.lib()
    muc, lvc, fdc, d1c, d2c, bc, nc = _f32c(mu), _f32c(log_var), _f32c(full_d), _f32c(diag1), _f32c(diag2), _f32c(bias), _f32c(noise)
    vc = _f32c(v) if v is not None else None
    ws = _f32c(workspace)
    gz = _f32c(grad_z) if grad_z is not None else None
    gk = _f32c(grad_kl) if grad_kl is not None else None
    S, B, D, K, H = _shapes(muc, lvc, fdc, d1c, d2c, bc, vc, nc, s_kl)
    if (gz is not None and gz.shape != (S, B, D)) or (gk is not None and gk.shape != (B,)):
        raise HodeConfigError("hode.snf: cotangents grad_z (S, B, D), grad_kl (B,) expected")
    d = NL.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl, d.n_householder = B, D, K, S, int(s_kl), H
    d.mu, d.log_var, d.full_d, d.diag1, d.diag2 = muc.data_ptr(), lvc.data_ptr(), fdc.data_ptr(), d1c.data_ptr(), d2c.data_ptr()
    d.bias, d.v, d.noise = bc.data_ptr(), _ptr(vc), nc.data_ptr()
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.grad_z_out, d.grad_kl = _ptr(gz), _ptr(gk)
    g_mu, g_lv, g_fd = torch.empty_like(muc), torch.empty_like(lvc), torch.empty_like(fdc)
    g_d1, g_d2, g_b = torch.empty_like(d1c), torch.empty_like(d2c), torch.empty_like(bc)
    g_v = torch.empty_like(vc) if vc is not None else None
    d.grad_mu, d.grad_log_var, d.grad_full_d = g_mu.data_ptr(), g_lv.data_ptr(), g_fd.data_ptr()
    d.grad_diag1, d.grad_diag2, d.grad_bias, d.grad_v = g_d1.data_ptr(), g_d2.data_ptr(), g_b.data_ptr(), _ptr(g_v)
    with torch.cuda.device(muc.device):
        NL.check(lib.hode_snf_bwd(d, _stream()), "hode_snf_bwd")
    return g_mu, g_lv, g_fd, g_d1, g_d2, g_b, g_v
