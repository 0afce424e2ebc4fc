"""Fused Monte-Carlo KL against the Exponential prior (``hode_mc_kl_exponential``): reference ``VariationalInference.mc_kl``
(``model.py:1198-1214``) as one kernel with analytic gradients instead of ~40 element-wise launches per step."""

from __future__ import annotations

import torch

from . import _lib as L
from .solver import _f32c, _require_gpu, _stream


def _launch(mu, log_var, noise, rate, clamp_value, need):
    """kl and, if ``need``, (grad_mu, grad_log_var); without ``need`` the kernel gets NULL gradient pointers."""
    _require_gpu(mu, log_var, noise)
    lib = L.lib()
    muc, lvc, nc = _f32c(mu), _f32c(log_var), _f32c(noise)
    rows = muc.numel()
    if nc.dim() < 1 or nc.numel() != nc.shape[0] * rows:
        raise ValueError("hode.mc_kl_exponential: noise must be (S,) + mu.shape")
    kl = torch.empty_like(muc)
    d = L.McKlDesc()
    d.struct_size = L.C.sizeof(L.McKlDesc)
    d.n_samples, d.rows, d.rate, d.clamp_value = nc.shape[0], rows, float(rate), float(clamp_value)
    d.mu, d.log_var, d.noise, d.kl = muc.data_ptr(), lvc.data_ptr(), nc.data_ptr(), kl.data_ptr()
    gmu = glv = None
    if need:
        gmu, glv = torch.empty_like(muc), torch.empty_like(muc)
        d.grad_mu, d.grad_log_var = gmu.data_ptr(), glv.data_ptr()
    with torch.cuda.device(mu.device):
        L.check(lib.hode_mc_kl_exponential(d, _stream()), "hode_mc_kl_exponential")
    return kl, gmu, glv


class _McKlExp(torch.autograd.Function):
    """Gradients for mu and log_var; none for noise (its .grad stays None)."""

    @staticmethod
    def forward(ctx, mu, log_var, noise, rate, clamp_value):
        kl, gmu, glv = _launch(mu, log_var, noise, rate, clamp_value, True)
        ctx.save_for_backward(gmu, glv)
        return kl

    @staticmethod
    def backward(ctx, g):
        gmu, glv = ctx.saved_tensors
        return g * gmu, g * glv, None, None, None


def mc_kl_exponential(mu, log_var, noise, rate=100.0, clamp_value=torch.finfo(torch.float32).eps):
    """Per-element Monte-Carlo KL terms, shape of ``mu``; ``noise`` is (S,) + mu.shape standard-normal draws.
    Sum over the latent axis to get the reference's ``mc_kl`` output (B,).  Under ``torch.no_grad`` (or with neither
    input requiring a gradient) the kernel runs forward-only; otherwise it forms both gradients in the same pass."""
    if torch.is_grad_enabled() and (mu.requires_grad or log_var.requires_grad):
        return _McKlExp.apply(mu, log_var, noise, rate, clamp_value)
    return _launch(mu, log_var, noise, rate, clamp_value, False)[0]
