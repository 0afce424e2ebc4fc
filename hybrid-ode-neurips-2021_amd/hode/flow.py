"""Planar normalizing-flow posterior with its Monte-Carlo KL (``hode_flow_fwd`` / ``hode_flow_bwd``, libhode_flow.so):
reference ``EncoderPlanarLSTM.reparameterize`` / ``log_density`` (``model.py:116-153``), ``Planar.forward``
(``flow.py:26-59``) and ``VariationalInferenceFlow.mc_kl`` (``model.py:1366-1380``) as one forward and one backward
launch instead of ~20 element-wise launches per flow and draw plus their autograd graph."""

from __future__ import annotations

import torch

from . import _flow_lib as F
from ._lib import HodeConfigError
from .solver import _f32c, _ptr, _require_gpu, _stream


def check_domain(B, D, K, S, s_kl):
    """Raise HodeConfigError outside the kernels' domain (include/hode_flow.h); there is no fallback."""
    if B < 1:
        raise HodeConfigError("hode.flow: batch %d must be >= 1" % B)
    if not 1 <= D <= F.MAX_LATENT:
        raise HodeConfigError("hode.flow: latent_dim %d outside 1..%d" % (D, F.MAX_LATENT))
    if not 1 <= K <= F.MAX_FLOWS:
        raise HodeConfigError("hode.flow: n_flows %d outside 1..%d" % (K, F.MAX_FLOWS))
    if not 1 <= S <= F.MAX_SAMPLES:
        raise HodeConfigError("hode.flow: n_samples %d outside 1..%d" % (S, F.MAX_SAMPLES))
    if s_kl not in (0, 1) or s_kl >= S:
        raise HodeConfigError("hode.flow: s_kl %r must be 0 or 1 and below n_samples %d" % (s_kl, S))


def _desc(mu, lv, u, w, b, noise, s_kl):
    S, B, D = noise.shape
    d = F.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl = B, D, u.shape[1], S, s_kl
    d.mu, d.log_var, d.u, d.w, d.b, d.noise = (x.data_ptr() for x in (mu, lv, u, w, b, noise))
    return d


class _PlanarFlowKL(torch.autograd.Function):
    """Gradients for mu, log_var, u, w, b; none for noise (its .grad stays None)."""

    @staticmethod
    def forward(ctx, mu, log_var, u, w, b, noise, s_kl, want_z):
        _require_gpu(mu, log_var, u, w, b, noise)
        ctx.set_materialize_grads(False)  # an unused output arrives as None: its gradient input stays NULL
        lib = F.lib()
        muc, lvc, uc, wc, bc, nc = (_f32c(x) for x in (mu, log_var, u, w, b, noise))
        S, B, D = nc.shape
        K = uc.shape[1]
        check_domain(B, D, K, S, s_kl)
        if muc.shape != (B, D) or lvc.shape != (B, D) or uc.shape != (B, K, D) or wc.shape != (B, K, D) or bc.shape != (B, K):
            raise HodeConfigError("hode.flow: shapes mu/log_var (B, D), u/w (B, K, D), b (B, K), noise (S, B, D) expected")
        z_out = torch.empty((S, B, D), device=muc.device, dtype=torch.float32) if want_z else None
        kl = torch.empty((B,), device=muc.device, dtype=torch.float32)
        d = _desc(muc, lvc, uc, wc, bc, nc, s_kl)
        d.z_out, d.kl = _ptr(z_out), kl.data_ptr()
        with torch.cuda.device(muc.device):
            F.check(lib.hode_flow_fwd(d, _stream()), "hode_flow_fwd")
        ctx.save_for_backward(muc, lvc, uc, wc, bc, nc)
        ctx.s_kl = s_kl
        if z_out is None:
            z_out = kl.new_zeros(())  # placeholder output: no gradient flows into it
            ctx.mark_non_differentiable(z_out)
        return z_out, kl

    @staticmethod
    def backward(ctx, g_z, g_kl):
        muc, lvc, uc, wc, bc, nc = ctx.saved_tensors
        if g_z is not None and g_z.dim() != 3:
            g_z = None
        if g_z is None and g_kl is None:
            return (None,) * 8
        gz = _f32c(g_z) if g_z is not None else None
        gk = _f32c(g_kl) if g_kl is not None else None
        d = _desc(muc, lvc, uc, wc, bc, nc, ctx.s_kl)
        g_mu, g_lv = torch.empty_like(muc), torch.empty_like(lvc)
        g_u, g_w, g_b = torch.empty_like(uc), torch.empty_like(wc), torch.empty_like(bc)
        d.grad_z_out, d.grad_kl = _ptr(gz), _ptr(gk)
        d.grad_mu, d.grad_log_var, d.grad_u, d.grad_w, d.grad_b = (x.data_ptr() for x in (g_mu, g_lv, g_u, g_w, g_b))
        with torch.cuda.device(muc.device):
            F.check(F.lib().hode_flow_bwd(d, _stream()), "hode_flow_bwd")
        return g_mu, g_lv, g_u, g_w, g_b, None, None, None


def planar_flow_sample(mu, log_var, u, w, b, noise, s_kl=1, want_z=True):
    """Planar-flow draws and their Monte-Carlo KL against the Exponential(100) prior, one kernel each way.

    mu, log_var (B, D); u, w (B, K, D) (or the encoder's (B, K, D, 1) / (B, K, 1, D) views); b (B, K) (or (B, K, 1, 1));
    noise (S, B, D) standard-normal draws.  Returns ``z_out`` (S, B, D) -- ``exp(z_K - 5)`` of every draw, ``None`` when
    ``want_z`` is False -- and ``kl`` (B,): the mean over draws ``s_kl .. S-1`` of ``log q(z) - log p(z)``."""
    B, D = mu.shape
    K = u.shape[1]
    z_out, kl = _PlanarFlowKL.apply(mu, log_var, u.reshape(B, K, D), w.reshape(B, K, D), b.reshape(B, K), noise,
                                    int(s_kl), bool(want_z))
    return (z_out if want_z else None), kl
