"""The reference's flow strategies (``flow.py``): ``Planar`` (``:8-59``), ``Sylvester`` (``:62-138``) and
``TriangularSylvester`` (``:141-219``), so that ``import flow`` resolves where the reference's ``model.py`` expects it.

``Planar`` is eager arithmetic: the training and evaluation hot path runs the whole planar stack with its Monte-Carlo KL
in ``hode.flow`` (libhode_flow.so), and this module is the per-draw call surface and the CPU path.  The Sylvester modules
run one fused kernel each way on HIP tensors (libhode_sylvester.so through ``hode.sylvester``, the K = 1, S = 1 case of
``sylvester_chain``) and eager arithmetic on CPU tensors; ``sylvester_chain`` is the K-flow, S-draw call.
``sylvester_posterior_sample`` is the Sylvester-flow posterior (LHM-SNF) built on them: the encoder's raw heads in, the
draws and their Monte-Carlo KL out, one fused kernel each way on HIP tensors (libhode_snf.so through ``hode.snf``)."""

import math

import torch
import torch.nn as nn


class Planar(nn.Module):
    """z' = z + u_hat tanh(w . z + b), u_hat = u + (m(w . u) - w . u) w / |w|^2, m(x) = -1 + softplus(x)
    (Rezende & Mohamed 2015, appendix A); amortized u (B, D, 1), w (B, 1, D), b (B, 1, 1), z (B, D)."""

    def __init__(self):
        super().__init__()
        self.h = nn.Tanh()
        self.softplus = nn.Softplus()

    def der_h(self, x):
        return 1 - self.h(x) ** 2

    def forward(self, zk, u, w, b):
        zk = zk.unsqueeze(2)
        uw = torch.bmm(w, u)
        m_uw = -1.0 + self.softplus(uw)
        w_norm_sq = torch.sum(w ** 2, dim=2, keepdim=True)
        u_hat = u + ((m_uw - uw) * w.transpose(2, 1) / w_norm_sq)
        wzb = torch.bmm(w, zk) + b
        z = (zk + u_hat * self.h(wzb)).squeeze(2)
        psi = w * self.der_h(wzb)
        log_det_jacobian = torch.log(torch.abs(1 + torch.bmm(psi, u_hat))).squeeze(2).squeeze(1)
        return z, log_det_jacobian


# --------------------------------------------------------------------------------------------------- Sylvester flows
class _SylvesterChain(torch.autograd.Function):
    """``hode.sylvester``'s two launches as one differentiable call.  Gradients for z0, r1, r2, b and q; none for perm."""

    @staticmethod
    def forward(ctx, z0, r1, r2, b, q, perm, want_log_diag):
        from hode.sylvester import sylvester_forward
        ctx.set_materialize_grads(False)  # an unused output arrives as None: its gradient input stays NULL
        z, logdet, log_diag, tape = sylvester_forward(z0, r1, r2, b, q, perm, want_log_diag,
                                                      save_tape=any(ctx.needs_input_grad))
        ctx.save_for_backward(z0, r1, r2, b, q, perm, tape)
        if log_diag is None:
            log_diag = logdet.new_zeros(())  # placeholder output: no gradient flows into it
            ctx.mark_non_differentiable(log_diag)
        return z, logdet, log_diag

    @staticmethod
    def backward(ctx, g_z, g_logdet, g_log_diag):
        if g_log_diag is not None and g_log_diag.dim() != 4:
            g_log_diag = None
        if g_z is None and g_logdet is None and g_log_diag is None:
            return (None,) * 7  # nothing to propagate: no launch
        from hode.sylvester import sylvester_backward
        z0, r1, r2, b, q, perm, tape = ctx.saved_tensors
        g_z0, g_r1, g_r2, g_b, g_q = sylvester_backward(z0, r1, r2, b, q, perm, tape, g_z, g_logdet, g_log_diag)
        return g_z0, g_r1, g_r2, g_b, g_q, None, None


def _sylvester_step_eager(z, r1, r2, b, q=None, perm=None):
    """One flow in eager arithmetic on z (..., B, D) with r1, r2 (B, M, M), b (B, M), q (B, D, M) or None, perm (D,) or
    None.  Returns z' and log_diag (..., B, M)."""
    zr = z.unsqueeze(-2)                                            # (..., B, 1, D)
    if q is not None:
        a = torch.matmul(zr, torch.bmm(q, r2.transpose(2, 1))) + b.unsqueeze(1)
        h = torch.tanh(a)
        z_new = torch.matmul(h, torch.bmm(q, r1).transpose(2, 1)) + zr
    else:
        z_per = zr if perm is None else zr[..., perm]
        a = torch.matmul(z_per, r2.transpose(2, 1)) + b.unsqueeze(1)
        h = torch.tanh(a)
        w = torch.matmul(h, r1.transpose(2, 1))
        if perm is not None:
            w = w[..., perm]  # the same index again: a forward gather, not the inverse permutation
        z_new = w + zr
    diag = torch.diagonal(r1, dim1=-2, dim2=-1) * torch.diagonal(r2, dim1=-2, dim2=-1)   # (B, M)
    # tanh a second time, as the reference's der_h does: autograd then adds the two paths into `a` in the reference's order
    log_diag = ((1 - torch.tanh(a) ** 2).squeeze(-2) * diag + 1.0).abs().log()
    return z_new.squeeze(-2), log_diag


def sylvester_chain(z0, r1, r2, b, q=None, perm=None, want_log_diag=False):
    """K Sylvester flows over S draws per patient, the flow parameters shared by the draws of a patient.

    z0 (S, B, D); r1, r2 (B, K, M, M), used as given (full matrices: no triangular mask is applied, and the conditions on
    their diagonals are the caller's); b (B, K, M).  Dense mode: q (B, K, D, M) with (ideally) orthonormal columns.
    Triangular mode: q None, M == D, and perm a (K, D) integer index or None (identity).  Per flow

        dense:       a = z q r2^T + b,      z' = z + tanh(a) r1^T q^T
        triangular:  a = z[p] r2^T + b,     w = tanh(a) r1^T,   z'[i] = z[i] + w[p[i]]
        log_diag[m] = log|1 + (1 - tanh(a)[m]^2) r1[m, m] r2[m, m]|

    In triangular mode the output is gathered with the same index p as the input, as the reference does: a forward
    gather, not the inverse permutation.  The two agree only for involutions such as the flip; for any other p this is
    not the flow z + P r1 tanh(r2 P^T z + b) and log_diag is not its Jacobian's diagonal.  Kept as the reference has it.

    Returns ``(z_K (S, B, D), logdet (S, B))`` or, with ``want_log_diag``, ``(z_K, logdet, log_diag (S, B, K, M))``;
    ``logdet`` is the sum of ``log_diag`` over flows and components.  HIP tensors run one fused kernel each way
    (domain: D, M 1 .. 32, K 1 .. 16, S 1 .. 256, B >= 1; outside it ``HodeConfigError``); CPU tensors run eager
    arithmetic."""
    if z0.is_cuda:
        if perm is not None:
            perm = torch.as_tensor(perm, device=z0.device)
        z, logdet, log_diag = _SylvesterChain.apply(z0, r1, r2, b, q, perm, bool(want_log_diag))
        return (z, logdet, log_diag) if want_log_diag else (z, logdet)
    z, diags = z0, []
    for k in range(r1.shape[1]):
        z, ld = _sylvester_step_eager(z, r1[:, k], r2[:, k], b[:, k], None if q is None else q[:, k],
                                      None if perm is None else torch.as_tensor(perm)[k].long())
        diags.append(ld)
    log_diag = torch.stack(diags, dim=-2)
    logdet = log_diag.sum(dim=(-2, -1))
    return (z, logdet, log_diag) if want_log_diag else (z, logdet)


# ------------------------------------------------------------------------------------ the Sylvester-flow posterior
_LOG_SQRT_2PI = 0.9189385332046727
_PRIOR_RATE = 100.0  # model.ExponentialPrior.rate: the prior of the kernels' KL


class _SylvesterPosterior(torch.autograd.Function):
    """``hode.snf``'s two launches as one differentiable call.  Gradients for every raw head; none for the noise."""

    @staticmethod
    def forward(ctx, mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl, want_z):
        from hode.snf import snf_forward
        ctx.set_materialize_grads(False)  # an unused output arrives as None: its gradient input stays NULL
        z_out, kl, ws = snf_forward(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl, want_z)
        ctx.save_for_backward(mu, log_var, full_d, diag1, diag2, bias, v, noise, ws)
        ctx.s_kl = s_kl
        if z_out is None:
            z_out = kl.new_zeros(())  # placeholder output: no gradient flows into it
            ctx.mark_non_differentiable(z_out)
        return z_out, kl

    @staticmethod
    def backward(ctx, g_z, g_kl):
        if g_z is not None and g_z.dim() != 3:
            g_z = None
        if g_z is None and g_kl is None:
            return (None,) * 10  # nothing to propagate: no launch
        from hode.snf import snf_backward
        mu, log_var, full_d, diag1, diag2, bias, v, noise, ws = ctx.saved_tensors
        grads = snf_backward(mu, log_var, full_d, diag1, diag2, bias, v, noise, ws, ctx.s_kl, g_z, g_kl)
        return grads + (None, None, None)


def sylvester_flow_parameters(full_d, diag1, diag2, v=None):
    """The flow parameters of the Sylvester posterior from the encoder's raw heads, in eager arithmetic: full_d
    (B, K, D, D), diag1, diag2 (B, K, D), v (B, K, H, D) or None.  With U the strictly-upper mask

        r1 = U * full_d   + diag(tanh(diag1))
        r2 = U * full_d^T + diag(tanh(diag2))          (|r1_mm r2_mm| < 1: every flow is invertible)

    Returns ``(r1, r2, q, perm)`` for ``sylvester_chain``.  Triangular type (v None): q None and perm (K, D) the identity
    for even flows, the flip D-1 .. 0 for odd ones (an involution, so ``sylvester_chain``'s forward gather is the inverse
    permutation).  Householder type: perm None and q (B, K, D, D) = (I - 2 v0 v0^T) ... (I - 2 v_{H-1} v_{H-1}^T) with
    vh = v[:, :, h] / |v[:, :, h]|_2, orthogonal by construction."""
    B, K, D, _ = full_d.shape
    upper = torch.triu(torch.ones(D, D, dtype=full_d.dtype, device=full_d.device), diagonal=1)
    r1 = upper * full_d + torch.diag_embed(torch.tanh(diag1))
    r2 = upper * full_d.transpose(-1, -2) + torch.diag_embed(torch.tanh(diag2))
    if v is None:
        idx = torch.arange(D, device=full_d.device)
        perm = torch.stack([idx if k % 2 == 0 else idx.flip(0) for k in range(K)])
        return r1, r2, None, perm
    vh = v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)
    q = torch.eye(D, dtype=full_d.dtype, device=full_d.device).expand(B, K, D, D)
    for h in range(v.shape[2]):
        w = vh[:, :, h]                                                    # (B, K, D)
        q = q - 2.0 * torch.matmul(q, w.unsqueeze(-1)) * w.unsqueeze(-2)   # Q (I - 2 w w^T)
    return r1, r2, q, None


def sylvester_posterior_sample(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl=1, want_z=True):
    """Sylvester-flow draws and their Monte-Carlo KL against the Exponential(100) prior.

    mu, log_var (B, D); full_d (B, K, D, D); diag1, diag2, bias (B, K, D): the encoder's raw heads; v (B, K, H, D) for the
    Householder type or None for the triangular type; noise (S, B, D) standard-normal draws.

        z0    = noise * exp(0.5 log_var) + mu
        z_K   = the K flows of ``sylvester_chain`` with ``sylvester_flow_parameters(full_d, diag1, diag2, v)``
        z_out = exp(z_K - 5);   logdet = the chain's + sum_d (z_K - 5)
        kl_s  = sum_d log N(z0; mu, exp(0.5 log_var)) - logdet - sum_d (log 100 - 100 z_out)

    Returns ``z_out`` (S, B, D) -- ``None`` when ``want_z`` is False -- and ``kl`` (B,), the mean of kl_s over the draws
    ``s_kl .. S-1``.  HIP tensors run one fused kernel each way (libhode_snf.so; domain D 1 .. 32, K 1 .. 16, S 1 .. 256,
    H 0 .. 8, B >= 1, 0 <= s_kl < S; outside it ``HodeConfigError``); CPU tensors run the same arithmetic eagerly."""
    if mu.is_cuda:
        z_out, kl = _SylvesterPosterior.apply(mu, log_var, full_d, diag1, diag2, bias, v, noise, int(s_kl), bool(want_z))
        return (z_out if want_z else None), kl
    if not 0 <= s_kl < noise.shape[0]:
        raise ValueError("sylvester_posterior_sample: s_kl %r outside 0..%d" % (s_kl, noise.shape[0] - 1))
    r1, r2, q, perm = sylvester_flow_parameters(full_d, diag1, diag2, v)
    sigma = torch.exp(0.5 * log_var)
    z0 = noise * sigma + mu
    z, logdet = sylvester_chain(z0, r1, r2, bias, q, perm)
    z_out = torch.exp(z - 5.0)
    logdet = logdet + torch.sum(z - 5.0, dim=-1)
    log_q = (-((z0 - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - _LOG_SQRT_2PI).sum(dim=-1) - logdet
    log_p = (math.log(_PRIOR_RATE) - _PRIOR_RATE * z_out).sum(dim=-1)
    return (z_out if want_z else None), torch.mean((log_q - log_p)[s_kl:], dim=0)


def _single_step(zk, r1, r2, b, q, perm, sum_ldj):
    """One module call: (B, D) draws through one flow.  HIP tensors take the kernel with K = 1, S = 1."""
    B, M = r1.shape[0], r1.shape[-1]
    b = b.reshape(B, M)
    if zk.is_cuda:
        out = sylvester_chain(zk.unsqueeze(0), r1.unsqueeze(1), r2.unsqueeze(1), b.unsqueeze(1),
                              None if q is None else q.unsqueeze(1), None if perm is None else perm.reshape(1, -1),
                              want_log_diag=not sum_ldj)
        return out[0][0], (out[1][0] if sum_ldj else out[2][0, :, 0])
    z, log_diag = _sylvester_step_eager(zk, r1, r2, b, q, None if perm is None else perm.long())
    return z, (log_diag.sum(-1) if sum_ldj else log_diag)


class Sylvester(nn.Module):
    """Sylvester normalizing flow (van den Berg et al. 2018), all parameters amortized:
    z'^T = z^T + tanh(z^T Q R2^T + b^T) R1^T Q^T with zk (B, D), r1, r2 (B, M, M), q_ortho (B, D, M), b (B, 1, M).  The
    conditions on the diagonals of R1 and R2 are the caller's; ``triu_mask`` is a buffer the reference registers and never
    applies, kept for the state_dict."""

    def __init__(self, num_ortho_vecs):
        super().__init__()
        self.num_ortho_vecs = num_ortho_vecs
        self.h = nn.Tanh()
        self.register_buffer("triu_mask", torch.triu(torch.ones(num_ortho_vecs, num_ortho_vecs), diagonal=1).unsqueeze(0))
        self.register_buffer("diag_idx", torch.arange(0, num_ortho_vecs).long())

    def der_h(self, x):
        return self.der_tanh(x)

    def der_tanh(self, x):
        return 1 - self.h(x) ** 2

    def _forward(self, zk, r1, r2, q_ortho, b, sum_ldj=True):
        """Returns z' (B, D) and log|det J| (B,), or its M terms (B, M) with ``sum_ldj=False``."""
        return _single_step(zk, r1, r2, b, q_ortho, None, sum_ldj)

    def forward(self, zk, r1, r2, q_ortho, b, sum_ldj=True):
        return self._forward(zk, r1, r2, q_ortho, b, sum_ldj)


class TriangularSylvester(nn.Module):
    """Sylvester flow with Q a permutation (or the identity): zk (B, D), r1, r2 (B, D, D), b (B, 1, D), ``permute_z`` a
    (D,) index or None.  The output is gathered with ``permute_z`` again (see ``sylvester_chain``): a forward gather, not
    the inverse, as in the reference."""

    def __init__(self, z_size):
        super().__init__()
        self.z_size = z_size
        self.h = nn.Tanh()
        self.register_buffer("diag_idx", torch.arange(0, z_size).long())

    def der_h(self, x):
        return self.der_tanh(x)

    def der_tanh(self, x):
        return 1 - self.h(x) ** 2

    def _forward(self, zk, r1, r2, b, permute_z=None, sum_ldj=True):
        """Returns z' (B, D) and log|det J| (B,), or its D terms (B, D) with ``sum_ldj=False``."""
        return _single_step(zk, r1, r2, b, None, permute_z, sum_ldj)

    def forward(self, zk, r1, r2, q_ortho, b, sum_ldj=True):
        """The reference's argument mapping, reproduced: the FOURTH argument (named ``q_ortho``) reaches ``_forward`` as
        the bias and the FIFTH (named ``b``) as the permutation index.  Call it as
        ``forward(zk, r1, r2, bias, permute_z_or_None, sum_ldj)``."""
        return self._forward(zk, r1, r2, q_ortho, b, sum_ldj)
