"""Float64 restatement of the Sylvester-flow posterior (include/hode_snf.h), the yardstick of tests/test_hip_snf.py and
tests/test_snf_host.py.  Written from the formulas with einsum and explicit index arithmetic, not from the product code
in flow.py: r1 and r2 are filled entry by entry from full_d, Q is a product of explicit reflection matrices, the odd
flows reverse the coordinates by slicing.  Gradients come from autograd over this arithmetic, in float64 by default;
`dtype=torch.float32` gives the float32 eager error a kernel's bound may be derived from."""
import math

import torch

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
RATE = 100.0


def parameters(full_d, diag1, diag2, v=None):
    """r1, r2 (B, K, D, D) and Q (B, K, D, D) or None."""
    B, K, D, _ = full_d.shape
    r1 = torch.zeros_like(full_d)
    r2 = torch.zeros_like(full_d)
    for i in range(D):
        r1[..., i, i] = torch.tanh(diag1[..., i])
        r2[..., i, i] = torch.tanh(diag2[..., i])
        for j in range(i + 1, D):
            r1[..., i, j] = full_d[..., i, j]
            r2[..., i, j] = full_d[..., j, i]
    if v is None:
        return r1, r2, None
    eye = torch.eye(D, dtype=full_d.dtype)
    q = eye.expand(B, K, D, D)
    for h in range(v.shape[2]):
        w = v[:, :, h]
        w = w / torch.sqrt(torch.einsum("bkd,bkd->bk", w, w)).unsqueeze(-1)
        q = torch.einsum("bkij,bkjl->bkil", q, eye - 2.0 * torch.einsum("bki,bkj->bkij", w, w))
    return r1, r2, q


def chain(z0, r1, r2, bias, q):
    """z_K (S, B, D), the chain's logdet (S, B), and the intermediate states [z_0 .. z_K]."""
    z, logdet, states = z0, 0.0, [z0]
    for k in range(r1.shape[1]):
        R1, R2 = r1[:, k], r2[:, k]
        if q is not None:
            zq = torch.einsum("sbd,bdj->sbj", z, q[:, k])
            h = torch.tanh(torch.einsum("sbj,bmj->sbm", zq, R2) + bias[:, k])
            z = z + torch.einsum("sbj,bdj->sbd", torch.einsum("sbm,bjm->sbj", h, R1), q[:, k])
        else:
            zp = z.flip(-1) if k % 2 else z
            h = torch.tanh(torch.einsum("sbj,bmj->sbm", zp, R2) + bias[:, k])
            w = torch.einsum("sbm,bjm->sbj", h, R1)
            z = z + (w.flip(-1) if k % 2 else w)
        dd = torch.diagonal(R1, dim1=-2, dim2=-1) * torch.diagonal(R2, dim1=-2, dim2=-1)
        logdet = logdet + torch.log(torch.abs(1 + (1 - h * h) * dd)).sum(-1)
        states.append(z)
    return z, logdet, states


def forward(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl):
    """-> z_out (S, B, D), kl (B,), logdet (S, B) (the chain's plus the output layer's), z0 (S, B, D)."""
    r1, r2, q = parameters(full_d, diag1, diag2, v)
    return posterior(mu, log_var, r1, r2, q, bias, noise, s_kl)


def posterior(mu, log_var, r1, r2, q, bias, noise, s_kl):
    """forward() from given flow parameters (r1, r2, q as parameters() returns them)."""
    sigma = torch.exp(0.5 * log_var)
    z0 = noise * sigma + mu
    z, logdet, _ = chain(z0, r1, r2, bias, q)
    z_out = torch.exp(z - 5.0)
    logdet = logdet + (z - 5.0).sum(-1)
    log_base = (-0.5 * ((z0 - mu) / sigma) ** 2 - torch.log(sigma) - LOG_SQRT_2PI).sum(-1)
    log_p = (math.log(RATE) - RATE * z_out).sum(-1)
    kl_s = log_base - logdet - log_p
    return z_out, kl_s[s_kl:].mean(0), logdet, z0


def forward_backward(mu, log_var, full_d, diag1, diag2, bias, v, noise, s_kl, grad_z=None, grad_kl=None, dtype=torch.float64):
    """Forward in `dtype` and the gradients of sum(z_out grad_z) + sum(kl grad_kl) for (mu, log_var, full_d, diag1, diag2,
    bias, v); v's entry is None for the triangular type; zeros where no cotangent reaches."""
    ins = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in (mu, log_var, full_d, diag1, diag2, bias, v)]
    z_out, kl, _, _ = forward(*ins, noise.to(dtype), s_kl)
    obj = 0.0
    for out, g in ((z_out, grad_z), (kl, grad_kl)):
        if g is not None:
            obj = obj + (out * g.to(dtype)).sum()
    live = [t for t in ins if t is not None]
    grads = torch.autograd.grad(obj, live, allow_unused=True) if torch.is_tensor(obj) else (None,) * len(live)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, live)]
    if v is None:
        grads.append(None)
    return z_out.detach(), kl.detach(), grads
