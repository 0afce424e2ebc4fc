"""Float64 restatement of the chain of Sylvester flows (include/hode_sylvester.h), the yardstick of
tests/test_hip_sylvester.py.  Written from the formulas with einsum, not from the mirror in flow.py: dense mode
A = q r2^T, C = q r1; triangular mode the gather z[p] in and the SAME gather w[p] out (a forward gather, not the inverse
permutation); log|1 + (1 - h^2) r1_mm r2_mm| through torch.abs / torch.log, whose derivative is 1 / g for either sign.
Gradients come from autograd over this arithmetic, in float64 by default; `dtype=torch.float32` gives the float32 eager
error a kernel's bound may be derived from."""
import torch


def forward(z0, r1, r2, b, q=None, perm=None):
    """z0 (S, B, D); r1, r2 (B, K, M, M); b (B, K, M); q (B, K, D, M) or None; perm (K, D) integer index or None
    -> z_K (S, B, D), logdet (S, B), log_diag (S, B, K, M)."""
    z, diags = z0, []
    for k in range(r1.shape[1]):
        R1, R2 = r1[:, k], r2[:, k]
        if q is not None:
            A = torch.einsum("bdj,bmj->bdm", q[:, k], R2)
            C = torch.einsum("bdj,bjm->bdm", q[:, k], R1)
            h = torch.tanh(torch.einsum("sbd,bdm->sbm", z, A) + b[:, k])
            z = z + torch.einsum("sbm,bdm->sbd", h, C)
        else:
            p = torch.arange(z.shape[-1]) if perm is None else perm[k].long()
            h = torch.tanh(torch.einsum("sbj,bmj->sbm", z[..., p], R2) + b[:, k])
            w = torch.einsum("sbm,bjm->sbj", h, R1)
            z = z + w[..., p]
        dd = torch.diagonal(R1, dim1=-2, dim2=-1) * torch.diagonal(R2, dim1=-2, dim2=-1)
        diags.append(torch.log(torch.abs(1 + (1 - h * h) * dd)))
    log_diag = torch.stack(diags, dim=2)
    return z, log_diag.sum(dim=(2, 3)), log_diag


def forward_backward(z0, r1, r2, b, q=None, perm=None, grad_z=None, grad_logdet=None, grad_log_diag=None, dtype=torch.float64):
    """Forward in `dtype` and the gradients of sum(z_K grad_z) + sum(logdet grad_logdet) + sum(log_diag grad_log_diag) for
    (z0, r1, r2, b, q); q's entry is None in triangular mode; zeros where no cotangent reaches."""
    ins = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in (z0, r1, r2, b, q)]
    z, logdet, log_diag = forward(*ins, perm)
    obj = 0.0
    for out, g in ((z, grad_z), (logdet, grad_logdet), (log_diag, grad_log_diag)):
        if g is not None:
            obj = obj + (out * g.to(dtype)).sum()
    live = [t for t in ins if t is not None]
    grads = torch.autograd.grad(obj, live, allow_unused=True) if torch.is_tensor(obj) else (None,) * len(live)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, live)]
    if q is None:
        grads.append(None)
    return z.detach(), logdet.detach(), log_diag.detach(), grads
