"""Float64 restatement of the planar-flow posterior and its Monte-Carlo KL (include/hode_flow.h), the yardstick of
tests/test_hip_flow.py.  Written from the formulas, not from the mirror: torch's softplus threshold (x > 20 -> x), the
u_hat reparameterisation, log|1 + psi . u_hat| (torch.abs / torch.log, whose derivative is 1 / g for either sign), the
exp(z - 5) output layer and the Exponential(100) prior.  Gradients come from float64 autograd over this arithmetic.

Also the GPU test table (CASES) and which compiled kernels each case reaches (kernels()), read by the no-GPU coverage
guard in tests/test_flow_host.py."""
import math

import torch

LOG_RATE, RATE = math.log(100.0), 100.0
TILES = (4, 8, 16, 32)


def softplus_t20(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def forward(mu, log_var, u, w, b, noise, s_kl):
    """mu, log_var (B, D); u, w (B, K, D); b (B, K); noise (S, B, D) -> z_out (S, B, D), kl (B,), log_det (S, B), z0."""
    sigma = torch.exp(0.5 * log_var)
    z0 = noise * sigma + mu
    uw = (w * u).sum(-1, keepdim=True)
    u_hat = u + (-1.0 + softplus_t20(uw) - uw) * w / (w * w).sum(-1, keepdim=True)
    z = z0
    log_det = torch.zeros(noise.shape[:2], dtype=noise.dtype)
    for k in range(u.shape[1]):
        h = torch.tanh((w[:, k] * z).sum(-1) + b[:, k])                  # (S, B)
        z = z + u_hat[:, k] * h.unsqueeze(-1)
        g = 1 + (1 - h * h) * (w[:, k] * u_hat[:, k]).sum(-1)
        log_det = log_det + torch.log(torch.abs(g))
    y = z - 5.0
    z_out = torch.exp(y)
    log_det = log_det + y.sum(-1)
    log_q = (-((z0 - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)).sum(-1) - log_det
    log_p = (LOG_RATE - RATE * z_out).sum(-1)
    kl = (log_q - log_p)[s_kl:].mean(0)
    return z_out, kl, log_det, z0


def forward_backward(mu, log_var, u, w, b, noise, s_kl, grad_z=None, grad_kl=None):
    """float64 forward and the gradients of sum(z_out * grad_z) + sum(kl * grad_kl) for (mu, log_var, u, w, b)."""
    ins = [t.detach().to(torch.float64).requires_grad_(True) for t in (mu, log_var, u, w, b)]
    z_out, kl, _, _ = forward(*ins, noise.to(torch.float64), s_kl)
    obj = 0.0
    if grad_z is not None:
        obj = obj + (z_out * grad_z.to(torch.float64)).sum()
    if grad_kl is not None:
        obj = obj + (kl * grad_kl.to(torch.float64)).sum()
    grads = torch.autograd.grad(obj, ins, allow_unused=True) if torch.is_tensor(obj) else (None,) * 5
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, ins)]
    return z_out.detach(), kl.detach(), grads


def tile(D):
    return next(t for t in TILES if D <= t)


# ------------------------------------------------------------------ GPU test table (tests/test_hip_flow.py)
# (D, K, S, B, s_kl): the D x K x S x B grid thinned so that every tile (forward and backward kernel) and every
# lanes-per-patient regime (B = 1 / 7 / 10 000 / 100 003, S = 1 / 50 / 64 / 65 / 256) is reached.
def _grid():
    cases = []
    Ds, Ks, Ss, Bs = (1, 3, 6, 12, 20, 32), (1, 4, 16), (1, 50, 64, 65, 256), (1, 7, 10000)
    for i, D in enumerate(Ds):
        for j, K in enumerate(Ks):
            S = Ss[(i + j) % len(Ss)]
            B = Bs[(i + 2 * j) % len(Bs)]
            if B == 10000 and S * D > 64 * 12:
                S = 50
            cases.append((D, K, S, B, 0 if S == 1 else 1))
    cases.append((12, 4, 50, 100003, 1))
    cases.append((6, 4, 51, 10, 1))
    return cases


CASES = _grid()


def kernels(case):
    t = tile(case[0])
    return {"hode_flow::flow_fwd_kernel<%d>" % t, "hode_flow::flow_bwd_kernel<%d>" % t}
