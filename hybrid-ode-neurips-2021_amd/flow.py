"""Planar normalizing flow (reference ``flow.py:8-59``), eager arithmetic, so that ``import flow`` resolves where the
reference's ``model.py`` expects it.  The training and evaluation hot path runs the whole flow stack with its
Monte-Carlo KL in ``hode.flow`` (libhode_flow.so); this module is the per-draw call surface and the CPU path."""

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
