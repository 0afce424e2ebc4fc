"""Bounds and comparison helpers the GPU test files share: each family's tolerance against its float64 reference lives
here once, so that the per-kernel files (test_hip_kernel_variants.py, test_hip_flow.py, test_hip_metric_cases.py) and
the binding file (test_hip_binding_contract.py) hold their kernels to the same numbers.  A plain helper module."""
import numpy as np
import torch

from oracle.evalmetrics import crps_sorted

# solver / decoder families (tests/test_hip_kernel_variants.py)
TRAJ_TOL, GRAD_TOL = 2e-5, 1e-4          # trajectory: TRAJ_TOL (1 + max|h|); gradients: rel-L2
NEURAL_REAL_GRAD_TOL = 2e-4
NEURAL_DOPRI5_TRAJ_TOL = 5e-6
LSTM_H_TOL, LSTM_C_TOL = 2e-5, 5e-5     # absolute
READOUT_TOL, READOUT_MLP_GRAD_TOL = 2e-5, 3e-5
# planar flow (tests/test_hip_flow.py): `close` bounds of outputs / gradients
FLOW_TOL, FLOW_GTOL = 2e-4, 2e-3
# metric kernels (tests/test_hip_metric_cases.py): per element, relative to the element's own scale
CRPS_TOL = 2e-5
MCKL_KL_TOL, MCKL_GRAD_TOL = 2e-5, 1e-5

LN_SQRT_2PI = 0.9189385332046727


def mckl_sum_error(S):
    """Worst-case relative error of the kernel's S-term fp32 running sum."""
    return S * 2.0 ** -24


def close(got, ref, rtol, what):
    """max |got - ref| <= rtol max|ref|."""
    ref = ref.to(torch.float64)
    got = got.to(torch.float64)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert np.isfinite(err) and err <= rtol * scale, "%s: max err %.3e, scale %.3e" % (what, err, scale)


def crps_oracle(h, truth, w, b):
    """fp64 CRPS field (Tn, B, obs) of h (Tn, M, B, Dv) and the per-element tolerance scale."""
    h64, y = h.double(), truth.double()
    if w is None:
        vals = h64[..., :truth.shape[-1]]                                   # (Tn, M, B, obs)
        extra = 0.0
    else:
        w64 = w.double()
        vals = torch.einsum("tmbd,od->tmbo", h64, w64) + (b.double() if b is not None else 0.0)
        extra = torch.einsum("tmbd,od->tmbo", h64.abs(), w64.abs()).mean(1) + (b.double().abs() if b is not None else 0.0)
    ens = vals.permute(0, 2, 3, 1)                                          # (Tn, B, obs, M)
    ref = torch.from_numpy(crps_sorted(y.numpy(), ens.numpy()))
    scale = (ens - y[..., None]).abs().mean(-1) + extra
    return ref, scale


def mckl_scales(mu, lv, eps, rate, clamp):
    """Per element: mean_s of the draw's |log q| + |log p| (plus the constants' magnitudes), of |d/dmu| and of |d/dlv|."""
    mu, lv, eps = mu.double(), lv.double(), eps.double()
    sd = torch.exp(0.5 * lv)
    z = eps * sd + mu
    pos = z > 0
    zc = torch.where(pos, z, torch.full_like(z, clamp))
    log_q = -0.5 * ((zc - mu) / sd) ** 2 - 0.5 * lv - LN_SQRT_2PI
    log_p = np.log(rate) - rate * zc
    kl = (log_q.abs() + log_p.abs()).mean(0) + 0.5 * lv.abs() + LN_SQRT_2PI + abs(np.log(rate))
    gmu = torch.where(pos, torch.full_like(z, rate), (clamp - mu) / sd ** 2).abs().mean(0)
    glv = 0.5 + torch.where(pos, 0.5 * rate * eps * sd, 0.5 * (clamp - mu) ** 2 / sd ** 2).abs().mean(0)
    return kl, gmu, glv, pos


def within(got, ref, scale, rel, what):
    """|got - ref| <= rel * scale, element by element."""
    err = (got.double() - ref).abs()
    ok = err <= rel * scale
    if not bool(ok.all()):
        i = int(torch.argmax(err / scale.clamp_min(1e-300)))
        raise AssertionError("%s: element %d got %r want %r (scale %r), %d bad" % (
            what, i, float(got[i]), float(ref[i]), float(scale[i]), int((~ok).sum())))
