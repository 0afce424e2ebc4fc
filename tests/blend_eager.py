"""Float64 eager forms of the two blend kernels (libhode_blend.so) with hode.blend's call contracts: the yardsticks of
tests/test_hip_blend.py and the stand-ins that tests/test_blend_host.py puts behind training_utils' swap points.  A plain
helper module."""
import numpy as np
import torch


def gram(x_e, x_m, truth):
    """The five float64 Gram sums per step, each (T',): a11, a22, a12, b1, b2."""
    e, m, y = (v.detach().cpu().double().reshape(v.shape[0], -1) for v in (x_e, x_m, truth))
    return (e * e).sum(1), (m * m).sum(1), (e * m).sum(1), (e * y).sum(1), (m * y).sum(1)


def solve2(a11, a22, a12, b1, b2):
    """The closed form of include/hode_blend.h for one step, in Python floats (float64, no contraction)."""
    g1 = b1 * b1 / a11 if a11 > 0.0 and b1 > 0.0 else 0.0
    g2 = b2 * b2 / a22 if a22 > 0.0 and b2 > 0.0 else 0.0
    gmax = g1 if g1 >= g2 else g2
    det = a11 * a22 - a12 * a12
    if det > 0.0:
        u1, u2 = (a22 * b1 - a12 * b2) / det, (a11 * b2 - a12 * b1) / det
        if u1 > 0.0 and u2 > 0.0:
            dec = 2.0 * (u1 * b1 + u2 * b2) - (u1 * u1 * a11 + 2.0 * (u1 * u2 * a12) + u2 * u2 * a22)
            if dec >= gmax - 1e-9 * gmax:     # false for a candidate that is not finite
                return u1, u2
    if g1 >= g2:
        return (b1 / a11 if g1 > 0.0 else 0.0), 0.0
    return 0.0, b2 / a22


def nnls2(x_e, x_m, truth):
    """hode.blend.nnls2_weights in float64: (w_e, w_m), each (T',) float64 on the inputs' device."""
    sums = [s.tolist() for s in gram(x_e, x_m, truth)]
    w = np.array([solve2(*step) for step in zip(*sums)], dtype=np.float64).reshape(-1, 2)
    return torch.from_numpy(w[:, 0].copy()).to(x_e.device), torch.from_numpy(w[:, 1].copy()).to(x_e.device)


def objective(w_e, w_m, x_e, x_m, truth):
    """sum_r (w_e x_e + w_m x_m - truth)^2 per step in float64, (T',)."""
    e, m, y = (v.detach().cpu().double().reshape(v.shape[0], -1) for v in (x_e, x_m, truth))
    w_e, w_m = (torch.as_tensor(w).detach().cpu().double().reshape(-1, 1) for w in (w_e, w_m))
    return ((w_e * e + w_m * m - y) ** 2).sum(1)


def active_set(w_e, w_m):
    """Per step 0 (neither), 1 (expert only), 2 (ml only) or 3 (both)."""
    return (torch.as_tensor(w_e).cpu() > 0).long() + 2 * (torch.as_tensor(w_m).cpu() > 0).long()


def _table(w, Tn, obs):
    if w is None:
        return torch.ones(Tn, 1, obs, dtype=torch.float64)
    if not torch.is_tensor(w):
        return torch.full((Tn, 1, obs), float(w), dtype=torch.float64)
    w = w.detach().cpu().double()
    if w.dim() == 0:
        return w.expand(Tn, 1, obs)
    if tuple(w.shape) == (Tn,):
        return w[:, None, None].expand(Tn, 1, obs)
    if tuple(w.shape) == (Tn, obs):
        return w[:, None, :]
    assert tuple(w.shape) == (Tn, 1, obs), tuple(w.shape)
    return w


def horizon_terms(x_e, truth, mask, x_m=None, weight_e=None, weight_m=None):
    """Float64 per-element squared error and tolerance scale (|truth| + |w_e x_e| + |w_m x_m|)^2, both times the mask."""
    Tn, _, obs = x_e.shape
    y, mk = truth.detach().cpu().double(), mask.detach().cpu().double()
    pe = _table(weight_e, Tn, obs) * x_e.detach().cpu().double()
    pm = _table(weight_m, Tn, obs) * x_m.detach().cpu().double() if x_m is not None else torch.zeros_like(pe)
    return (y - (pe + pm)) ** 2 * mk, (y.abs() + pe.abs() + pm.abs()) ** 2 * mk, mk


def _prefixes(field, horizons):
    Tn = field.shape[0]
    return torch.stack([field[:min(int(n), Tn)].sum(dim=(0, 2)) for n in horizons])


def horizon_sse(x_e, truth, mask, horizons, x_m=None, weight_e=None, weight_m=None):
    """hode.blend.horizon_sse in float64: (sse, cnt), each (H, B) float64 on the inputs' device."""
    sq, _, mk = horizon_terms(x_e, truth, mask, x_m, weight_e, weight_m)
    return _prefixes(sq, horizons).to(x_e.device), _prefixes(mk, horizons).to(x_e.device)


def horizon_scale(x_e, truth, mask, horizons, x_m=None, weight_e=None, weight_m=None):
    """S (H, B) of the error bound |sse - sse64| <= 8 * 2^-24 * S."""
    _, scale, _ = horizon_terms(x_e, truth, mask, x_m, weight_e, weight_m)
    return _prefixes(scale, horizons)


def script_rmse(x_hat, x, mask, t0, horizons):
    """The scripts' formula, literally (run_real_ensemble.py:146-151), in the tensors' own dtype: per horizon the
    per-patient vector (NaN patients dropped) and sqrt of its mean."""
    out = []
    for n in horizons:
        t1 = t0 + n
        a = torch.sum((x[t0:t1] - x_hat[:(t1 - t0)]) ** 2 * mask[t0:t1], dim=(0, 2)) / torch.sum(mask[t0:t1], dim=(0, 2))
        a = a[~torch.isnan(a)]
        out.append((a, torch.sqrt(torch.mean(a)).item()))
    return out
