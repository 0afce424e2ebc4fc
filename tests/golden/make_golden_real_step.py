#!/usr/bin/env python
"""Generate ``tests/golden/g18_real_step.npz`` (G18) from the REFERENCE's ``DecoderReal(ode_type="hybrid")`` called with a
3-D ``init`` (model.py:833-862): the one-step-ahead mode, one solver call per interval from a start state of its own.

Run in the build container only, like ``make_golden_lstm_seq.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    python tests/golden/make_golden_real_step.py

Cases: T = t_max 8, B 5, obs 6, statics 3, hidden 5; D in {7, 20} x t0 in {0, 1} x (method, ode_step_div) in
{(midpoint, 1), (rk4, 2), (euler, 1)}.  ``init`` has T rows: the reference reads the first T - 1.

Keys (arrays only, ``allow_pickle=False``):
    meta                         T, B, obs, action, statics, hidden
    actions, statics             the seeded batch (T, B, 1), (T, B, 3), shared by all cases
    cases                        one row per case: D, t0, method (0 euler, 1 midpoint, 2 rk4), ode_step_div
    c<k>_sd_<key>                the seeded state_dict of case k ("." written "__")
    c<k>_init, c<k>_c1, c<k>_c2  the start states (T, B, D) and the cotangents of x_hat and h
    c<k>_x_hat, c<k>_h           the outputs (T - 1, B, obs) and (T, B, D)
    c<k>_g_init, c<k>_g_<key>    the gradients of sum(x_hat * c1) + sum(h * c2) for ``init`` and every parameter"""

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from oracle.solvers import odeint as oracle_odeint  # noqa: E402

_stub = types.ModuleType("torchdiffeq")
_stub.odeint = oracle_odeint
sys.modules["torchdiffeq"] = _stub
sys.modules["properscoring"] = types.ModuleType("properscoring")
sys.path.insert(0, REF)

import model  # noqa: E402  (reference)

CPU = torch.device("cpu")
OUT = os.path.join(HERE, "g18_real_step.npz")
T, B, OBS, ACT, STAT, HID = 8, 5, 6, 1, 3, 5
METHODS = {"euler": 0, "midpoint": 1, "rk4": 2}
CASES = [(D, t0, m, div) for D in (7, 20) for t0 in (0, 1) for m, div in (("midpoint", 1), ("rk4", 2), ("euler", 1))]


def npy(x):
    return x.detach().cpu().numpy()


def key(k):
    return k.replace(".", "__")


def gen():
    out = {"meta": np.array([T, B, OBS, ACT, STAT, HID], dtype=np.int64),
           "cases": np.array([[D, t0, METHODS[m], div] for D, t0, m, div in CASES], dtype=np.int64)}
    g = torch.Generator().manual_seed(1818)
    a = (torch.rand(T, B, ACT, generator=g) < 0.4).float() * torch.rand(T, B, ACT, generator=g)
    s = torch.randn(1, B, STAT, generator=g).expand(T, B, STAT).contiguous()
    out["actions"], out["statics"] = npy(a), npy(s)
    for k, (D, t0, method, div) in enumerate(CASES):
        torch.manual_seed(1800 + k)
        dec = model.DecoderReal(OBS, D, ACT, STAT, HID, T, 1, t0=t0, method=method, ode_step_size=1.0 / div, ode_type="hybrid",
                                device=CPU)
        for n, v in dec.state_dict().items():
            out["c%d_sd_%s" % (k, key(n))] = npy(v).copy()
        init = (torch.randn(T, B, D, generator=g) * 0.3).requires_grad_(True)
        c1, c2 = torch.randn(T - 1, B, OBS, generator=g), torch.randn(T, B, D, generator=g)
        x_hat, h = dec(init, a, s)
        assert x_hat.shape == c1.shape and h.shape == c2.shape and bool(torch.isfinite(h).all())
        ((x_hat * c1).sum() + (h * c2).sum()).backward()
        for n, v in (("init", init), ("c1", c1), ("c2", c2), ("x_hat", x_hat), ("h", h), ("g_init", init.grad)):
            out["c%d_%s" % (k, n)] = npy(v).copy()
        for n, p in dec.named_parameters():
            out["c%d_g_%s" % (k, key(n))] = npy(p.grad).copy()
        print("case %d D %d t0 %d %s div %d: max|h| %.3f" % (k, D, t0, method, div, float(h.abs().max())))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    gen()
