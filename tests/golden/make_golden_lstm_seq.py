#!/usr/bin/env python
"""Generate ``tests/golden/g17_lstm_seq.npz`` (G17) from the REFERENCE's ``LSTMBaseline`` (model.py:322-380) and
``EncoderLSTMReal(output_all=True)`` (model.py:180-242): the two classes whose LSTM hands back every step.

Run in the build container only, like ``make_golden.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    python tests/golden/make_golden_lstm_seq.py

Size: 390 KB, nearly all of it weights and their gradients -- the shapes are fixed (H 44, inputs 36 / 37, as the real-data
runs use them): one LSTMBaseline state (70 KB) and its gradient, one encoder state (82 KB, shared by the two directions) and
a gradient set per direction.  Batch, outputs and cotangents together are 25 KB; float32 noise does not compress.

Keys (arrays only, ``allow_pickle=False``):
    meta                     T, B, obs, action, statics, H, encoder output_dim
    measurements, actions, masks, statics        the seeded batch (T 7, B 5, obs 24, action 1, statics 11)
    base_sd_<key>            ``LSTMBaseline(36, 44, 24)``'s seeded state_dict ("." written "__")
    base_forward, base_loss  ``forward(x, cat(a, s), mask)`` (T, B, obs) and ``loss(data)``
    base_g_<key>             the gradient of ``loss`` for every parameter
    enc_sd_<key>             ``EncoderLSTMReal(37, 44, 20, output_all=True)``'s seeded state_dict, shared by both directions
    enc_cot_mu, enc_cot_lv   the seeded cotangents of the linear functional sum(mu * cot_mu) + sum(log_var * cot_lv)
    enc_r<0|1>_mu, enc_r<0|1>_log_var, enc_r<0|1>_g_<key>   outputs (T, B, 20) and parameter gradients, reverse False / True"""

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
OUT = os.path.join(HERE, "g17_lstm_seq.npz")
T, B, OBS, ACT, STAT, H, DZ = 7, 5, 24, 1, 11, 44, 20


def npy(x):
    return x.detach().cpu().numpy()


def key(k):
    return k.replace(".", "__")


def gen():
    out = {"meta": np.array([T, B, OBS, ACT, STAT, H, DZ], dtype=np.int64)}
    g = torch.Generator().manual_seed(1717)
    data = {"measurements": torch.randn(T, B, OBS, generator=g),
            "actions": (torch.rand(T, B, ACT, generator=g) < 0.3).float(),
            "masks": (torch.rand(T, B, OBS, generator=g) < 0.7).float(),
            "statics": torch.randn(1, B, STAT, generator=g).expand(T, B, STAT).contiguous()}
    for k, v in data.items():
        out[k] = npy(v)

    torch.manual_seed(1701)
    base = model.LSTMBaseline(OBS + ACT + STAT, H, OBS, device=CPU)
    for k, v in base.state_dict().items():
        out["base_sd_" + key(k)] = npy(v).copy()
    a_in = torch.cat([data["actions"], data["statics"]], dim=-1)
    out["base_forward"] = npy(base(data["measurements"], a_in, data["masks"]))
    loss = base.loss(data)
    loss.backward()
    out["base_loss"] = npy(loss)
    for k, p in base.named_parameters():
        out["base_g_" + key(k)] = npy(p.grad).copy()

    torch.manual_seed(1702)
    sd = None
    out["enc_cot_mu"] = npy(torch.randn(T, B, DZ, generator=g))
    out["enc_cot_lv"] = npy(torch.randn(T, B, DZ, generator=g))
    for r, reverse in enumerate((False, True)):
        enc = model.EncoderLSTMReal(OBS + ACT + STAT + 1, H, DZ, output_all=True, reverse=reverse, device=CPU)
        if sd is None:
            sd = {k: v.clone() for k, v in enc.state_dict().items()}
            for k, v in sd.items():
                out["enc_sd_" + key(k)] = npy(v).copy()
        enc.load_state_dict(sd)
        mu, lv = enc(data["measurements"], a_in, data["masks"])
        ((mu * torch.from_numpy(out["enc_cot_mu"])).sum() + (lv * torch.from_numpy(out["enc_cot_lv"])).sum()).backward()
        out["enc_r%d_mu" % r], out["enc_r%d_log_var" % r] = npy(mu), npy(lv)
        for k, p in enc.named_parameters():
            out["enc_r%d_g_%s" % (r, key(k))] = npy(p.grad).copy()
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    gen()
