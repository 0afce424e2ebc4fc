#!/usr/bin/env python
"""Generate ``tests/golden/g9_seqdec.npz`` (G9) from the REFERENCE's ``DecoderRealBenchmark`` / ``GRUODECell``
(model.py:865-966), the ``tlstm`` and ``gruode`` baselines of the real-data experiment.

Run in the build container only, like ``make_golden.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty; neither is used by these classes):

    python tests/golden/make_golden_seqdec.py

Per case (kind, D, t0) on CPU with B = 7, Ta = t_max = 30, obs 24, statics 11: the seeded state_dict, the inputs,
``x_hat`` and ``h``, the gradients of sum(x_hat * cot) for ``init`` and every parameter, and one single-step
``GRUODECell`` call.  Per kind: one ``VariationalInferenceReal(elbo=False)`` loss with an ``EncoderLSTMReal`` (run_real.py's
setting) and its gradients.  Only arrays are written."""

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
KINDS = ("tlstm", "gruode")
OBS, ACT, STAT, TA, B = 24, 1, 11, 30, 7
HIDDEN = int((OBS + ACT + STAT) * 1.2)
CASES = [(kind, D, t0) for kind in KINDS for D, t0 in ((4, 8), (20, 8), (13, 8), (20, 29))]


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(module, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in module.state_dict().items()}


def gen():
    out = {}
    gen = torch.Generator().manual_seed(909)
    for ci, (kind, D, t0) in enumerate(CASES):
        pre = "c%d_" % ci
        torch.manual_seed(900 + ci)
        dec = model.DecoderRealBenchmark(OBS, D, ACT, STAT, HIDDEN, TA, 1, ode_type=kind, t0=t0, device=CPU)
        out[pre + "kind"] = np.array(kind)
        out[pre + "meta"] = np.array([D, t0, B, TA, OBS, 900 + ci], dtype=np.int64)
        out[pre + "model_name"] = np.array(dec.model_name)
        out[pre + "sd_keys"] = np.array(list(dec.state_dict().keys()))
        out.update(sd_arrays(dec, pre + "sd_"))
        out[pre + "t"] = npy(dec.t)
        init = (torch.randn(B, D, generator=gen) * 0.5).requires_grad_(True)
        a = (torch.rand(TA, B, ACT, generator=gen) < 0.3).float() * torch.rand(TA, B, ACT, generator=gen) * 2
        s = torch.rand(TA, B, STAT, generator=gen)
        x_hat, h = dec(init, a, s)
        cot = torch.randn(x_hat.shape, generator=gen)
        (x_hat * cot).sum().backward()
        out[pre + "init"], out[pre + "a"], out[pre + "cot"] = npy(init), npy(a), npy(cot)
        out[pre + "x_hat"], out[pre + "h"] = npy(x_hat), npy(h)
        out[pre + "g_init"] = npy(init.grad)
        for n, p in dec.named_parameters():
            out[pre + "g_" + n.replace(".", "__")] = npy(p.grad)
        if kind == "gruode":  # one bare cell call: GRUODECell.forward(a, (h, c))
            ca = torch.randn(1, B, 2, generator=gen)
            ch = torch.randn(1, B, D, generator=gen)
            dh, (hh, c0) = dec.rnn(ca, (ch, ch))
            out[pre + "cell_a"], out[pre + "cell_h"], out[pre + "cell_dh"] = npy(ca), npy(ch), npy(dh)
    out["n_cases"] = np.array(len(CASES))

    # VariationalInferenceReal(elbo=False) with EncoderLSTMReal, as run_real.py:38-72 builds them (D = 20, t0 = 24)
    D, t0, T = 20, 24, TA
    input_dim = OBS + ACT + STAT + 1
    for vi_i, kind in enumerate(KINDS):
        pre = "vi%d_" % vi_i
        torch.manual_seed(950 + vi_i)
        enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=CPU)
        dec = model.DecoderRealBenchmark(OBS, D, ACT, STAT, HIDDEN, T, 1, ode_type=kind, t0=t0, device=CPU)
        vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0, weight=False)
        data = {"measurements": torch.randn(T, B, OBS, generator=gen),
                "actions": (torch.rand(T, B, ACT, generator=gen) < 0.15).float() * torch.rand(T, B, ACT, generator=gen),
                "masks": (torch.rand(T, B, OBS, generator=gen) < 0.5).float(),
                "statics": torch.rand(1, B, STAT, generator=gen).expand(T, B, STAT).contiguous()}
        loss = vi.loss(data)
        loss.backward()
        out[pre + "kind"] = np.array(kind)
        out[pre + "meta"] = np.array([D, t0, B, T, OBS, 950 + vi_i], dtype=np.int64)
        for k, v in data.items():
            out[pre + k] = npy(v)
        out[pre + "loss"] = npy(loss)
        out.update(sd_arrays(enc, pre + "enc_"))
        out.update(sd_arrays(dec, pre + "dec_"))
        for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
            for n, p in mod.named_parameters():
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                out[pre + tag + n.replace(".", "__")] = npy(g)
    np.savez_compressed(os.path.join(HERE, "g9_seqdec.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic reduction order
    gen()
    print("wrote", os.path.join(HERE, "g9_seqdec.npz"), os.path.getsize(os.path.join(HERE, "g9_seqdec.npz")), "bytes")
