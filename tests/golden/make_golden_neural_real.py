#!/usr/bin/env python
"""Generate ``tests/golden/g10_neural_real.npz`` (G10) from the REFERENCE's ``DecoderReal`` with ``ode_type`` "neural" /
"2nd" (``NeuralODEReal`` / ``NeuralODEReal2nd``, model.py:660-862), the neural ODE baselines of the real-data experiment.

Run in the build container only, like ``make_golden_seqdec.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    python tests/golden/make_golden_neural_real.py

Per case (kind, D, H, method, ode_step_div, t0, Ta, t_max) on CPU with B = 5, obs 24, statics 11: the seeded state_dict,
the inputs, ``x_hat`` and ``h``, the gradients of sum(x_hat * cot) for ``init`` and every parameter, the sequence of
times the reference's ``dose_at_time`` received with the ``int(t)`` it used, the eager rhs at one (t, y), and
``dose_at_time`` at a handful of probe times (fractional, negative, >= Ta).  Per kind: one
``VariationalInferenceReal(elbo=False)`` loss with an ``EncoderLSTMReal`` and its gradients.  Only arrays are written."""

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
OBS, ACT, STAT, B = 24, 1, 11, 5
# (kind, D, H, method, ode_step_div, t0, Ta, t_max)
CASES = [
    ("neural", 20, 43, "midpoint", 1, 24, 40, 40),
    ("neural", 13, 17, "rk4", 2, 8, 20, 20),
    ("2nd", 40, 43, "rk4", 1, 24, 36, 36),
    ("2nd", 6, 9, "euler", 1, 8, 20, 20),
    ("neural", 4, 9, "midpoint", 1, 0, 12, 12),     # grid starts at -1: int() truncates, floor would read row -1
    ("2nd", 8, 11, "rk4", 2, 4, 10, 16),            # Ta < t_max: stages at t >= Ta read zeros
]
PROBES = (-1.5, -1.0, -0.5, 0.0, 0.99, 3.7, 7.0)


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(module, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in module.state_dict().items()}


def logged(ode, log):
    orig = ode.dose_at_time

    def dose_at_time(t):
        log.append((float(t), int(t)))
        return orig(t)

    ode.dose_at_time = dose_at_time


def gen():
    out = {}
    gen = torch.Generator().manual_seed(1010)
    for ci, (kind, D, H, method, div, t0, TA, TMAX) in enumerate(CASES):
        pre = "c%d_" % ci
        torch.manual_seed(1000 + ci)
        dec = model.DecoderReal(OBS, D, ACT, STAT, H, TMAX, 1, t0=t0, method=method, ode_step_size=1.0 / div,
                                ode_type=kind, device=CPU)
        out[pre + "kind"] = np.array(kind)
        out[pre + "method"] = np.array(method)
        out[pre + "meta"] = np.array([D, H, div, t0, TA, TMAX, B, OBS, 1000 + ci], dtype=np.int64)
        out[pre + "model_name"] = np.array(dec.model_name)
        out[pre + "sd_keys"] = np.array(list(dec.state_dict().keys()))
        out.update(sd_arrays(dec, pre + "sd_"))
        out[pre + "t"] = npy(dec.t)
        init = (torch.randn(B, D, generator=gen) * 0.5).requires_grad_(True)
        a = (torch.rand(TA, B, ACT, generator=gen) < 0.3).float() * torch.rand(TA, B, ACT, generator=gen) * 2
        s = torch.rand(TA, B, STAT, generator=gen)
        log = []
        logged(dec.ode, log)
        x_hat, h = dec(init, a, s)
        cot = torch.randn(x_hat.shape, generator=gen)
        (x_hat * cot).sum().backward()
        out[pre + "init"], out[pre + "a"], out[pre + "s"], out[pre + "cot"] = npy(init), npy(a), npy(s), npy(cot)
        out[pre + "x_hat"], out[pre + "h"] = npy(x_hat), npy(h)
        out[pre + "g_init"] = npy(init.grad)
        for n, p in dec.named_parameters():
            out[pre + "g_" + n.replace(".", "__")] = npy(p.grad)
        out[pre + "dose_t"] = np.array([v[0] for v in log], dtype=np.float32)
        out[pre + "dose_row"] = np.array([v[1] for v in log], dtype=np.int64)
        # the eager rhs and dose_at_time at probe times (fractional, negative, past the action)
        with torch.no_grad():
            ty = torch.tensor(2.5)
            y = torch.randn(B, D, generator=gen)
            out[pre + "rhs_y"], out[pre + "rhs_t"] = npy(y), npy(ty)
            out[pre + "rhs_f"] = npy(dec.ode(ty, y))
            probes = list(PROBES) + [TA - 0.01, float(TA), TA + 3.5]
            out[pre + "probe_t"] = np.array(probes, dtype=np.float32)
            out[pre + "probe_dose"] = np.stack([npy(dec.ode.dose_at_time(torch.tensor(v, dtype=torch.float32))) for v in probes])
    out["n_cases"] = np.array(len(CASES))

    # VariationalInferenceReal(elbo=False) with EncoderLSTMReal, as run_real.py builds them
    T, t0 = 30, 24
    hidden = int((OBS + ACT + STAT) * 1.2)
    input_dim = OBS + ACT + STAT + 1
    for vi_i, (kind, D, method) in enumerate((("neural", 20, "midpoint"), ("2nd", 40, "rk4"))):
        pre = "vi%d_" % vi_i
        torch.manual_seed(1050 + vi_i)
        enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=CPU)
        dec = model.DecoderReal(OBS, D, ACT, STAT, hidden, T, 1, t0=t0, method=method, ode_step_size=1.0, ode_type=kind,
                                device=CPU)
        vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0, weight=False)
        data = {"measurements": torch.randn(T, B, OBS, generator=gen),
                "actions": (torch.rand(T, B, ACT, generator=gen) < 0.15).float() * torch.rand(T, B, ACT, generator=gen),
                "masks": (torch.rand(T, B, OBS, generator=gen) < 0.5).float(),
                "statics": torch.rand(1, B, STAT, generator=gen).expand(T, B, STAT).contiguous()}
        loss = vi.loss(data)
        loss.backward()
        out[pre + "kind"] = np.array(kind)
        out[pre + "method"] = np.array(method)
        out[pre + "meta"] = np.array([D, t0, B, T, OBS, 1050 + vi_i, hidden], dtype=np.int64)
        for k, v in data.items():
            out[pre + k] = npy(v)
        out[pre + "loss"] = npy(loss)
        out.update(sd_arrays(enc, pre + "enc_"))
        out.update(sd_arrays(dec, pre + "dec_"))
        for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
            for n, p in mod.named_parameters():
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                out[pre + tag + n.replace(".", "__")] = npy(g)
    np.savez_compressed(os.path.join(HERE, "g10_neural_real.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic reduction order
    gen()
    print("wrote", os.path.join(HERE, "g10_neural_real.npz"), os.path.getsize(os.path.join(HERE, "g10_neural_real.npz")), "bytes")
