#!/usr/bin/env python
"""Generate ``tests/golden/g15_neural_odd.npz`` (G15) from the REFERENCE's ``NeuralODE`` at latent size 15, the size
``experiments/Fig9.sh`` reaches with ``run_simulation --method=neural --encoder_output_dim=15``.

Run in the build container only, like ``make_golden_neural_real.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    python tests/golden/make_golden_neural_odd.py

``c0_``: ``model.NeuralODE(15, ...)`` -- the seeded state_dict, an action with one dose per patient, states ``y``, and per
time in ``t`` (three of them dose times, one of those also the midpoint stage time of a grid step) the rhs value with the autograd VJP
of sum(f * cot) for ``y`` and every parameter.  Same keys as G2, plus the parameter gradients.
``vi_``: one ``VariationalInference(EncoderLSTM(normalize=False), RocheExpertDecoder(roche=False, latent 15),
prior_log_pdf=None)`` loss with the default solver (dopri5), as ``run_simulation`` builds it for ``--method=neural``, with
every parameter gradient.  Same keys as a G5 case.  Only arrays are written."""

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
D = 15
OUT = os.path.join(HERE, "g15_neural_odd.npz")


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(module, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in module.state_dict().items()}


def one_dose_actions(T, B, gen, idx, dose_max=10.0):
    a = torch.zeros(T, B, 1)
    a[idx, torch.arange(B), 0] = torch.rand(B, generator=gen) * dose_max
    return a


def gen():
    out = {}
    g = torch.Generator().manual_seed(1515)
    step, T, B = 0.125, 16, 5
    torch.manual_seed(1500)
    ode = model.NeuralODE(D, 1, (T - 1) * step, step, device=CPU)
    a = one_dose_actions(T, B, g, torch.tensor([2, 2, 5, 0, 14]))
    ode.set_action(a)
    y = torch.randn(B, D, generator=g)
    # 0, 2 step and 5 step are dose times; 5 step = 0.625 is also the midpoint stage time of the grid step [0.5, 0.75]:
    # a stage time equal to a dose time.  2 step + 1e-3 is off every dose.
    ts = [0.0, 2 * step, 2 * step + 1e-3, 5 * step, 1.0]
    cot = torch.randn(B, D, generator=g)
    pre = "c0_"
    out[pre + "meta"] = np.array([D, T, B], dtype=np.int64)
    out[pre + "step"] = np.float64(step)
    out[pre + "action"], out[pre + "y"], out[pre + "cot"] = npy(a), npy(y), npy(cot)
    out[pre + "t"] = np.array(ts, dtype=np.float32)
    out.update(sd_arrays(ode, pre + "sd_"))
    fs, gys, gps = [], [], {n: [] for n, _ in ode.named_parameters()}
    for t in ts:
        yy = y.clone().requires_grad_(True)
        ode.zero_grad()
        f = ode(torch.tensor(t, dtype=torch.float32), yy)
        (f * cot).sum().backward()
        fs.append(npy(f))
        gys.append(npy(yy.grad))
        for n, p in ode.named_parameters():
            gps[n].append(npy(p.grad if p.grad is not None else torch.zeros_like(p)).copy())
    out[pre + "f"], out[pre + "gy"] = np.stack(fs), np.stack(gys)
    for n, v in gps.items():
        out[pre + "g_" + n.replace(".", "__")] = np.stack(v)
    out["n_cases"] = np.array(1)

    # VariationalInference.loss as run_simulation --method=neural --encoder_output_dim=15 builds it
    obs, T, B = 10, 12, 6
    t_max = (T - 1) * step
    torch.manual_seed(1550)
    enc = model.EncoderLSTM(obs + 1, obs * 2, D, device=CPU, normalize=False)
    dec = model.RocheExpertDecoder(obs, D, 1, t_max, step, roche=False, method="dopri5", device=CPU)
    vi = model.VariationalInference(enc, dec, prior_log_pdf=None, elbo=True)
    x = torch.randn(T, B, obs, generator=g)
    a = one_dose_actions(T, B, g, torch.randint(0, T, (B,), generator=g))
    m = (torch.rand(T, B, obs, generator=g) < 0.5).float()
    torch.manual_seed(1590)  # seeds the reparameterisation draw
    loss = vi.loss({"measurements": x, "actions": a, "masks": m})
    for p in vi.parameters():
        p.grad = None
    loss.backward()
    pre = "vi_"
    out[pre + "method"], out[pre + "mode"] = np.array("dopri5"), np.array("kl_normal")
    out[pre + "meta"] = np.array([obs, D, T, B, 1590], dtype=np.int64)
    out[pre + "step"] = np.float64(step)
    out[pre + "x"], out[pre + "a"], out[pre + "mask"] = npy(x), npy(a), npy(m)
    out[pre + "loss"], out[pre + "z"], out[pre + "h_hat"], out[pre + "x_hat"] = npy(loss), npy(vi.z), npy(vi.h_hat), npy(vi.x_hat)
    out[pre + "model_name"] = np.array(dec.model_name)
    out.update(sd_arrays(enc, pre + "enc_"))
    out.update(sd_arrays(dec, pre + "dec_"))
    for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
        for n, p in mod.named_parameters():
            out[pre + tag + n.replace(".", "__")] = npy(p.grad if p.grad is not None else torch.zeros_like(p))
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic reduction order
    gen()
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
