#!/usr/bin/env python
"""Generate ``tests/golden/g16_roche_dims.npz`` (G16) from the REFERENCE's ``RocheODE`` at the latent sizes
``run_simulation --method=hybrid --encoder_output_dim=D`` reaches beside 4, 6, 8, 12, 20: D in 5, 7, 10, 15, 16.

Run in the build container only, like ``make_golden.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    python tests/golden/make_golden_roche_dims.py

The recipe is G1's (``make_golden.py::gen_roche_rhs``), with the same keys per case ``c<i>_``: the seeded state_dict, an
action with one dose per patient, states ``y`` (one patient negative: ``pow`` with exponent 2.0 stays finite), and per time
in ``t`` -- before all doses, exactly at a dose time, one ulp before it, one ulp after it, between doses, late -- the rhs
value, ``dose_at_time`` and the autograd VJP of sum(f * cot) for ``y`` and every parameter.  Cases: every size with
``ablate`` off and on, the rate constants at their defaults (off: also random ones).  Only arrays are written."""

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
DIMS = (5, 7, 10, 15, 16)
OUT = os.path.join(HERE, "g16_roche_dims.npz")
RATES = ("ec50_patho", "emax_patho", "k_dexa", "k_discure_immunereact", "k_discure_immunity", "k_disprog",
         "k_immune_disease", "k_immune_feedback", "k_immune_off", "k_immunity", "kel")


def npy(x):
    return x.detach().cpu().numpy()


def gen():
    out = {}
    g = torch.Generator().manual_seed(1616)
    step, T, B = 0.125, 24, 7
    cases = [(D, ablate, mode) for D in DIMS for ablate in (False, True) for mode in ("default", "random")
             if not (ablate and mode == "random")]
    for ci, (D, ablate, mode) in enumerate(cases):
        torch.manual_seed(1600 + ci)
        ode = model.RocheODE(D, 1, (T - 1) * step, step, ablate=ablate, device=CPU)
        if mode == "random":
            with torch.no_grad():
                for name in RATES:
                    getattr(ode, name).fill_(float(0.3 + 1.5 * torch.rand((), generator=g)))
        a = torch.zeros(T, B, 1)
        a[torch.tensor([3, 3, 8, 12, 0, 22, 8]), torch.arange(B), 0] = torch.rand(B, generator=g) * 10.0
        ode.set_action(a)
        y = torch.rand(B, D, generator=g) * 2.0
        y[1, :] = -y[1, :]
        t8 = 8 * step
        ts = [0.0, 3 * step, float(np.nextafter(np.float32(t8), np.float32(0))), t8,
              float(np.nextafter(np.float32(t8), np.float32(9))), t8 + step / 3, 2.9]
        cot = torch.randn(B, D, generator=g)
        pre = "c%d_" % ci
        out[pre + "meta"] = np.array([D, int(ablate), T, B], dtype=np.int64)
        out[pre + "mode"] = np.array(mode)
        out[pre + "step"] = np.float64(step)
        out[pre + "action"], out[pre + "y"], out[pre + "cot"] = npy(a), npy(y), npy(cot)
        out[pre + "t"] = np.array(ts, dtype=np.float32)
        out[pre + "times"], out[pre + "dosage"] = npy(ode.times), npy(ode.dosage)
        out.update({pre + "sd_" + k.replace(".", "__"): npy(v) for k, v in ode.state_dict().items()})
        fs, doses, gys, gparams = [], [], [], {}
        for t in ts:
            tt = torch.tensor(t, dtype=torch.float32)
            yy = y.clone().requires_grad_(True)
            f = ode(tt, yy)
            fs.append(npy(f))
            doses.append(npy(ode.dose_at_time(tt)))
            ode.zero_grad()
            (f * cot).sum().backward()
            gys.append(npy(yy.grad))
            for n, p in ode.named_parameters():
                gparams.setdefault(n, []).append(npy(p.grad if p.grad is not None else torch.zeros_like(p)).copy())
        out[pre + "f"], out[pre + "dose"], out[pre + "gy"] = np.stack(fs), np.stack(doses), np.stack(gys)
        for n, gr in gparams.items():
            out[pre + "g_" + n.replace(".", "__")] = np.stack(gr)
    out["n_cases"] = np.array(len(cases))
    out["dims"] = np.array(DIMS, dtype=np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d B, %d cases)" % (OUT, os.path.getsize(OUT), len(cases)))


if __name__ == "__main__":
    gen()
