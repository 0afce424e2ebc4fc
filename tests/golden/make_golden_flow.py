#!/usr/bin/env python
"""Generate ``tests/golden/g11_flow.npz`` (G11) from the REFERENCE's planar-flow posterior: ``EncoderPlanarLSTM``
(model.py:48-153), ``Planar`` (flow.py:8-59) and ``VariationalInferenceFlow`` (model.py:1299-1380).

Run in the build container only, like ``make_golden_seqdec.py`` (same stubs: ``torchdiffeq`` -> the oracle solver,
``properscoring`` empty):

    HODE_REFERENCE_TREE=<checkout of the reference> python tests/golden/make_golden_flow.py

Per case (D, K, B) on CPU, window T = 5, obs 20, action 1, hidden 40: the seeded state_dict, the inputs, the encoder
outputs, one ``reparameterize`` call with its recorded ``randn_like`` draw.  For the D = 6 case additionally
``VariationalInferenceFlow.loss`` at mc_size 1 and 50 with a ``RocheExpertDecoder`` (rk4) on an 8-step grid, the recorded
draws of the call in order (decoder draw first) and every gradient.  Only arrays are written."""

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("HODE_REFERENCE_TREE")
if not REF:
    sys.exit("set HODE_REFERENCE_TREE to a checkout of the reference code base")
sys.path.insert(0, ROOT)

from oracle.solvers import odeint as oracle_odeint  # noqa: E402

_stub = types.ModuleType("torchdiffeq")
_stub.odeint = oracle_odeint
sys.modules["torchdiffeq"] = _stub
sys.modules["properscoring"] = types.ModuleType("properscoring")
sys.path.insert(0, REF)

import model  # noqa: E402  (reference)

CPU = torch.device("cpu")
OBS, ACT, HIDDEN, TW = 20, 1, 40, 5
CASES = [(6, 4, 7, False), (12, 4, 7, False), (20, 1, 5, True), (3, 16, 5, False)]  # (D, K, B, normalize)
LOSS_T, LOSS_STEP = 8, 1.0


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(module, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in module.state_dict().items()}


class Recorder:
    """Wraps torch.randn_like and keeps every draw in call order."""

    def __init__(self):
        self.draws, self._orig = [], torch.randn_like

    def __enter__(self):
        def rec(*args, **kw):
            r = self._orig(*args, **kw)
            self.draws.append(r.detach().clone())
            return r
        torch.randn_like = rec
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def one_dose_actions(T, B, gen, dose_max=10.0):
    a = torch.zeros(T, B, 1)
    idx = torch.randint(0, T - 1, (B,), generator=gen)
    a[idx, torch.arange(B), 0] = torch.rand(B, generator=gen) * dose_max
    return a


def gen():
    out = {}
    g = torch.Generator().manual_seed(1111)
    for ci, (D, K, B, normalize) in enumerate(CASES):
        pre = "c%d_" % ci
        torch.manual_seed(1100 + ci)
        enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, D, K, normalize=normalize, device=CPU)
        out[pre + "meta"] = np.array([D, K, B, int(normalize), TW, 1100 + ci], dtype=np.int64)
        out[pre + "keys"] = np.array(list(enc.state_dict().keys()))
        out.update(sd_arrays(enc, pre + "enc_"))
        x = torch.randn(TW, B, OBS, generator=g)
        a = one_dose_actions(TW, B, g)
        m = (torch.rand(TW, B, OBS, generator=g) < 0.5).float()
        out[pre + "x"], out[pre + "a"], out[pre + "mask"] = npy(x), npy(a), npy(m)
        with torch.no_grad():
            eo = enc(x, a, m)
            for n, t in zip(("mu", "log_var", "u", "w", "b"), eo):
                out[pre + n] = npy(t)
            with Recorder() as r:
                mu, lv, z, ldj, z0 = enc.reparameterize(*eo)
        out[pre + "rep_eps"] = npy(r.draws[0])
        out[pre + "rep_z"], out[pre + "rep_log_det_j"], out[pre + "rep_z0"] = npy(z), npy(ldj), npy(z0)
        out[pre + "rep_log_density"] = npy(enc.log_density(mu, lv, z, ldj, z0))
        if D != 6:
            continue
        for mc in (1, 50):
            lp = "%sm%d_" % (pre, mc)
            torch.manual_seed(1200 + mc)
            enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, D, K, normalize=normalize, device=CPU)
            dec = model.RocheExpertDecoder(OBS, D, ACT, LOSS_T * LOSS_STEP, LOSS_STEP, roche=True, method="rk4", device=CPU)
            vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=mc)
            T = LOSS_T + 1
            xl = torch.randn(T, B, OBS, generator=g) * 0.1
            al = one_dose_actions(T, B, g)
            ml = (torch.rand(T, B, OBS, generator=g) < 0.5).float()
            data = {"measurements": xl, "actions": al, "masks": ml}
            with Recorder() as r:
                loss = vi.loss(data)
            for p in vi.parameters():
                p.grad = None
            loss.backward()
            out[lp + "model_name"] = np.array(vi.model_name)
            out[lp + "x"], out[lp + "a"], out[lp + "mask"] = npy(xl), npy(al), npy(ml)
            out[lp + "noise"] = npy(torch.stack(r.draws))
            out[lp + "loss"] = npy(loss)
            out[lp + "z"] = npy(vi.z)
            out.update(sd_arrays(enc, lp + "enc_"))
            out.update(sd_arrays(dec, lp + "dec_"))
            for prefix, mod in (("genc_", enc), ("gdec_", dec)):
                for n, p in mod.named_parameters():
                    gr = p.grad if p.grad is not None else torch.zeros_like(p)
                    out[lp + prefix + n.replace(".", "__")] = npy(gr)
    out["n_cases"] = np.array(len(CASES))
    np.savez_compressed(os.path.join(HERE, "g11_flow.npz"), **out)


if __name__ == "__main__":
    gen()
