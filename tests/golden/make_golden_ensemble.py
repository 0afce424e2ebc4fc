#!/usr/bin/env python
"""Generate ``tests/golden/g12_ensemble_eval.npz`` (G12) from the REFERENCE's two-model evaluators:
``training_utils.evaluate_ensemble`` and ``evaluate_ensemble_horizon`` (training_utils.py:383-565), run on the
reference's own ``EncoderLSTM`` / ``RocheExpertDecoder`` pair of ``experiments/run_simulation_ensemble.py`` (an
expert-only model, D = 4, and a NeuralODE, D = 6).

Run in the build container only, like ``make_golden_flow.py`` (``torchdiffeq`` -> the oracle solver;
``properscoring.crps_ensemble`` -> ``oracle.evalmetrics.crps_ensemble``, the package is not installed):

    HODE_REFERENCE_TREE=<checkout of the reference> python tests/golden/make_golden_ensemble.py

Every run: CPU, rk4 on a step-0.125 grid, obs 20, T = 10, t0 = 5.  Runs ``s_`` (scalar weights 1 / 1) and ``w_``
((T, 1, obs) weight tensors) have two test chunks of three patients, each of whom keeps an observation after t0
(asserted: the NaN-free path); run ``n_`` is tiny -- one chunk of two patients, the second fully unobserved after t0 -- and
pins what the reference does with the NaN that follows.  Recorded per run: both state dicts, the data, the weights, the
seed, the printed lines, the returned tuple and the returned dict.  Only arrays are written."""

import contextlib
import io
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

from oracle.evalmetrics import crps_ensemble as oracle_crps_ensemble  # noqa: E402
from oracle.solvers import odeint as oracle_odeint  # noqa: E402

_stub = types.ModuleType("torchdiffeq")
_stub.odeint = oracle_odeint
sys.modules["torchdiffeq"] = _stub
_ps = types.ModuleType("properscoring")
_ps.crps_ensemble = oracle_crps_ensemble
sys.modules["properscoring"] = _ps
sys.path.insert(0, REF)

import model  # noqa: E402  (reference)
import training_utils  # noqa: E402  (reference)

CPU = torch.device("cpu")
OBS, ACT, D_EXPERT, D_ML, T, T0, STEP = 20, 1, 4, 6, 10, 5, 0.125
# (prefix, patients, batch size, mc_itr of evaluate_ensemble, mc_itr of the horizon call, tensor weights, blind patient)
RUNS = (("s_", 6, 3, 5, 4, False, False), ("w_", 6, 3, 5, 4, True, False), ("n_", 2, 2, 3, 3, False, True))


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(module, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in module.state_dict().items()}


class Folds:
    """The part of the reference's data generator the evaluators read."""
    expert_dim = D_EXPERT

    def __init__(self, n, seed, blind):
        g = torch.Generator().manual_seed(seed)
        self.test_size = n
        self.data = {
            "measurements": 0.5 * torch.randn(T, n, OBS, generator=g),
            "masks": (torch.rand(T, n, OBS, generator=g) < 0.6).float(),
            "latents": torch.rand(T, n, D_ML, generator=g) * 0.05,
            "actions": torch.zeros(T, n, ACT),
        }
        idx = torch.randint(0, T - 1, (n,), generator=g)
        self.data["actions"][idx, torch.arange(n), 0] = torch.rand(n, generator=g) * 5 + 0.5
        if blind:
            self.data["masks"][T0:, n - 1, :] = 0.0

    def get_split(self, fold, bs, chunk=0):
        assert fold == "test"
        return {k: v[:, chunk * bs:(chunk + 1) * bs] for k, v in self.data.items()}


def models(seed):
    t_max = (T - 1) * STEP
    torch.manual_seed(seed)
    pair = []
    for D, roche in ((D_EXPERT, True), (D_ML, False)):
        enc = model.EncoderLSTM(OBS + ACT, 2 * OBS, D, device=CPU, normalize=roche)
        dec = model.RocheExpertDecoder(OBS, D, ACT, t_max, STEP, roche=roche, method="rk4", device=CPU)
        prior = model.ExponentialPrior.log_density if roche else None
        pair.append(model.VariationalInference(enc, dec, prior_log_pdf=prior, elbo=True))
    return pair


def gen():
    out = {"runs": np.array([r[0] for r in RUNS])}
    for ri, (pre, n, bs, mc, mc_h, tensor_w, blind) in enumerate(RUNS):
        folds = Folds(n, 1200 + ri, blind)
        seen = folds.data["masks"][T0:].sum(dim=(0, 2))
        if blind:
            assert (seen[:-1] > 0).all() and seen[-1] == 0
        else:
            assert (seen > 0).all(), "every patient must keep an observation after t0 (the NaN-free path)"
        expert, ml = models(1210 + ri)
        if tensor_w:
            g = torch.Generator().manual_seed(1220 + ri)
            w_e, w_m = torch.zeros(T, 1, OBS), torch.zeros(T, 1, OBS)
            w_e[T0:] = 1.2 * torch.rand(T - T0, 1, OBS, generator=g)
            w_m[T0:] = 1.2 * torch.rand(T - T0, 1, OBS, generator=g)
        else:
            w_e, w_m = 1, 1
        seed = 1230 + ri
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            torch.manual_seed(seed)
            tup = training_utils.evaluate_ensemble(expert, ml, folds, bs, T0, mc_itr=mc, weight_expert=w_e, weight_ml=w_m)
        torch.manual_seed(seed)
        hz = training_utils.evaluate_ensemble_horizon(expert, ml, folds, bs, T0, mc_itr=mc_h, weight_expert=w_e, weight_ml=w_m)
        lines = buf.getvalue().strip().split("\n")
        assert len(lines) == 4 and len(tup) == 6
        if not blind:
            assert all(np.isfinite(v) for v in tup) and all(np.isfinite(v).all() for v in hz.values())
        out[pre + "meta"] = np.array([n, bs, mc, mc_h, seed, int(tensor_w), int(blind)], dtype=np.int64)
        for k, v in folds.data.items():
            out[pre + "data_" + k] = npy(v)
        out[pre + "w_e"] = npy(w_e) if tensor_w else np.array(float(w_e))
        out[pre + "w_m"] = npy(w_m) if tensor_w else np.array(float(w_m))
        for tag, vi in (("e", expert), ("m", ml)):
            out.update(sd_arrays(vi.encoder, "%s%s_enc_" % (pre, tag)))
            out.update(sd_arrays(vi.decoder, "%s%s_dec_" % (pre, tag)))
        out[pre + "lines"] = np.array(lines)
        out[pre + "tuple"] = np.array([float(v) for v in tup], dtype=np.float64)
        for k, v in hz.items():
            out[pre + "hz_" + k] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, "g12_ensemble_eval.npz"), **out)


if __name__ == "__main__":
    gen()
