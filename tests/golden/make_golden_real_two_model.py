#!/usr/bin/env python
"""Generate ``tests/golden/g13_real_two_model.npz`` (G13) from the REFERENCE's real-data two-model scripts:
``experiments.run_real_ensemble.run`` and ``experiments.run_real_residual.run``, with ``ode_method="midpoint"`` as in
``experiments/real.sh``.

Run in the build container only, like ``make_golden_ensemble.py`` (``torchdiffeq`` -> the oracle solver,
``properscoring`` stubbed: the package is not installed and these scripts never call it; scipy is needed):

    HODE_REFERENCE_TREE=<checkout of the reference> python tests/golden/make_golden_real_two_model.py

The scripts read four DDW-shaped pickles from ``../data/``; this script writes synthetic ones into a temporary directory
and runs there: 997 + 100 + 5 patients (the constructor's 2097 only fixes the training fold at 997; the folds are slices),
T = 37 (13 forecast steps: the horizons 6 and 12 are distinct, 24 and 72 are clipped), obs 10 (``latent_dim=10`` slices the
mask), three static columns with nonzero values, the last test patient unobserved after t0 = 24.  The scripts'
module-global ``weight`` is set to False and the checkpoints are made by the scripts' own ``init_and_load(...,
init_path=None)`` plus ``vi.save``.  Everything a run computes but does not return is recorded from outside: every
decoder call's forecast (a wrapper around the two decoder classes' ``forward``), every ``nnls`` result, the residual
run's trained model (a wrapper around ``variational_training_loop``), and ``bootstrap_RMSE`` is reseeded before every
call with a recorded seed.  The ml model's readout is perturbed with a recorded seed until at least three of the four
NNLS active sets occur over the steps; every step's Gram determinant is asserted to exceed 1e-6 a11 a22.
Only arrays are written."""

import contextlib
import io
import os
import pickle
import sys
import tempfile
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
sys.modules.setdefault("properscoring", types.ModuleType("properscoring"))
sys.path.insert(0, REF)

import dataloader  # noqa: E402  (reference)
import model  # noqa: E402  (reference)
import sim_config  # noqa: E402  (reference)
import training_utils  # noqa: E402  (reference)
from experiments import run_real_ensemble as ens  # noqa: E402  (reference)
from experiments import run_real_residual as res  # noqa: E402  (reference)

N_TRAIN, N_VAL, N_TEST, T, T0, OBS, STATIC = 997, 100, 5, 37, 24, 10, 3
NITERS, DATA_SEED, BOOT_SEED0 = 3, 1300, 1310


def npy(x):
    return x.detach().cpu().numpy()


def sd_arrays(sd, prefix):
    return {prefix + k.replace(".", "__"): npy(v) for k, v in sd.items()}


def write_pickles(data_dir):
    g = torch.Generator().manual_seed(DATA_SEED)
    n = N_TRAIN + N_VAL + N_TEST
    trend = torch.linspace(-0.4, 0.4, T)[:, None, None]
    x = 0.5 * torch.randn(T, n, OBS, generator=g) + trend * torch.randn(1, 1, OBS, generator=g)
    mask = (torch.rand(T, n, OBS, generator=g) < 0.6).float()
    mask[T0:, n - 1, :] = 0.0                                   # the last test patient: nothing observed after t0
    act = (torch.rand(T, n, 1, generator=g) < 0.15).float() * torch.rand(T, n, 1, generator=g)
    stat = 0.1 + 0.4 * torch.rand(n, STATIC, generator=g)       # nonzero: every column is added into the expert's dose
    for name, arr in (("array_xt_mask5", mask), ("array_xt5", x), ("array_at5", act), ("array_x_constant", stat)):
        with open(os.path.join(data_dir, name + ".pkl"), "wb") as f:
            pickle.dump(arr.numpy(), f)


def generator():
    dg = dataloader.DataGeneratorReal(2097, 1, 1, 1, sim_config.RochConfig(), 1, val_size=N_VAL, test_size=1000, latent_dim=10,
                                      data_type="5")
    dg.split_sample()
    return dg


class Recorder:
    """Wraps, from outside, what the scripts call but do not return."""

    def __init__(self):
        self.forecasts, self.nnls, self.seeds, self.trained = [], [], [], None
        self._orig = {}

    def __enter__(self):
        rec = self

        def wrap_forward(cls):
            orig = cls.forward

            def forward(self_, init, a, s):
                out = orig(self_, init, a, s)
                rec.forecasts.append((cls.__name__, a.shape[1], a.shape[2], out[0].detach().clone()))
                return out
            rec._orig[(cls, "forward")] = orig
            cls.forward = forward

        wrap_forward(model.DecoderReal)
        wrap_forward(model.DecoderRealBenchmark)
        orig_nnls = ens.nnls

        def nnls(A, b):
            out = orig_nnls(A, b)
            rec.nnls.append((np.array(out[0], dtype=np.float64), np.array(A, dtype=np.float64), np.array(b, dtype=np.float64)))
            return out
        self._orig[(ens, "nnls")] = orig_nnls
        ens.nnls = nnls
        orig_boot = training_utils.bootstrap_RMSE

        def bootstrap_RMSE(err_sq):
            seed = BOOT_SEED0 + len(rec.seeds)
            rec.seeds.append(seed)
            torch.manual_seed(seed)
            return orig_boot(err_sq)
        self._orig[(training_utils, "bootstrap_RMSE")] = orig_boot
        training_utils.bootstrap_RMSE = bootstrap_RMSE
        orig_loop = training_utils.variational_training_loop

        def loop(*args, **kwargs):
            out = orig_loop(*args, **kwargs)
            rec.trained = ({k: v.clone() for k, v in out[0].encoder.state_dict().items()},
                           {k: v.clone() for k, v in out[0].decoder.state_dict().items()})
            return out
        self._orig[(training_utils, "variational_training_loop")] = orig_loop
        training_utils.variational_training_loop = loop
        return self

    def __exit__(self, *exc):
        for (owner, name), fn in self._orig.items():
            setattr(owner, name, fn)


def run_script(mod, **kw):
    buf = io.StringIO()
    with Recorder() as rec, contextlib.redirect_stdout(buf):
        mod.run(ode_method="midpoint", init_path="model/", **kw)
    lines = [l for l in buf.getvalue().strip().split("\n") if l.startswith("rmse_x,")]
    assert len(lines) == 4 and len(rec.seeds) == 4, buf.getvalue()
    return rec, lines


def fold_arrays(data, prefix):
    out = {prefix + k: npy(data[k]) for k in ("measurements", "actions", "masks")}
    assert bool((data["statics"] == data["statics"][:1]).all())
    out[prefix + "statics"] = npy(data["statics"][0])            # constant along time: (B, static)
    return out


def active_sets(w):
    return sorted({int(a > 0) + 2 * int(b > 0) for a, b in w})


def gen():
    ens.weight = False
    res.weight = False
    out = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data"))
        os.makedirs(os.path.join(tmp, "work", "model"))
        write_pickles(os.path.join(tmp, "data"))
        os.chdir(os.path.join(tmp, "work"))
        try:
            dg = generator()
            assert (dg.train_size, dg.t_max, dg.obs_dim, dg.static_dim) == (N_TRAIN, T, OBS, STATIC)
            assert dg.data_val["measurements"].shape == (T, N_VAL, OBS) and dg.data_test["measurements"].shape == (T, N_TEST, OBS)
            torch.manual_seed(DATA_SEED + 1)
            expert = ens.init_and_load(dg, 4, 1.2, 1, "expert", "midpoint", None, T0)
            ml = ens.init_and_load(dg, 20, 1.2, 1, "gruode", "midpoint", None, T0)
            expert.save("model/", 0, 0.0)
            base = {k: v.clone() for k, v in ml.decoder.state_dict().items()}
            for perturb_seed in range(1320, 1360):
                g = torch.Generator().manual_seed(perturb_seed)
                sd = {k: v.clone() for k, v in base.items()}
                for k in ("output_function.2.weight", "output_function.2.bias"):
                    sd[k] = sd[k] + 0.3 * torch.randn(sd[k].shape, generator=g)
                ml.decoder.load_state_dict(sd)
                ml.save("model/", 0, 0.0)
                rec, lines = run_script(ens)
                w = np.stack([r[0] for r in rec.nnls])
                dets = [(A[:, 0] @ A[:, 0]) * (A[:, 1] @ A[:, 1]) - (A[:, 0] @ A[:, 1]) ** 2 for _, A, _ in rec.nnls]
                ok = all(d > 1e-6 * (A[:, 0] @ A[:, 0]) * (A[:, 1] @ A[:, 1]) for d, (_, A, _) in zip(dets, rec.nnls))
                print("perturb seed %d: active sets %s, det condition %s" % (perturb_seed, active_sets(w), ok))
                if len(active_sets(w)) >= 3 and ok:
                    break
            else:
                sys.exit("no perturbation of the ml readout gave three NNLS active sets")
            assert w.shape == (T - T0, 2) and len(active_sets(w)) >= 3 and ok
            # decoder calls of the ensemble run: expert (val), ml (val), expert (test), ml (test)
            kinds = [(f[0], f[1], f[2]) for f in rec.forecasts]
            assert kinds == [("DecoderReal", N_VAL, 1 + STATIC), ("DecoderRealBenchmark", N_VAL, 1),
                             ("DecoderReal", N_TEST, 1 + STATIC), ("DecoderRealBenchmark", N_TEST, 1)], kinds
            ev = pickle.load(open("model/ensembleeval.pkl", "rb"))
            out["meta"] = np.array([T, T0, OBS, STATIC, N_VAL, N_TEST, NITERS, perturb_seed], dtype=np.int64)
            out.update(fold_arrays(dg.data_val, "val_"))
            out.update(fold_arrays(dg.data_test, "test_"))
            out.update(sd_arrays(expert.encoder.state_dict(), "e_enc_"))
            out.update(sd_arrays(expert.decoder.state_dict(), "e_dec_"))
            out.update(sd_arrays(ml.encoder.state_dict(), "ens_m_enc_"))
            out.update(sd_arrays(ml.decoder.state_dict(), "ens_m_dec_"))
            out["ens_weights"] = w                                                     # (T', 2) float64, scipy's
            out["ens_val_x_hat_e"], out["ens_val_x_hat_m"] = npy(rec.forecasts[0][3]), npy(rec.forecasts[1][3])
            out["ens_test_x_hat_e"], out["ens_test_x_hat_m"] = npy(rec.forecasts[2][3]), npy(rec.forecasts[3][3])
            out["ens_x_hat"] = npy(ev["x_hat"])
            out["ens_lines"], out["ens_seeds"] = np.array(lines), np.array(rec.seeds, dtype=np.int64)
            assert np.array_equal(npy(ev["x"]), out["test_measurements"])

            # the residual run trains its own ml model (NITERS iterations) and mutates the training fold: a fresh process
            # state is not needed, the script builds its own generator and models
            rec, lines = run_script(res, niters=NITERS)
            assert rec.trained is not None
            kinds = [(f[0], f[1], f[2]) for f in rec.forecasts]
            assert kinds[0] == ("DecoderReal", N_TRAIN, 1 + STATIC) and kinds[-2:] == [
                ("DecoderReal", N_TEST, 1 + STATIC), ("DecoderRealBenchmark", N_TEST, 1)], kinds
            ev = pickle.load(open("model/residualeval.pkl", "rb"))
            out.update(sd_arrays(rec.trained[0], "res_m_enc_"))
            out.update(sd_arrays(rec.trained[1], "res_m_dec_"))
            out["res_test_x_hat_e"], out["res_test_x_hat_m"] = npy(rec.forecasts[-2][3]), npy(rec.forecasts[-1][3])
            out["res_x_hat"] = npy(ev["x_hat"])
            out["res_lines"], out["res_seeds"] = np.array(lines), np.array(rec.seeds, dtype=np.int64)
            assert np.array_equal(out["res_test_x_hat_e"], out["ens_test_x_hat_e"])   # the same expert checkpoint
        finally:
            os.chdir(cwd)
    for k, v in out.items():
        assert v.dtype != object, k
    path = os.path.join(HERE, "g13_real_two_model.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print("\n".join(out["ens_lines"]), "\n" + "\n".join(out["res_lines"]))


if __name__ == "__main__":
    gen()
