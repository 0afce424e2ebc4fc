#!/usr/bin/env python
"""Generate ``tests/golden/g20_real_loader.npz`` (G20) from the REFERENCE's ``dataloader.DataGeneratorReal``
(``dataloader.py:344-491``): what the class makes of four pickles, its folds, its batches and where it leaves numpy's
stream.

Run in the build container only, like the other ``make_golden_*`` scripts (the reference's ``dataloader`` imports numpy,
scipy, torch and its own ``global_config``; nothing is stubbed):

    HODE_REFERENCE_TREE=<checkout of the reference> python tests/golden/make_golden_real_loader.py

Inputs: four seeded arrays, T = 30, N = 23, obs = 5, three static columns, one action column, stored in the fixture
(``in_*``) so that the test can write the same pickles.  Two cases, the constructor's ``n_sample`` 23 (folds 13 / 4 / 6) and
20 (the class keeps ``train_size = 20 - 4 - 6``: folds 10 / 4 / 9), both with ``val_size=4, test_size=6, latent_dim=4,
data_type="5"`` under ``np.random.seed(666)``.  Recorded per case, in the order of the calls: the scalar attributes,
``output_coef``, ``ml_coef``, the three folds after ``split_sample()``, three ``get_mini_batch("train", 5)``,
``get_split("val", 2, 1)``, then ``set_train_size(8)`` with ``n_sample``, ``train_size`` and the train fold after it, and the
next ``np.random.rand()``.  Only arrays are written, every zip member with a fixed date, so that a second run gives the
same bytes."""

import contextlib
import io
import os
import pickle
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HODE_REFERENCE_TREE")
if not REF:
    sys.exit("set HODE_REFERENCE_TREE to a checkout of the reference code base")
sys.path.insert(0, REF)

import dataloader  # noqa: E402  (reference)
import sim_config  # noqa: E402  (reference)

T, N, OBS, STATIC, VAL, TEST, LATENT, SEED, DATA_SEED = 30, 23, 5, 3, 4, 6, 4, 666, 2000
CASES = (23, 20)
FIELDS = ("measurements", "actions", "latents", "masks", "statics")
SCALARS = ("n_sample", "obs_dim", "t_max", "step_size", "time_dim", "train_size", "val_size", "test_size", "static_dim",
           "latent_dim", "action_dim", "expert_dim", "ml_dim")


def inputs():
    rng = np.random.RandomState(DATA_SEED)
    x = rng.randn(T, N, OBS).astype(np.float32)
    mask = (rng.rand(T, N, OBS) < 0.6).astype(np.float32)
    act = ((rng.rand(T, N, 1) < 0.15) * rng.rand(T, N, 1)).astype(np.float32)
    stat = rng.randn(N, STATIC).astype(np.float32)
    return {"array_xt_mask5": mask, "array_xt5": x, "array_at5": act, "array_x_constant": stat}


def batch_arrays(batch, prefix):
    assert tuple(batch) == FIELDS, tuple(batch)
    return {prefix + k: batch[k].detach().cpu().numpy().copy() for k in FIELDS}


def record(n_sample, data_path):
    pre = "n%d_" % n_sample
    out = {}
    np.random.seed(SEED)
    dg = dataloader.DataGeneratorReal(n_sample, 1, 1, 1, sim_config.RochConfig(), 1, val_size=VAL, test_size=TEST,
                                      latent_dim=LATENT, device=torch.device("cpu"), data_type="5", data_path=data_path)
    assert type(dg.t_max) is int
    out[pre + "scalars"] = np.array([float(getattr(dg, k)) for k in SCALARS], dtype=np.float64)
    out[pre + "output_coef"], out[pre + "ml_coef"] = np.array(dg.output_coef), np.array(dg.ml_coef)
    dg.split_sample()
    for fold in ("train", "val", "test"):
        out.update(batch_arrays(getattr(dg, "data_" + fold), pre + fold + "_"))
    for i in range(3):
        out.update(batch_arrays(dg.get_mini_batch("train", 5), pre + "mini%d_" % i))
    out.update(batch_arrays(dg.get_split("val", 2, 1), pre + "split_"))
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        dg.set_train_size(8)
    out[pre + "set_train_prints"] = np.array(buf.getvalue().strip().split("\n"))
    out[pre + "after_set_train"] = np.array([dg.n_sample, dg.train_size], dtype=np.int64)
    out.update(batch_arrays(dg.data_train, pre + "cut_train_"))
    out[pre + "next_rand"] = np.array(np.random.rand(), dtype=np.float64)
    return out


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            assert arrays[k].dtype != object, k
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def gen():
    arrays = inputs()
    out = {"in_" + k: v for k, v in arrays.items()}
    out["scalar_names"] = np.array(SCALARS)
    out["cases"] = np.array(CASES, dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        for name, arr in arrays.items():
            with open(os.path.join(tmp, name + ".pkl"), "wb") as f:
                pickle.dump(arr, f)
        for n_sample in CASES:
            out.update(record(n_sample, tmp + "/"))
    assert out["n20_train_measurements"].shape[1] == 10 and out["n20_test_measurements"].shape[1] == 9
    assert out["n23_train_measurements"].shape[1] == 13 and out["n23_test_measurements"].shape[1] == 6
    path = os.path.join(HERE, "g20_real_loader.npz")
    save(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    gen()
