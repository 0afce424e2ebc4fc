#!/usr/bin/env python
"""Generate ``tests/golden/g14_generator.npz`` (G14) from the REFERENCE's ``dataloader.DataGeneratorRoche``.

Run in the build container only, like ``make_golden.py``:

    python tests/golden/make_golden_generator.py

Three cases of 48 patients (val 10, test 10) under ``np.random.seed(666)`` / ``torch.manual_seed(666)``:
``sim_config.dim8_config``, ``dim12_config`` and ``DataConfig(latent_dim=4, dose_max=10, output_sigma=0.2)``.  Per case
``c<i>_``: ``output_coef``, ``ml_coef``, the float64 initial states, ``dose_time``, ``dose_amount`` and the reference's
``latents``, ``actions`` and ``masks`` (bit-packed) of all patients.  The per-patient output noise is re-drawn from the numpy
state saved around each ``solve`` call; LSODA draws nothing, so the noise of patient n is simply the n-th
``randn(obs, T)`` of the stream after ``get_action``, which a test replays: to stay below the size of G7 the file keeps the
noise of the first N_NOISE patients only (to pin the replay) and the measurements of the first N_MEAS patients (every
value of which depends on all 48 through the z-score).  Only arrays are written."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import dataloader  # noqa: E402  (reference)
import sim_config  # noqa: E402  (reference)

N, VAL, TEST, SEED = 48, 10, 10, 666
N_NOISE, N_MEAS = 2, 16
CASES = (sim_config.dim8_config, sim_config.dim12_config,
         sim_config.DataConfig(latent_dim=4, dose_max=10, output_sigma=0.2))


def gen():
    out = {"meta": np.array([N, VAL, TEST, SEED, N_NOISE, N_MEAS], dtype=np.int64)}
    for ci, c in enumerate(CASES):
        pre = "c%d_" % ci
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        dg = dataloader.DataGeneratorRoche(N, c.obs_dim, c.t_max, c.step_size, sim_config.RochConfig(kel=1), c.output_sigma,
                                           c.dose_max, c.latent_dim, c.sparsity, p_remove=c.p_remove,
                                           output_sparsity=c.output_sparsity, device=torch.device("cpu"), val_size=VAL,
                                           test_size=TEST)
        inits, noises = [], []
        orig_init, orig_solve = dg.get_initial_conditions, dg.solve

        def get_initial_conditions():
            inits.append(orig_init())
            return inits[-1]

        def solve(init, dose_times, dose_amount):
            before = np.random.get_state()
            res = orig_solve(init, dose_times, dose_amount)
            after = np.random.get_state()
            np.random.set_state(before)
            noises.append(np.random.randn(dg.obs_dim, dg.time_dim))
            assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), after))
            return res

        dg.get_initial_conditions, dg.solve = get_initial_conditions, solve
        dg.generate_data()
        assert len(noises) == N and dg.latents.shape == (dg.time_dim, N, c.latent_dim)
        out[pre + "config"] = np.array([c.obs_dim, c.latent_dim, c.t_max, c.step_size, c.sparsity, c.output_sparsity,
                                        c.output_sigma, c.dose_max, c.p_remove], dtype=np.float64)
        out[pre + "output_coef"] = dg.output_coef
        out[pre + "ml_coef"] = dg.ml_coef
        out[pre + "init"] = inits[0]
        out[pre + "dose_time"] = dg.dose_time.astype(np.int64)
        out[pre + "dose_amount"] = dg.dose_amount
        out[pre + "noise"] = np.stack(noises[:N_NOISE]).transpose(2, 0, 1)              # (T, N_NOISE, obs) float64
        out[pre + "latents"] = dg.latents.numpy()
        out[pre + "actions"] = dg.actions.numpy()
        out[pre + "measurements"] = dg.measurements.numpy()[:, :N_MEAS]
        out[pre + "masks"] = np.packbits(dg.masks.numpy().astype(np.uint8))
        out[pre + "masks_shape"] = np.array(dg.masks.shape, dtype=np.int64)
    path = os.path.join(HERE, "g14_generator.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen()
