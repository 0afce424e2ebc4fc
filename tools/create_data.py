#!/usr/bin/env python
"""Write the data files of the reference's simulation experiments (experiments/create_data.sh and its five
generated_data/*.py scripts, restated as one table) with the GPU generator: `python tools/create_data.py [--out data]`.

Every set is seeded with 666 like the reference's; coefficients, initial states and dose schedules are then the
reference's own, the latents are its latents to solver accuracy, and the output noise and masks come from the kernel's
counter-based generator (dataloader.py).  The noise_level variants add randn * (level - 0.2) to the measurements of the
test set, as generate_data_noise.py does."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import dataloader  # noqa: E402
import sim_config  # noqa: E402

SEED = 666
_BASE = sim_config.DataConfig()
# file name -> (n_sample, val_size, test_size, obs_dim, latent_dim, output_sparsity); every set: t_max 14, step 1,
# sparsity 0.5, p_remove 0.5, output_sigma 0.2, dose_max 10, RochConfig(kel=1)
SETS = {
    "datafile_dose_exp.pkl": (1300, 100, 200, _BASE.obs_dim, _BASE.latent_dim, 0.5),          # generate_data_train.py
    "datafile_dose_exp_test.pkl": (2100, 100, 1000, _BASE.obs_dim, _BASE.latent_dim, 0.5),    # generate_data_test.py
    "datafile_dim8.pkl": (2100, 100, 1000, 40, 8, 1 - 0.375),                                 # generate_data_dim8.py
    "datafile_dim12.pkl": (2100, 100, 1000, 80, 12, 1 - 0.25),                                # generate_data_dim12.py
}
NOISE_SOURCE, NOISE_LEVELS, NOISE_NAME = "datafile_dose_exp_test.pkl", (0.4, 0.8, 1.0), "datafile_dose_noise_{}.pkl"
OUTPUT_SIGMA, DOSE_MAX = 0.2, 10


def make(name, device):
    n_sample, val_size, test_size, obs_dim, latent_dim, output_sparsity = SETS[name]
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    dg = dataloader.DataGeneratorRoche(n_sample, obs_dim, _BASE.t_max, _BASE.step_size, sim_config.RochConfig(kel=1), OUTPUT_SIGMA,
                                       DOSE_MAX, latent_dim, _BASE.sparsity, p_remove=_BASE.p_remove,
                                       output_sparsity=output_sparsity, device=device, val_size=val_size, test_size=test_size)
    dg.generate_data()
    dg.split_sample()
    return dg


def add_noise(dg, level):
    torch.manual_seed(SEED)
    with torch.no_grad():
        dg.measurements = dg.measurements + torch.randn_like(dg.measurements) * (level - 0.2)
        dg.split_sample()
    return dg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "data"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    device = torch.device(a.device)

    def dump(dg, name):
        with open(os.path.join(a.out, name), "wb") as f:
            pickle.dump(dg, f)
        print("%s: %d patients, latent_dim %d, obs_dim %d, %d failed" % (name, dg.n_sample, dg.latent_dim, dg.obs_dim,
                                                                        int((dg.status != 0).sum())))

    for name in SETS:
        dump(make(name, device), name)
    for level in NOISE_LEVELS:
        dump(add_noise(make(NOISE_SOURCE, device), level), NOISE_NAME.format(level))


if __name__ == "__main__":
    main()
