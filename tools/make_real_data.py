#!/usr/bin/env python
"""Write a SYNTHETIC data set in the layout `dataloader.DataGeneratorReal` reads, for trying the real-data flow without the
licensed DDW data: `python tools/make_real_data.py --out data/ --patients 2097 --hours 120`.

Four pickles of float32 numpy arrays: array_xt{data_type}.pkl (T, N, labs) and array_xt_mask{data_type}.pkl (T, N, labs)
are the measurements and masks of `DataGeneratorRoche` (the GPU generator kernel, hourly grid, time_dim = T),
array_at{data_type}.pkl (T, N, 1) is that generator's dose channel, array_x_constant.pkl (N, statics) holds seeded standard
normals.  Nothing in them is patient data; README.txt next to them says so."""
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

LATENT_DIM, OUTPUT_SIGMA, DOSE_MAX, P_REMOVE = 6, 0.2, 10, 0.5
README = ("SYNTHETIC data written by tools/make_real_data.py (patients {patients}, hours {hours}, labs {labs}, statics {statics}, "
          "seed {seed}).\nMeasurements, masks and doses come from the simulated hybrid ODE of dataloader.DataGeneratorRoche, the "
          "statics are standard normals.\nNo file here holds or derives from patient data.\n")


def generator(patients, hours, labs, seed, device):
    """The seeded `DataGeneratorRoche` behind the files, data generated."""
    np.random.seed(seed)
    dg = dataloader.DataGeneratorRoche(patients, labs, hours - 1, 1, sim_config.RochConfig(kel=1), OUTPUT_SIGMA, DOSE_MAX,
                                       LATENT_DIM, p_remove=P_REMOVE, val_size=0, test_size=0, device=device)
    dg.generate_data()
    return dg


def main(argv=None):
    ap = argparse.ArgumentParser(description="Write a SYNTHETIC (simulated, not patient) data set in DataGeneratorReal's layout.")
    ap.add_argument("--out", required=True)
    ap.add_argument("--patients", type=int, default=2097)
    ap.add_argument("--hours", type=int, default=120)
    ap.add_argument("--labs", type=int, default=24)
    ap.add_argument("--statics", type=int, default=11)
    ap.add_argument("--seed", type=int, default=666)
    ap.add_argument("--data_type", default="5")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dg = generator(a.patients, a.hours, a.labs, a.seed, torch.device(a.device))
    statics = np.random.randn(a.patients, a.statics)     # the stream np.random.seed(seed) started, behind the generator's draws
    npy = lambda x: np.ascontiguousarray(x.cpu().numpy(), dtype=np.float32)
    os.makedirs(a.out, exist_ok=True)
    for name, arr in (("array_xt{}.pkl".format(a.data_type), npy(dg.measurements)),
                      ("array_xt_mask{}.pkl".format(a.data_type), npy(dg.masks)),
                      ("array_at{}.pkl".format(a.data_type), npy(dg.actions)),
                      ("array_x_constant.pkl", statics.astype(np.float32))):
        with open(os.path.join(a.out, name), "wb") as f:
            pickle.dump(arr, f)
    with open(os.path.join(a.out, "README.txt"), "w") as f:
        f.write(README.format(**vars(a)))
    print("%s: %d patients x %d hours, %d labs, %d statics, %d failed solves; SYNTHETIC" % (
        a.out, a.patients, a.hours, a.labs, a.statics, int((dg.status != 0).sum())))


if __name__ == "__main__":
    main()
