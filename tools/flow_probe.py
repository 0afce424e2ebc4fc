#!/usr/bin/env python
"""Planar-flow posterior timing on the device: the fused pair (hode_flow_fwd + hode_flow_bwd through
hode.flow.planar_flow_sample) against the reference-style eager loop (mc_kl's Python loop over reparameterize / Planar,
autograd backward), and one full VariationalInferenceFlow training step at the script's shape.  HIP events, median of
`--reps` timed repeats after warm-up.  Prints one line per measurement and a JSON summary line.

    python tools/flow_probe.py [--reps 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import model  # noqa: E402
from hode.flow import planar_flow_sample  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def inputs(B, D, K, S):
    g = torch.Generator(device=DEV).manual_seed(0)
    mk = lambda *s, sc=0.5: (sc * torch.randn(*s, device=DEV, generator=g)).requires_grad_(True)
    return mk(B, D, sc=0.3), mk(B, D, sc=0.3), mk(B, K, D), mk(B, K, D), mk(B, K, sc=0.3), torch.randn(S, B, D, device=DEV, generator=g)


def fused_step(mu, lv, u, w, b, noise):
    z, kl = planar_flow_sample(mu, lv, u, w, b, noise, s_kl=1)
    (z[0].sum() + kl.mean()).backward()


def eager_step(enc, mu, lv, u, w, b, noise):
    """The reference's arithmetic: one reparameterize per draw (decoder draw + S - 1 KL draws), autograd backward."""
    S = noise.shape[0]
    eo = (mu, lv, u.unsqueeze(-1), w.unsqueeze(-2), b.unsqueeze(-1).unsqueeze(-1))
    _, _, z_dec, _, _ = enc.reparameterize(*eo)
    mc = []
    for _ in range(S - 1):
        m_, l_, z, ldj, z0 = enc.reparameterize(*eo)
        mc.append(enc.log_density(m_, l_, z, ldj, z0) - model.ExponentialPrior.log_density(z))
    kl = torch.stack(mc, -1).mean(-1)
    (z_dec.sum() + kl.mean()).backward()


def algorithmic_bytes(B, D, K, S):
    """noise read once per direction, z_out written (fwd) / grad_z read (bwd), parameters and gradients once."""
    params = 4 * (2 * B * D + 2 * B * K * D + B * K)
    fwd = 4 * S * B * D * 2 + params + 4 * B
    bwd = 4 * S * B * D * 2 + params + 4 * B + params
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    res = {}
    for B, D, K, S in ((10, 6, 4, 51), (10000, 12, 4, 51)):
        mu, lv, u, w, b, noise = inputs(B, D, K, S)
        enc = model.EncoderPlanarLSTM(21, 40, D, K, normalize=False, device=DEV)
        t_fwd = timed(lambda: planar_flow_sample(mu.detach(), lv.detach(), u.detach(), w.detach(), b.detach(), noise, 1), a.reps)
        t_pair = timed(lambda: fused_step(mu, lv, u, w, b, noise), a.reps)
        t_eager = timed(lambda: eager_step(enc, mu, lv, u, w, b, noise), max(3, a.reps // 10), warmup=1)
        fb, bb = algorithmic_bytes(B, D, K, S)
        key = "B%d_D%d_K%d_S%d" % (B, D, K, S)
        res[key] = {"fused_fwd_us": t_fwd, "fused_fwd_bwd_us": t_pair, "eager_fwd_bwd_us": t_eager,
                    "speedup": t_eager / t_pair, "bytes_fwd": fb, "bytes_bwd": bb,
                    "fwd_bw_frac_of_peak": fb / (t_fwd * 1e-6) / HBM_PEAK,
                    "pair_bw_frac_of_peak": (fb + bb) / (t_pair * 1e-6) / HBM_PEAK}
        print("%s: fused fwd %.1f us, fused fwd+bwd %.1f us, eager loop fwd+bwd %.1f us (x%.0f); fwd %.2f%% / pair %.2f%% of HBM peak"
              % (key, t_fwd, t_pair, t_eager, t_eager / t_pair, 100 * res[key]["fwd_bw_frac_of_peak"],
                 100 * res[key]["pair_bw_frac_of_peak"]), flush=True)

    # one full VariationalInferenceFlow training step at the script's shape (B 10, obs 20, D 6, t_max 14, dopri5, mc 50)
    from hode.batches import DeviceFolds
    folds = DeviceFolds.synthetic(200, 15, 20, 6, 20, 20, DEV, seed=2, step=1.0)
    torch.manual_seed(0)
    enc = model.EncoderPlanarLSTM(21, 40, 6, 4, normalize=False, device=DEV)
    dec = model.RocheExpertDecoder(20, 6, 1, 14, 1, roche=True, method="dopri5", device=DEV)
    vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=50)
    params = list(enc.parameters()) + list(dec.output_function.parameters()) + list(dec.ode.ml_net.parameters())
    opt = torch.optim.Adam(params, lr=0.01)
    data = folds.get_split("train", 10, 0)

    def step():
        opt.zero_grad()
        vi.loss(data).backward()
        opt.step()
    res["train_step_us"] = timed(step, max(5, a.reps // 5))
    print("VariationalInferenceFlow training step (B 10, D 6, K 4, mc 50, dopri5): %.1f us" % res["train_step_us"], flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
