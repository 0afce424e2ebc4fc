#!/usr/bin/env python
"""Sylvester-flow posterior timing on the device: forward + backward through autograd of

    fused     flow.sylvester_posterior_sample: hode_snf_fwd + hode_snf_bwd (libhode_snf.so), one launch each way
    composed  the same posterior from what libhode_sylvester.so offers: torch ops for r1 / r2 / Q, z0, the output layer and
              the KL around the flow.sylvester_chain kernel pair
    eager     the module loop: one eager flow step per draw and flow on (B, D) tensors, autograd backward

at the flow script's shape (B 10, D 6, K 4, 51 draws) and at B 10 000, D 12, for both flow types, on the same device in
one call.  The three are timed in alternating rounds (fused, composed, fused, composed, ...; the eager loop every
`--eager-every` rounds), HIP events around each step; every line gives the median and the spread (min .. max) of the
repeats.  Each shape is warmed up first and the clock is ramped by a quarter of a second of the fused pair.

    python tools/snf_probe.py [--reps 30] [--eager-every 10] [--out profiles/snf_probe.txt]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import flow  # noqa: E402
import model  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = ((10, 6, 4, 51), (10000, 12, 4, 51))  # (B, D, K, S)


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def ramp(fn, seconds=0.25):
    t0 = time.time()
    while time.time() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def inputs(B, D, K, S, H):
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    heads = [0.1 * torch.rand(B, D, device=DEV, generator=g), -5.0 + 0.3 * rn(B, D), 0.5 * rn(B, K, D, D) / D ** 0.5,
             rn(B, K, D), rn(B, K, D), 0.3 * rn(B, K, D), rn(B, K, H, D) if H else None]
    return [None if h is None else h.requires_grad_(True) for h in heads], rn(S, B, D)


def objective(z_out, kl):
    return z_out[0].sum() + kl.mean()   # the decoder's draw and the KL term, as VariationalInferenceFlow.loss uses them


def fused_step(heads, noise):
    objective(*flow.sylvester_posterior_sample(*heads, noise, 1)).backward()


def composed_step(heads, noise):
    mu, log_var, full_d, diag1, diag2, bias, v = heads
    r1, r2, q, perm = flow.sylvester_flow_parameters(full_d, diag1, diag2, v)
    z0 = noise * torch.exp(0.5 * log_var) + mu
    z, logdet = flow.sylvester_chain(z0, r1, r2, bias, q, perm)
    z_out = torch.exp(z - 5.0)
    log_q = model.GaussianReparam.log_density(mu, log_var, z0) - logdet - torch.sum(z - 5.0, dim=-1)
    objective(z_out, torch.mean((log_q - model.ExponentialPrior.log_density(z_out))[1:], dim=0)).backward()


def eager_step(heads, noise):
    mu, log_var, full_d, diag1, diag2, bias, v = heads
    r1, r2, q, perm = flow.sylvester_flow_parameters(full_d, diag1, diag2, v)
    zs, kls = [], []
    for s in range(noise.shape[0]):
        z0 = noise[s] * torch.exp(0.5 * log_var) + mu
        z, logdet = z0, 0.0
        for k in range(full_d.shape[1]):
            z, log_diag = flow._sylvester_step_eager(z, r1[:, k], r2[:, k], bias[:, k], None if q is None else q[:, k],
                                                     None if perm is None else perm[k])
            logdet = logdet + log_diag.sum(-1)
        z_out = torch.exp(z - 5.0)
        log_q = model.GaussianReparam.log_density(mu, log_var, z0) - logdet - torch.sum(z - 5.0, dim=-1)
        zs.append(z_out)
        kls.append(log_q - model.ExponentialPrior.log_density(z_out))
    objective(torch.stack(zs), torch.stack(kls[1:]).mean(0)).backward()


def stats(ts):
    ts = sorted(ts)
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1], "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--eager-every", type=int, default=10)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    lines, res = [], {}
    for B, D, K, S in SHAPES:
        for H in (0, min(D, 8)):
            heads, noise = inputs(B, D, K, S, H)
            steps = {"fused": fused_step, "composed": composed_step, "eager": eager_step}
            for fn in steps.values():
                fn(heads, noise)
            for fn in (fused_step, composed_step):
                for _ in range(3):
                    fn(heads, noise)
            ramp(lambda: fused_step(heads, noise))
            ts = {k: [] for k in steps}
            for r in range(a.reps):
                ts["fused"].append(event_time(lambda: fused_step(heads, noise)))
                ts["composed"].append(event_time(lambda: composed_step(heads, noise)))
                if r % a.eager_every == 0:
                    ts["eager"].append(event_time(lambda: eager_step(heads, noise)))
            key = "%s_B%d_D%d_K%d_S%d_H%d" % ("householder" if H else "triangular", B, D, K, S, H)
            res[key] = {k: stats(v) for k, v in ts.items()}
            f, c, e = (res[key][k] for k in ("fused", "composed", "eager"))
            apart = f["max_us"] < c["min_us"]
            lines.append("%s: fused %.1f us (%.1f .. %.1f, n %d) | composed %.1f us (%.1f .. %.1f, n %d): x%.2f, %s | eager loop "
                         "%.1f us (%.1f .. %.1f, n %d): x%.1f"
                         % (key, f["median_us"], f["min_us"], f["max_us"], f["n"], c["median_us"], c["min_us"], c["max_us"], c["n"],
                            c["median_us"] / f["median_us"],
                            "the ranges do not overlap" if apart else "THE RANGES OVERLAP: no difference beyond the spread",
                            e["median_us"], e["min_us"], e["max_us"], e["n"], e["median_us"] / f["median_us"]))
            print(lines[-1], flush=True)
    lines.append(json.dumps(res))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
