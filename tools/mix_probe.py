#!/usr/bin/env python
"""Two-model mixture CRPS timing on the device, three ways in one process:

  (a) fused:     hode.mix.mixture_crps -- one hode_mix_crps launch, both readouts and the weights applied on the fly;
  (b) composed:  the same field from what shipped before the kernel: two torch readouts of the latent trajectories, the
                 weighted mix, and hode.crps.ensemble_crps with the identity readout over the materialised x_hat;
  (c) eager:     the reference's way (training_utils.py:453-463) -- stacked x_hat copied to the host and one
                 crps_ensemble call per element from three nested Python loops -- on a small sample, scaled to the shape.

Shapes: the three simulation shapes (obs, De, Dm) at B 50, M 50, T' 9 (batch 50, mc_itr 50, 14 steps with t0 5), and the
benchmark's batch (B 10 000) at its shape (obs 80, D 12).  Each figure is the median of `--reps` timed windows (HIP
events around `calls` back-to-back calls) after the path has been replayed for 60 ms; the spread is max - min of the
windows.  Condition printed per shape: (a) is no slower than (b) beyond (b)'s own spread.

    python tools/mix_probe.py [--reps 5]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

from hode.crps import ensemble_crps  # noqa: E402
from hode.mix import mixture_crps, rows_per_workgroup  # noqa: E402
from oracle.evalmetrics import crps_ensemble  # noqa: E402

DEV = torch.device("cuda:0")
WARM_MS = 60.0
SHAPES = ((20, 4, 6, 50), (40, 4, 8, 50), (80, 4, 12, 50), (80, 4, 12, 10000))   # (obs, De, Dm, B)
M, TN = 50, 9


def windows(fn, reps, calls):
    """Per-call microseconds of `reps` windows of `calls` calls, after a warm replay of WARM_MS."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return sorted(out)


def inputs(obs, De, Dm, B):
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(h_e=r(TN, M * B, De), h_m=r(TN, M * B, Dm), truth=r(TN, B, obs), w_e=r(obs, De) / De ** 0.5, b_e=0.3 * r(obs),
                w_m=r(obs, Dm) / Dm ** 0.5, b_m=0.3 * r(obs), g_e=torch.rand(TN, obs, device=DEV, generator=g),
                g_m=torch.rand(TN, obs, device=DEV, generator=g))


def fused(i):
    return mixture_crps(i["h_e"], i["h_m"], i["truth"], M, (i["w_e"], i["b_e"]), (i["w_m"], i["b_m"]), weight_e=i["g_e"],
                        weight_m=i["g_m"], per_component=True)


def composed(i):
    x_e = torch.addmm(i["b_e"], i["h_e"].reshape(-1, i["h_e"].shape[-1]), i["w_e"].t()).reshape(TN, -1, i["w_e"].shape[0])
    x_m = torch.addmm(i["b_m"], i["h_m"].reshape(-1, i["h_m"].shape[-1]), i["w_m"].t()).reshape(TN, -1, i["w_m"].shape[0])
    x = x_e * i["g_e"][:, None, :] + x_m * i["g_m"][:, None, :]
    return ensemble_crps(x, i["truth"], M, per_component=True)


def eager_sample(i, n_t=1, n_b=2):
    """Seconds per element of the reference's loop, measured on n_t x n_b x obs elements (device-to-host copy included)."""
    B = i["truth"].shape[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = composed_values(i)[:n_t, :, :n_b].permute(0, 2, 3, 1)    # (n_t, n_b, obs, M), as torch.stack(x_hat_list, -1)
    y = i["truth"]
    n = 0
    for d1 in range(n_t):
        for d2 in range(n_b):
            for d3 in range(y.shape[2]):
                crps_ensemble(y[d1, d2, d3].item(), x[d1, d2, d3, :].cpu().numpy())
                n += 1
    return (time.perf_counter() - t0) / n, B


def composed_values(i):
    x_e = (i["h_e"] @ i["w_e"].t() + i["b_e"]) * i["g_e"][:, None, :]
    x_m = (i["h_m"] @ i["w_m"].t() + i["b_m"]) * i["g_m"][:, None, :]
    return (x_e + x_m).reshape(TN, M, -1, i["truth"].shape[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res, ok_all = {}, True
    for obs, De, Dm, B in SHAPES:
        i = inputs(obs, De, Dm, B)
        fa, fb = fused(i), composed(i)
        torch.cuda.synchronize()
        diff = (fa - fb).abs().max().item()
        calls = 200 if B <= 50 else 5
        ta = windows(lambda: fused(i), a.reps, calls)
        tb = windows(lambda: composed(i), a.reps, calls)
        per_elem, _ = eager_sample(i)
        tc = per_elem * TN * B * obs * 1e6
        med_a, med_b, spread_b = ta[len(ta) // 2], tb[len(tb) // 2], tb[-1] - tb[0]
        ok = med_a <= med_b + spread_b
        ok_all = ok_all and ok
        key = "obs%d_De%d_Dm%d_B%d_M%d_T%d" % (obs, De, Dm, B, M, TN)
        res[key] = {"fused_us": med_a, "fused_spread_us": ta[-1] - ta[0], "composed_us": med_b, "composed_spread_us": spread_b,
                    "eager_us_extrapolated": tc, "eager_us_per_element": per_elem * 1e6, "rows_per_workgroup":
                    rows_per_workgroup(M, De, Dm, obs), "max_abs_diff_fused_vs_composed": diff, "condition_holds": ok}
        print("%s (%d rows per workgroup): (a) fused %.1f us [spread %.1f], (b) composed %.1f us [spread %.1f], x%.2f; "
              "(c) eager loop %.0f us per element -> %.3g s at this shape; max |a - b| = %.2e; (a) <= (b) + spread(b): %s"
              % (key, res[key]["rows_per_workgroup"], med_a, ta[-1] - ta[0], med_b, spread_b, med_b / med_a, per_elem * 1e6,
                 tc * 1e-6, diff, "holds" if ok else "FAILS"), flush=True)
    res["condition_holds_at_every_shape"] = ok_all
    print(json.dumps(res))


if __name__ == "__main__":
    main()
