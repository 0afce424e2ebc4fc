#!/usr/bin/env python
"""What the dose-table gradient of the real-data hybrid solve costs, at config 5's shape (D 20, hidden 43, the decoder's grid
from t0 = 24 to t_max = 120, perturb) at 2 097 and 8 192 patients, midpoint and rk4:

    dose    model._RocheRealDoseGrad: hode.real.real_solve forward, hode.real_dose.real_dose_backward (libhode_real_dose.so),
            which also returns d loss / d act
    plain   hode.real.real_solve through autograd (libhode.so at D = 20), no gradient for the action: the yardstick

forward + backward through autograd, gradients for y0, theta and the flat weights in both, the two timed in alternating
repeats in one process after a warm-up of every shape, HIP events around each repeat; then the backward launches alone
(hode_real_dose_bwd through the binding against the plain autograd backward with the graph kept).  Every line gives the
median with min .. max and says whether the ranges overlap.

    python tools/real_dose_probe.py [--reps 9] [--inner 3] [--out profiles/real_dose_probe.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import model  # noqa: E402
from hode.real import real_solve  # noqa: E402
from hode.real_dose import real_dose_backward  # noqa: E402

DEV = torch.device("cuda:0")
D, HIDDEN, STAT, T_MAX, T0 = 20, 43, 11, 120, 24
BATCHES = (2097, 8192)
METHODS = ("midpoint", "rk4")
WAYS = ("dose", "plain")


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def problem(B):
    gen = torch.Generator().manual_seed(D)
    torch.manual_seed(D)
    ode = model.RocheODEReal(D, 1, STAT, HIDDEN, T_MAX, 1, device=DEV)
    act = ((torch.rand(T_MAX, B, generator=gen) < 0.15).float() * torch.rand(T_MAX, B, generator=gen)).to(DEV)
    t = torch.arange(T0 - 1, T_MAX, 1, device=DEV, dtype=torch.float32)
    return dict(y0=(torch.randn(B, D, generator=gen) * 0.3).to(DEV), theta=torch.stack([ode.k_immunity, ode.kel, ode.kel2]).detach(),
                wflat=ode.flat_weights().detach(), t=t, act=act, cot=torch.randn(t.numel(), B, D, generator=gen).to(DEV))


def forward_backward(way, method, p):
    y0, theta, wflat = (p[k].detach().requires_grad_(True) for k in ("y0", "theta", "wflat"))
    if way == "dose":
        act = p["act"].detach().requires_grad_(True)
        h = model._RocheRealDoseGrad.apply(y0, theta, wflat, p["t"], act, HIDDEN, method, True)
    else:
        act = p["act"]
        h = real_solve(y0, theta, wflat, p["t"], act, HIDDEN, method=method, perturb=True)
    torch.autograd.backward(h, p["cot"])
    return act.grad


def backward_only(way, method, p):
    """A callable that runs the backward launches alone."""
    if way == "dose":
        with torch.no_grad():
            h = real_solve(p["y0"], p["theta"], p["wflat"], p["t"], p["act"], HIDDEN, method=method, perturb=True)
        return lambda: real_dose_backward(h, p["theta"], p["wflat"], p["t"], p["act"], p["cot"], HIDDEN, method=method, perturb=True)
    y0, theta, wflat = (p[k].detach().requires_grad_(True) for k in ("y0", "theta", "wflat"))
    h = real_solve(y0, theta, wflat, p["t"], p["act"], HIDDEN, method=method, perturb=True)
    return lambda: torch.autograd.grad(h, (y0, theta, wflat), p["cot"], retain_graph=True)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "n": len(ts)}


def verdict(what, st):
    a, b = st["dose"], st["plain"]
    if not (a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]):
        return "%s: dose vs plain: THE RANGES OVERLAP, no difference beyond the spread (medians x%.3f)" % (what, a["median_ms"] / b["median_ms"])
    return "%s: dose / plain = x%.3f, the ranges do not overlap" % (what, a["median_ms"] / b["median_ms"])


def cell(st):
    return " | ".join("%s %.3f ms (%.3f .. %.3f, n %d)" % (w, s["median_ms"], s["min_ms"], s["max_ms"], s["n"]) for w, s in st.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    assert a.reps >= 7
    lines = ["# tools/real_dose_probe.py --reps %d --inner %d on %s: D %d, hidden %d, t = %d .. %d (%d steps), perturb; ms per call, HIP events,"
             % (a.reps, a.inner, torch.cuda.get_device_name(0), D, HIDDEN, T0 - 1, T_MAX - 1, T_MAX - T0),
             "# median (min .. max) over the repeats of %d back-to-back calls, dose and plain alternating in one process after a warm-up" % a.inner]
    res = {}
    for B in BATCHES:
        p = problem(B)
        for method in METHODS:
            bwd = {way: backward_only(way, method, p) for way in WAYS}
            for way in WAYS:  # warm-up: code objects, allocator, clocks
                for _ in range(3):
                    g = forward_backward(way, method, p)
                    bwd[way]()
                if way == "dose":
                    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
            torch.cuda.synchronize()
            both = {way: [] for way in WAYS}
            back = {way: [] for way in WAYS}
            for _ in range(a.reps):
                for way in WAYS:
                    both[way].append(event_ms(lambda: forward_backward(way, method, p), a.inner))
                for way in WAYS:
                    back[way].append(event_ms(bwd[way], a.inner))
            st = {way: stats(v) for way, v in both.items()}
            sb = {way: stats(v) for way, v in back.items()}
            res["B%d_%s" % (B, method)] = dict(fwd_bwd=st, bwd=sb, patients=B, steps=T_MAX - T0)
            lines.append("B %d %s fwd+bwd: %s" % (B, method, cell(st)))
            lines.append("    " + verdict("fwd+bwd", st))
            lines.append("B %d %s backward launches alone: %s" % (B, method, cell(sb)))
            lines.append("    " + verdict("backward", sb))
            print("\n".join(lines[-4:]), flush=True)
    lines.append(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
