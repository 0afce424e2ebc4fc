"""The real-data hybrid rhs at the latent sizes of libhode_real_dims.so against libhode.so's size 20, at config 5's shape
(8 192 patients, t_max 120, t0 24, hidden 43, midpoint + perturb): HIP-event times of the forward and of forward +
backward through ``hode.real.real_solve``, all sizes alternating in one process, median (min .. max) over the rounds, and
the run-to-run spread of the size-20 rows -- the yardstick for "a smaller size is not slower than size 20".  Then a
reference-style eager loop (``model.RocheODEReal.forward`` through the torchdiffeq-style oracle loop, autograd backward) on
a stated sample.  Writes profiles/real_dims_probe.txt.

    python tools/real_dims_probe.py [--batch 8192] [--t-max 120] [--t0 24] [--rounds 9] [--inner 10] [--eager-batch 8192]"""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))

import torch  # noqa: E402

import hode  # noqa: E402
import model  # noqa: E402
from hode import _real_dims_lib as RD  # noqa: E402
from hode.real import real_solve  # noqa: E402
from oracle.solvers import odeint as oracle_odeint  # noqa: E402

SIZES = (8, 12, 16, 19)
HIDDEN, STAT = 43, 11


def problem(D, B, t_max, t0, dev, library):
    gen = torch.Generator().manual_seed(D)
    torch.manual_seed(D)
    ode = model.RocheODEReal(D, 1, STAT, HIDDEN, t_max, 1, device=dev)
    a = ((torch.rand(t_max, B, 1, generator=gen) < 0.15).float() * torch.rand(t_max, B, 1, generator=gen)).to(dev)
    t = torch.arange(t0 - 1, t_max, 1, device=dev, dtype=torch.float32)
    y0 = (torch.randn(B, D, generator=gen) * 0.3).to(dev).requires_grad_(True)
    theta = torch.stack([ode.k_immunity, ode.kel, ode.kel2]).detach().requires_grad_(True)
    wflat = ode.flat_weights().detach().requires_grad_(True)
    cot = torch.randn(t.numel(), B, D, generator=gen).to(dev)
    act = a[..., 0].contiguous()

    def fwd():
        with torch.no_grad():
            return real_solve(y0, theta, wflat, t, act, HIDDEN, method="midpoint", perturb=True, library=library)

    def fwd_bwd():
        y0.grad = theta.grad = wflat.grad = None
        h = real_solve(y0, theta, wflat, t, act, HIDDEN, method="midpoint", perturb=True, library=library)
        torch.autograd.backward(h, cot)
    return dict(ode=ode, a=a, t=t, y0=y0, cot=cot, fwd=fwd, fwd_bwd=fwd_bwd)


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def eager_ms(p, B):
    """One forward + backward of the reference-style loop on the first B patients: the eager rhs (every past dose re-summed
    per call) stepped by the oracle's torchdiffeq-style midpoint loop."""
    ode, y0 = p["ode"], p["y0"].detach()[:B].clone().requires_grad_(True)
    ode.set_action_static(p["a"][:, :B], None)

    def step():
        h = oracle_odeint(ode, y0, p["t"], method="midpoint", options={"perturb": True, "step_size": 1.0})
        torch.autograd.backward(h, p["cot"][:, :B])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        step()
        torch.cuda.synchronize()
        return event_ms(step, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--t-max", type=int, default=120)
    ap.add_argument("--t0", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--eager-batch", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_dims_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [(D, "libhode_real_dims.so", RD.side_library()) for D in SIZES]
    rows += [(20, "libhode_real_dims.so", RD.side_library()), (20, "libhode.so", hode.lib())]
    probs = [problem(D, args.batch, args.t_max, args.t0, dev, lib) for D, _, lib in rows]
    for p in probs:   # warm-up: allocator, code objects, clocks
        for _ in range(3):
            p["fwd"]()
            p["fwd_bwd"]()
    torch.cuda.synchronize()
    times = [{"fwd": [], "fwd_bwd": []} for _ in rows]
    for _ in range(args.rounds):
        for p, tm in zip(probs, times):
            for k in ("fwd", "fwd_bwd"):
                tm[k].append(event_ms(p[k], args.inner))

    def cell(v):
        return "%8.3f (%7.3f .. %7.3f)" % (statistics.median(v), min(v), max(v))
    ref = times[-1]
    spread = {k: (max(ref[k]) - min(ref[k])) / statistics.median(ref[k]) for k in ref}
    lines = ["# tools/real_dims_probe.py --batch %d --t-max %d --t0 %d --rounds %d --inner %d on %s"
             % (args.batch, args.t_max, args.t0, args.rounds, args.inner, torch.cuda.get_device_name(0)),
             "# midpoint + perturb, hidden %d, %d steps; ms per call through hode.real.real_solve (HIP events): median (min .. max) over"
             % (HIDDEN, args.t_max - args.t0), "# %d rounds of %d back-to-back calls, all rows alternating in one process" % (args.rounds, args.inner),
             "%-4s %-22s %31s %31s" % ("D", "library", "forward ms", "forward + backward ms")]
    for (D, name, _), tm in zip(rows, times):
        lines.append("%-4d %-22s %31s %31s" % (D, name, cell(tm["fwd"]), cell(tm["fwd_bwd"])))
    lines.append("# run-to-run spread of the libhode.so D = 20 row, (max - min) / median: forward %.1f %%, forward + backward %.1f %%"
                 % (100 * spread["fwd"], 100 * spread["fwd_bwd"]))
    for (D, name, _), tm in zip(rows[:-1], times[:-1]):
        for k in ("fwd", "fwd_bwd"):
            excess = statistics.median(tm[k]) / statistics.median(ref[k]) - 1
            lines.append("# D = %-2d %-8s %+6.1f %% against libhode.so D = 20: %s" % (D, k, 100 * excess, "within the spread or faster"
                                                                                   if excess <= spread[k] else "SLOWER than the spread allows"))
    eb = min(args.eager_batch, args.batch)
    p12 = probs[1]
    em = eager_ms(p12, eb)
    km = statistics.median(times[1]["fwd_bwd"]) * eb / args.batch
    lines.append("# reference-style eager loop (RocheODEReal.forward through the torchdiffeq-style loop, autograd backward), D = 12, first %d patients:" % eb)
    lines.append("#   forward + backward %.1f ms (2 calls after one warm-up) against %.3f ms of the kernels scaled to that many patients: %.0fx"
                 % (em, km, em / km))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
