#!/usr/bin/env python
"""dopri5 step control on the device: the same problems through

    batch    hode.adaptive.roche_dopri5: torchdiffeq's controller, one error norm and one dt for the whole batch, one
             launch per attempted step (the default; its adjoint run with detach_first_step, the semantics of the other side)
    patient  model._RochePatientDopri5 (hode.patient_dopri5): a controller per patient, the whole solve in one launch, the
             sweep over the per-patient tapes in a second one

at the benchmark shape (10 000 patients, T 100, D 12), at the scripts' batch (50) and at evaluate()'s ensemble (2 500 x 50
draws, forward only under no_grad), rtol 1e-7, atol 1e-8 (the reference's), inputs as bench.py's solver problem.  The two
are timed in alternating repeats in one call, HIP events around each step; every line gives the median and the spread
(min .. max) and says whether the ranges overlap.  Each shape is warmed up first.  Next to the times: the accepted /
rejected steps of the batch-global controller and the per-patient counts (min, median, max).

    python tools/patient_dopri5_probe.py [--reps 7] [--out profiles/patient_dopri5_probe.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import model  # noqa: E402
from hode import adaptive, patient_dopri5, synth  # noqa: E402

DEV = torch.device("cuda:0")
RTOL, ATOL = 1e-7, 1e-8
#: (name, patients, T, D, with the backward)
SHAPES = (("bench", 10000, 100, 12, True), ("script_batch", 50, 100, 12, True), ("evaluate_2500x50", 125000, 100, 12, False))


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def problem(N, T, D):
    inp = synth.solver_inputs(N, T, D, seed=synth.SEED)
    w, b = synth.default_ml_weights(D)
    theta = torch.tensor((2.0, 2.0) + (1.0,) * 11 + (0.0,) * 3)
    chan = inp["actions"][..., 0]
    times = (torch.nonzero((chan != 0).t())[:, 1].reshape(N, -1) * synth.STEP).float()
    cot = torch.randn(T, N, D, generator=torch.Generator().manual_seed(99))
    return {k: v.to(DEV) for k, v in {"y0": inp["z0"], "t": inp["t"], "w": w, "b": b, "theta": theta, "dosage": chan.max(dim=0)[0],
                                      "times": times, "cot": cot}.items()}


def solve(control, p, y0, w, b):
    if control == "batch":
        return adaptive.roche_dopri5(y0, p["theta"], w, b, p["t"], p["dosage"], p["times"], rtol=RTOL, atol=ATOL, detach_first_step=True)
    return model._RochePatientDopri5.apply(y0, p["theta"], w, b, p["t"], p["dosage"], p["times"], RTOL, ATOL, False,
                                           torch.is_grad_enabled())


def forward_only(control, p):
    with torch.no_grad():
        solve(control, p, p["y0"], p["w"], p["b"])


def forward_backward(control, p):
    y0, w, b = (p[k].detach().requires_grad_(True) for k in ("y0", "w", "b"))
    (solve(control, p, y0, w, b) * p["cot"]).sum().backward()


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "n": len(ts)}


def spread(v):
    v = sorted(v.tolist())
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1], "total": sum(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    lines, res = [], {}
    for name, N, T, D, with_bwd in SHAPES:
        p = problem(N, T, D)
        modes = {"fwd": forward_only} if not with_bwd else {"fwd": forward_only, "fwd_bwd": forward_backward}
        for fn in modes.values():  # warm-up: code objects, allocator
            for control in ("batch", "patient"):
                fn(control, p)
        forward_only("batch", p)
        counts = {"batch": {"accepted": adaptive.last_stats["n_accepted"], "rejected": adaptive.last_stats["n_rejected"]}}
        forward_only("patient", p)
        st = patient_dopri5.last_stats
        counts["patient"] = {"accepted": spread(st["n_accepted"].cpu()), "rejected": spread(st["n_rejected"].cpu())}
        res[name] = {"patients": N, "T": T, "D": D, "steps": counts}
        lines.append("%s (%d x %d x %d): batch-global controller %d accepted / %d rejected; per patient accepted %s, rejected %s"
                     % (name, N, T, D, counts["batch"]["accepted"], counts["batch"]["rejected"],
                        counts["patient"]["accepted"], counts["patient"]["rejected"]))
        print(lines[-1], flush=True)
        for mode, fn in modes.items():
            ts = {"batch": [], "patient": []}
            for _ in range(a.reps):
                for control in ("batch", "patient"):
                    ts[control].append(event_time(lambda: fn(control, p)))
            bt, pt = stats(ts["batch"]), stats(ts["patient"])
            res[name][mode] = {"batch": bt, "patient": pt}
            apart = pt["max_ms"] < bt["min_ms"] or bt["max_ms"] < pt["min_ms"]
            lines.append("%s %s: batch %.3f ms (%.3f .. %.3f, n %d) | patient %.3f ms (%.3f .. %.3f, n %d): %s"
                         % (name, mode, bt["median_ms"], bt["min_ms"], bt["max_ms"], bt["n"], pt["median_ms"], pt["min_ms"],
                            pt["max_ms"], pt["n"],
                            "batch / patient = x%.2f, the ranges do not overlap" % (bt["median_ms"] / pt["median_ms"]) if apart
                            else "THE RANGES OVERLAP: no difference beyond the spread"))
            print(lines[-1], flush=True)
    lines.append(json.dumps(res))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
