#!/usr/bin/env python
"""Time the synthetic data generator on the device and a restatement of the reference's per-patient LSODA loop on this
machine's CPU: `python tools/datagen_probe.py > profiles/datagen_probe.txt`.  HIP events, warm clock (the timed calls
follow untimed ones of the same shape), median of the repeats."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"), os.path.join(ROOT, "tests")]

import datagen_eager as eager  # noqa: E402
from hode import datagen  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X
SHAPES = ((2100, 14, 12, 80, 5), (10000, 100, 12, 80, 5), (1000000, 14, 12, 80, 3))   # N, t_max, D, obs, repeats
LSODA_SAMPLE = 24


def flops_per_step(D):
    """fp64 operations of one attempted step as the kernel forms it: six right-hand sides (the D x (D - 4) product as
    fma = 2, about 25 for the expert block, tanh and exp counted as one), the stage sums, the error norm."""
    M = D - 4
    rhs = 2 * D * M + M + 25
    stage_sums = 2 * D * (1 + 2 + 3 + 4 + 5 + 5) + 2 * 6 * D
    return 6 * rhs + stage_sums + 2 * 6 * D + 6 * D


def inputs(N, D, obs, t_max, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(2)
    init = torch.empty(N, D, device=dev, dtype=torch.float64).exponential_(100.0, generator=g)
    times = torch.randint(0, t_max, (N, 1), device=dev, generator=g).double()
    amount = torch.rand(N, device=dev, dtype=torch.float64, generator=g) * 10
    ml = rng.standard_normal((D, D - 4)) * rng.binomial(1, 0.5, (D, D - 4)) / D
    oc = rng.standard_normal((obs, D + 1)) * rng.binomial(1, 0.25, (obs, D + 1))
    return init, times, amount, ml, oc


def lsoda_seconds_per_patient(init, times, amount, ml, t_max):
    import scipy.integrate
    t0 = time.perf_counter()
    for n in range(init.shape[0]):
        f = eager.make_rhs(eager.THETA, ml, np.zeros(0), 0.0)
        kel, tau, amt = eager.THETA[12], times[n], amount[n]

        def rhs(t, y):
            out = f(t, y)
            out[3] += kel * amt * np.sum(np.exp(kel * (tau - t) * (t >= tau)) * (t >= tau))
            return out
        ode = scipy.integrate.ode(rhs).set_integrator("lsoda")
        ode.set_initial_value(init[n], 0)
        while ode.successful() and ode.t < t_max:
            ode.integrate(ode.t + 1.0)
    return (time.perf_counter() - t0) / init.shape[0]


def main():
    dev = torch.device("cuda:0")
    print("device: %s; CPU: %s, 1 of %d cores used by the LSODA loop" % (
        torch.cuda.get_device_name(0), next((l.split(":")[1].strip() for l in open("/proc/cpuinfo") if "model name" in l), "?"),
        os.cpu_count()))
    for N, t_max, D, obs, reps in SHAPES:
        init, times, amount, ml, oc = inputs(N, D, obs, t_max, dev)
        call = lambda **kw: datagen.simulate(init, times, amount, eager.THETA, torch.as_tensor(ml).to(dev), torch.as_tensor(oc).to(dev),
                                             0.2, t_max, 1.0, 0.5, 7, **kw)
        out = call(return_steps=True)
        steps = out["steps"].double()
        failed = int((out["status"] != 0).sum())
        del out
        call()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        t = float(np.median(ms)) * 1e-3
        T = t_max + 1
        written = T * N * (2 * obs + D + 1) * 4
        flops = float(steps.sum()) * flops_per_step(D)
        k = min(LSODA_SAMPLE, N)
        per = lsoda_seconds_per_patient(init[:k].cpu().numpy(), times[:k, 0].cpu().numpy(), amount[:k].cpu().numpy(), ml, t_max)
        print("N %8d  T %3d  D %2d  obs %3d: simulate %9.3f ms (median of %d, min %.3f)  steps/patient mean %.1f max %d  failed %d"
              % (N, T, D, obs, t * 1e3, reps, min(ms), steps.mean().item(), int(steps.max().item()), failed))
        print("    written %.1f MB -> %.1f GB/s = %.2f %% of HBM peak;  %.2f Tflop/s fp64 executed;  LSODA loop %.2f ms/patient on %d"
              " patients -> %.1f s for this shape on one core (x %.0f)"
              % (written / 1e6, written / t / 1e9, 100 * written / t / HBM_PEAK, flops / t / 1e12, per * 1e3, k, per * N, per * N / t))


if __name__ == "__main__":
    main()
