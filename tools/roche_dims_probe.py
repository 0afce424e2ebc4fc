"""Fixed-grid Roche kernels at the latent sizes of libhode_roche_dims.so: a patient per quad (ragged where (D - 4) % 4 != 0)
against one patient per lane, forward and adjoint apart, with libhode.so's D = 8 and 12 forced to the quad layout as
neighbours; and the dopri5 per-attempt time at D = 10 and 16.

    python tools/roche_dims_probe.py [--patients 10000] [--rounds 15] [--inner 20] [--out profiles/roche_dims_probe.txt]

One process, all layouts alternating round by round, device events around `inner` back-to-back calls through the C ABI on
preallocated buffers, medians over the rounds with the min .. max spread; the card is pre-conditioned with untimed calls for
60 ms first (the clock ramps for ~25 ms from idle, profiles/r03_v0_clock_ramp.txt), as bench.py does.  The adjoint's time
is the whole hode_rk_bwd call: gradient clear, kernel, fold.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))

import torch  # noqa: E402

from hode import _lib as L, _roche_dims_lib as RL, adaptive, synth  # noqa: E402
from hode.solver import pack_theta  # noqa: E402
from oracle.rhs import RocheRHS, THETA_NAMES, dose_schedule  # noqa: E402

#: (D, lanes_per_patient, name of the layout): every size of libhode_roche_dims.so in both layouts, then the neighbours
CONFIGS = [(D, lanes, ("quad" if D == 16 else "ragged quad") if lanes == 4 else "lane") for D in RL.DIMS for lanes in (4, 1)] + \
    [(8, 4, "quad (libhode.so)"), (12, 4, "quad (libhode.so)")]


class Call:
    """One (D, layout): the descriptor and its buffers, ready for hode_rk_fwd / hode_rk_bwd."""

    def __init__(self, D, lanes, B, T, dev):
        self.lib = RL.roche_solver_library(D)
        inp = synth.solver_inputs(B, T, D, seed=D)
        torch.manual_seed(D)
        f = RocheRHS(D, synth.STEP)
        dosage, times = dose_schedule(inp["actions"], synth.STEP)
        k = self.keep = dict(
            t=inp["t"].to(dev), y0=inp["z0"].to(dev), dosage=dosage.to(dev), times=times.to(dev).float().contiguous(),
            theta=pack_theta([getattr(f, n).detach() for n in THETA_NAMES], dev).to(dev).contiguous(),
            w=f.ml_net[0].weight.detach().to(dev).contiguous(), b=f.ml_net[0].bias.detach().to(dev).contiguous(),
            h=torch.empty(T, B, D, device=dev), gh=torch.randn(T, B, D, device=dev), gy0=torch.empty(B, D, device=dev),
            gw=torch.empty(D - 4, D, device=dev), gb=torch.empty(D - 4, device=dev), gth=torch.empty(L.N_THETA, device=dev))
        d = self.d = L.new_solve_desc()
        d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.n_dose = L.RHS_ROCHE, L.METHODS["rk4"], B, D, T, times.shape[1]
        d.lanes_per_patient, d.need_theta_grad = lanes, 1
        d.t, d.y0, d.dosage, d.dose_times, d.theta = (k["t"].data_ptr(), k["y0"].data_ptr(), k["dosage"].data_ptr(),
                                                      k["times"].data_ptr(), k["theta"].data_ptr())
        d.w1, d.b1, d.h = k["w"].data_ptr(), k["b"].data_ptr(), k["h"].data_ptr()
        d.grad_h, d.grad_y0 = k["gh"].data_ptr(), k["gy0"].data_ptr()
        d.grad_w1, d.grad_b1, d.grad_theta = k["gw"].data_ptr(), k["gb"].data_ptr(), k["gth"].data_ptr()
        d.flags = L.FLAG_OVERWRITE_GRADS
        n = self.lib.hode_workspace_bytes(d, L.WS_RK_BWD)
        k["ws"] = torch.empty(max(n, 16), device=dev, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = k["ws"].data_ptr(), n
        self.stream = torch.cuda.current_stream().cuda_stream

    def fwd(self):
        self.d.flags = 0
        L.check(self.lib.hode_rk_fwd(self.d, self.stream), "hode_rk_fwd")

    def bwd(self):
        self.d.flags = L.FLAG_OVERWRITE_GRADS
        L.check(self.lib.hode_rk_bwd(self.d, self.stream), "hode_rk_bwd")


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per call


def dopri5_attempt_us(D, B, T, dev, rounds):
    """us per attempted step of the whole forward (host loop included), under no_grad: HODE_FLAG_NO_TAPE."""
    inp = synth.solver_inputs(B, T, D, seed=D)
    torch.manual_seed(D)
    f = RocheRHS(D, synth.STEP)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    args = (inp["z0"].to(dev), pack_theta([getattr(f, n).detach() for n in THETA_NAMES], dev).to(dev),
            f.ml_net[0].weight.detach().to(dev), f.ml_net[0].bias.detach().to(dev), inp["t"].to(dev), dosage.to(dev), times.to(dev))
    out = []
    with torch.no_grad():
        for _ in range(rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            adaptive.roche_dopri5(*args, rtol=1e-7, atol=1e-8, library=RL.roche_solver_library(D))
            torch.cuda.synchronize()
            n = adaptive.last_stats["n_accepted"] + adaptive.last_stats["n_rejected"]
            out.append((time.perf_counter() - t0) * 1e6 / n)
    return out[2:], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=10000)
    ap.add_argument("--times", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roche_dims_probe: needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say("# tools/roche_dims_probe.py --patients %d --times %d --rounds %d --inner %d on %s" % (
        a.patients, a.times, a.rounds, a.inner, torch.cuda.get_device_name(0)))
    say("# rk4, us per call: median (min .. max) over %d rounds of %d back-to-back calls, all layouts alternating in one process" % (a.rounds, a.inner))
    calls = [(D, lanes, name, Call(D, lanes, a.patients, a.times, dev)) for D, lanes, name in CONFIGS]
    for _, _, _, c in calls:
        c.fwd()
        c.bwd()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 60.0:   # clock ramp
        calls[0][3].fwd()
        torch.cuda.synchronize()
    res = {i: ([], []) for i in range(len(calls))}
    for _ in range(a.rounds):
        for i, (_, _, _, c) in enumerate(calls):
            res[i][0].append(timed(c.fwd, a.inner))
            res[i][1].append(timed(c.bwd, a.inner))
    say("%-4s %-5s %-20s %28s %28s" % ("D", "lanes", "layout", "forward us", "adjoint us"))
    for i, (D, lanes, name, _) in enumerate(calls):
        f, b = res[i]
        say("%-4d %-5d %-20s %10.1f (%6.1f .. %6.1f) %10.1f (%6.1f .. %6.1f)" % (
            D, lanes, name, statistics.median(f), min(f), max(f), statistics.median(b), min(b), max(b)))
    say("# dopri5 forward under no_grad, rtol 1e-7, atol 1e-8: us per attempted step (whole call / attempts), median (min .. max)")
    for D in (10, 16):
        us, n = dopri5_attempt_us(D, a.patients, a.times, dev, max(5, a.rounds // 3))
        say("D %-3d %d attempts: %.2f (%.2f .. %.2f)" % (D, n, statistics.median(us), min(us), max(us)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
