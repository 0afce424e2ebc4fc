"""The one-step-ahead solve of the real-data hybrid rhs (hode.real_step, libhode_real_step.so) at config 5's shape -- D 20,
hidden 43, T 120 (119 intervals), midpoint + perturb -- forward + backward through autograd, against
    (a) the same result composed from T - 1 chained real_solve calls of two grid points each (what the kernels before this
        library could do), and
    (b) one chained real_solve over the same grid (the same arithmetic volume, serialised over T - 1 steps),
with a sweep of C, the consecutive intervals one wave owns.

    python tools/real_step_solve_probe.py [B ...]        (default 2097 8192)

Every variant is warmed up, then timed alternately with the others over ROUNDS rounds of REPS calls; the median round is
printed (ms per forward + backward, host clock around a device synchronise).  (tools/real_step_probe.py is an older tool
of another subject: the time of a whole config 5 training step.)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))
import torch  # noqa: E402

from hode import _lib as L, _real_step_lib as RS  # noqa: E402
from hode.real import real_solve  # noqa: E402
from hode.real_step import real_step_solve  # noqa: E402

D, H, T, TA = 20, 43, 120, 120
ROUNDS, REPS = 5, 4
C_SWEEP = (1, 2, 3, 4, 6, 8, 12, 14, 17, 20, 30, 40, 60, 119)


def problem(B, dev):
    g = torch.Generator().manual_seed(B)
    M = D - 4
    q = dict(wflat=(torch.randn(9 * H + 2 + 3 * M * M, generator=g) * 0.2).to(dev).requires_grad_(True),
             theta=torch.tensor([1.0, 0.2, 0.2], device=dev).requires_grad_(True),
             act=((torch.rand(TA, B, generator=g) < 0.1).float() * torch.rand(TA, B, generator=g)).to(dev),
             t=torch.arange(0.0, float(T), device=dev),
             init=(torch.randn(T - 1, B, D, generator=g) * 0.3).to(dev).requires_grad_(True),
             cot=torch.randn(T, B, D, generator=g).to(dev))
    q["pairs"] = [q["t"][i:i + 2].clone() for i in range(T - 1)]
    return q


def run(fn, q):
    for k in ("wflat", "theta", "init"):
        q[k].grad = None
    fn(q)


def step_call(C):
    def fn(q):
        h = real_step_solve(q["init"], q["theta"], q["wflat"], q["t"], q["act"], H, intervals_per_wave=C)
        (h * q["cot"]).sum().backward()
    return fn


def composed(q):   # (a)
    ends = [real_solve(q["init"][i], q["theta"], q["wflat"], q["pairs"][i], q["act"], H)[1] for i in range(T - 1)]
    h = torch.stack([torch.zeros_like(ends[0])] + ends)
    (h * q["cot"]).sum().backward()


def chained(q):    # (b)
    h = real_solve(q["init"][0], q["theta"], q["wflat"], q["t"], q["act"], H)
    (h * q["cot"]).sum().backward()


def main():
    dev = torch.device("cuda:0")
    for B in [int(v) for v in sys.argv[1:]] or [2097, 8192]:
        q = problem(B, dev)
        d = L.new_solve_desc()
        d.rhs_kind, d.batch, d.latent_dim, d.hidden_dim, d.n_action_times = L.RHS_ROCHE_REAL, B, D, H, TA
        chosen = RS.step_library(T - 1, 1, 0).chosen_intervals_per_wave(d)
        variants = [("step C=%d" % c, step_call(c)) for c in C_SWEEP] + [("step default (C=%d)" % chosen, step_call(0)),
                                                                            ("(a) %d real_solve calls" % (T - 1), composed),
                                                                            ("(b) chained real_solve", chained)]
        for _, fn in variants:
            run(fn, q)
            run(fn, q)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(ROUNDS):
            for name, fn in variants:   # alternating: a drift of the machine hits every variant alike
                reps = 1 if name.startswith("(a)") else REPS
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    run(fn, q)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / reps * 1e3)
        print("B = %d, D %d, hidden %d, %d intervals, midpoint: ms per forward + backward (median of %d rounds; min .. max)"
              % (B, D, H, T - 1, ROUNDS))
        for name, _ in variants:
            v = times[name]
            waves = ""
            if name.startswith("step C="):
                c = int(name.split("=")[1])
                waves = "   %6d waves" % (-(-B // 16) * -(-(T - 1) // c))
            print("  %-28s %9.3f   (%.3f .. %.3f)%s" % (name, statistics.median(v), min(v), max(v), waves), flush=True)


if __name__ == "__main__":
    main()
