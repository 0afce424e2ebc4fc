"""Timing of the fused neural dopri5 (solve + adjoint) at the bench shape, next to rk4 on the same rhs.

    python tools/neural_dopri5_probe.py [latent size ...]      (default: 12)

Every latent size given is timed in the same process, one after the other: `14 15` puts the largest size libhode.so
serves next to the largest of libhode_neural_odd.so (hidden tiles HT 9 : 10)."""
import sys, os, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))
from hode import adaptive, synth
from hode.neural import neural_solve
from oracle.rhs import NeuralRHS, dose_schedule
dev = torch.device("cuda:0")
N, T = 10000, 100


def probe(D):
    inp = synth.solver_inputs(N, T, D)
    torch.manual_seed(0)
    f = NeuralRHS(D, synth.STEP)
    prm = [p.detach().clone().to(dev).requires_grad_(True) for p in (f.ml_net[0].weight, f.ml_net[0].bias, f.ml_net[2].weight, f.ml_net[2].bias)]
    y0 = inp["z0"].to(dev).requires_grad_(True)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    dosage, times, t = dosage.to(dev), times.to(dev), inp["t"].to(dev)
    cot = torch.randn(T, N, D, device=dev)

    def run(fn, iters=5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        fw, bw = [], []
        for i in range(iters + 1):
            y0.grad = None
            for q in prm: q.grad = None
            ev[0].record(); h = fn(); ev[1].record(); (h * cot).sum().backward(); ev[2].record()
            torch.cuda.synchronize()
            if i: fw.append(ev[0].elapsed_time(ev[1])); bw.append(ev[1].elapsed_time(ev[2]))
        return sum(fw) / len(fw), sum(bw) / len(bw)

    print("D = %d (N = %d, T = %d, hidden tiles %d)" % (D, N, T, (10 * D + 15) // 16))
    for rtol in (1e-7, 1e-5):
        fwd, bwd = run(lambda: adaptive.neural_dopri5(y0, *prm, t, dosage, times, rtol=rtol, atol=1e-8))
        st = adaptive.last_stats
        print("  dopri5 rtol %g: fwd %.2f ms (%d + %d attempts, %.2f us each), bwd %.2f ms (%.2f us per accepted step)" % (
            rtol, fwd, st["n_accepted"], st["n_rejected"], fwd * 1e3 / (st["n_accepted"] + st["n_rejected"]), bwd, bwd * 1e3 / st["n_accepted"]))
    fwd, bwd = run(lambda: neural_solve(y0, *prm, t, dosage, times, method="rk4"))
    print("  rk4: fwd %.2f ms, bwd (weight gradients on chip) %.2f ms" % (fwd, bwd))


if __name__ == "__main__":
    for D in [int(a) for a in sys.argv[1:]] or [12]:
        probe(D)
