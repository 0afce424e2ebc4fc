"""The GPU cases of libhode_neural_odd.so (tests/test_hip_neural_odd.py runs them, tests/test_neural_odd_host.py checks
that they reach every kernel the library's objects contain), their inputs and their float64 references.  A plain helper
module: no tests here.

Fixed grid: every odd size x three methods at N = 17 (one full 16-patient wave and one lane of the next), T = 6, on
hode.synth's inputs with z0 * 30; one more case with perturb, one with a dose on a stage time (the midpoint of a grid
step: t0 + dt / 2 is exact in fp32 and fp64 on the dyadic grid).  dopri5: D = 5 (fewest hidden tiles, ragged last one) and
D = 15 (most) at N in {1, 17} with the replay checks, the other sizes once at N = 17.  All of these are on synth's uniform
0.125 grid from 0; two different step sizes in one call, a start at t[0] != 0 and, for dopri5, several output times inside
one accepted step are tests/time_grids.py's neural_odd and neural_odd_dopri5 families (tests/test_hip_time_grids.py)."""
import copy
import functools

import torch

import kernel_variants as kv

DIMS = (5, 7, 9, 11, 13, 15)
N, T_FIXED, T_DOPRI5 = 17, 6, 14
RTOL, ATOL = 1e-6, 1e-8

FIXED_CASES = [dict(D=D, method=m, perturb=False, dose="grid") for D in DIMS for m in ("euler", "midpoint", "rk4")]
FIXED_CASES += [dict(D=15, method="rk4", perturb=True, dose="grid"), dict(D=15, method="midpoint", perturb=False, dose="stage")]
DOPRI5_FULL = [dict(D=D, N=n) for D in (5, 15) for n in (1, 17)]          # free-running oracle + both replays
DOPRI5_ONCE = [dict(D=D, N=N) for D in (7, 9, 11, 13)]                      # free-running oracle


def fixed_id(c):
    return "D%d-%s%s%s" % (c["D"], c["method"], "-perturb" if c["perturb"] else "", "-stage-dose" if c["dose"] == "stage" else "")


def dopri5_id(c):
    return "D%d-N%d" % (c["D"], c["N"])


def kernels_reached():
    """Every kernel the cases above launch, by the dispatch rules tests/kernel_variants.py restates for libhode.so (the side
    library's launchers follow the same ones, on-chip backward only; every dopri5 case accepts steps and runs attached)."""
    out = set()
    for c in FIXED_CASES:
        out.update(kv.neural_fixed(c["D"], kv.METHODS[c["method"]], 0, True))
    for c in DOPRI5_FULL + DOPRI5_ONCE:
        out.update(kv.neural_dopri5_kernels(c["D"], 1, False))
    return out


def expected_kernels():
    """sizes x (ndp_fwd phases 0..2, ndp_bwd, ndp_initbwd 1 and 2, neural_mf_fwd x 3 methods, neural_mf_bwd<.., true> x 3,
    neural_grad_fold), written out independently of kernels_reached()."""
    out = set()
    for D in DIMS:
        out.update("hode::ndp_fwd_kernel<%d, %d>" % (D, ph) for ph in (0, 1, 2))
        out.update(["hode::ndp_bwd_kernel<%d>" % D, "hode::ndp_initbwd_kernel<%d, 1>" % D, "hode::ndp_initbwd_kernel<%d, 2>" % D,
                    "hode::neural_grad_fold_kernel<%d>" % D])
        out.update("hode::neural_mf_fwd_kernel<%d, %d>" % (D, m) for m in (0, 1, 2))
        out.update("hode::neural_mf_bwd_kernel<%d, %d, true>" % (D, m) for m in (0, 1, 2))
    return out


# ------------------------------------------------------------------------------------------------------ fixed grid
@functools.lru_cache(maxsize=None)
def fixed_problem(D, dose="grid", n=N, T=T_FIXED):
    """dict(f, t, y0, dosage, times, cot): an fp32 oracle.rhs.NeuralRHS and the tensors the kernels read."""
    from hode import synth
    from oracle.rhs import NeuralRHS, dose_schedule
    inp = synth.solver_inputs(n, T, D, seed=D)
    torch.manual_seed(D)
    f = NeuralRHS(D, synth.STEP)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    times = times.to(torch.float32).reshape(n, -1).clone()
    if dose == "stage":
        times[:, 0] = times[:, 0] + 0.5 * synth.STEP   # the midpoint stage of the grid step that starts at the dose's grid point
        assert torch.equal(times.double(), (times.double() / (synth.STEP / 2)).round() * (synth.STEP / 2))
    cot = torch.randn(T, n, D, generator=torch.Generator().manual_seed(1))
    return dict(f=f, t=inp["t"], y0=inp["z0"] * 30.0, dosage=dosage.to(torch.float32), times=times, cot=cot)


@functools.lru_cache(maxsize=None)
def fixed_reference(D, method, perturb, dose="grid", n=N, T=T_FIXED):
    """oracle.solvers.odeint on the problem's values in float64: h and the gradients of sum(h * cot)."""
    from oracle.solvers import odeint as oracle_odeint
    p = fixed_problem(D, dose, n, T)
    f64 = copy.deepcopy(p["f"]).double()
    f64.dosage, f64.times = p["dosage"].double(), p["times"].double()
    y64 = p["y0"].double().requires_grad_(True)
    h = oracle_odeint(f64, y64, p["t"].double(), method=method, options={"perturb": perturb})
    (h * p["cot"].double()).sum().backward()
    net = f64.ml_net
    g = [q.grad if q.grad is not None else torch.zeros_like(q) for q in (net[0].weight, net[0].bias, net[2].weight, net[2].bias)]
    return dict(h=h.detach(), gy0=y64.grad, gw1=g[0], gb1=g[1], gw2=g[2], gb2=g[3])


GRADS = ("gy0", "gw1", "gb1", "gw2", "gb2")


def params(f, dev, dtype=torch.float32):
    net = f.ml_net
    return [x.detach().clone().to(dev, dtype).requires_grad_(True) for x in (net[0].weight, net[0].bias, net[2].weight, net[2].bias)]


def rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
