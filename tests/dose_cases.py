"""The case table of the dose-gradient adjoint kernels (libhode_dose.so): every compiled instantiation is named by a case,
tests/test_dose_host.py holds the table against the library's kernel symbols and the oracle's own fp32 error, and
tests/test_hip_dose.py runs every case.  The reference of every number is oracle.rhs.RocheRHS in float64 under
oracle.solvers.odeint with `dosage` a leaf.  No GPU here.

Every non-ablate case with B >= 5 carries a patient whose dosage is 0 (ZERO: row B - 2; its gradient is not 0) and a
patient all of whose doses lie after t[-1] (LATE: row B - 1; its gradient is exactly 0)."""
import functools

import numpy as np
import torch

from oracle.rhs import RocheRHS, THETA_DEFAULT

DIMS = (4, 6, 8, 12)
METHODS = ("euler", "midpoint", "rk4")  # HODE_METHOD_EULER, _MIDPOINT, _RK4_38 = 0, 1, 2
#: Hill exponents 3 and 1.5: the general-pow body of the rhs (values of tests/dopri5_pp_cases.py)
THETA_GENERAL = (3.0, 1.5, 0.8, 1.3, 0.7, 0.9, 1.1, 0.6, 1.2, 0.5, 1.4, 0.75, 0.65)
BATCHES = (5, 63, 64, 65, 130)
DOSES = (1, 2, 3)
#: patients_per_wave(B, 1) is 1 up to B = 1024 (a wave per patient until every SIMD has one): the smallest batch at which a
#: wave holds two patients and the last wave is partly filled
TWO_PER_WAVE = 1027


def _case(D, method, B, T, K=1, ablate=False, hill="two", need_theta=True, perturb=False, grid="uniform", edge=False):
    return {"D": D, "method": method, "B": B, "T": T, "K": K, "ablate": ablate, "hill": "two" if ablate else hill,
            "need_theta": need_theta, "perturb": perturb, "grid": grid, "edge": edge, "seed": 70 + D + B}


def _product():
    """One case per compiled kernel, the other axes rotated through it (T = 1 takes no step: it is among the extra cases)."""
    out, i = [], 0
    for D in DIMS:
        for method in METHODS:
            for ablate in (False, True):
                for need_theta in (True, False):
                    out.append(_case(D, method, BATCHES[i % 5], (9, 2, 9)[(i // 4 + i) % 3], DOSES[(i // 3 + i) % 3], ablate,
                                     "general" if i % 4 == 1 else "two", need_theta, perturb=(i % 6 == 2)))
                    i += 1
    return out


CASES = _product() + [
    # every (T, K) with the one-dose fast path, the dose-list body and the general body at the largest size
    _case(12, "rk4", 130, 9, 1), _case(12, "rk4", 65, 9, 3), _case(12, "rk4", 5, 9, 2, hill="general"),
    _case(8, "midpoint", 64, 9, 1, hill="general"), _case(6, "euler", 63, 2, 3, hill="general"),
    # a single output time: no step, every gradient but gy0 = grad_h[0] is 0
    _case(4, "rk4", 5, 1, 1), _case(12, "midpoint", 63, 1, 2), _case(8, "euler", 64, 1, 3, ablate=True),
    _case(6, "rk4", 65, 1, 1, hill="general", need_theta=False),
    _case(8, "rk4", 65, 9, 2, perturb=True), _case(12, "midpoint", 5, 9, 1, perturb=True), _case(6, "euler", 64, 9, 2, perturb=True),
    # non-uniform and offset grids of tests/time_grids.py, doses inside steps, on nodes and before t[0]
    _case(12, "rk4", 65, 9, 3, grid="offset+", hill="general"), _case(6, "midpoint", 63, 9, 2, grid="offset-", perturb=True),
    _case(8, "euler", 5, 12, 1, grid="clustered"),
    # across the clustered grid's gap of 1.25 rk4's extrapolated last stage has a negative ImmuneReact for 9 of the 130
    # patients, in float64 too, where the log in d ir ** HillPatho / d HillPatho is NaN in the oracle as well: the sweep
    # without the expert gradient (every other gradient is finite and held)
    _case(4, "rk4", 130, 12, 2, grid="clustered", need_theta=False),
    _case(8, "rk4", 64, 9, 1, grid="offset-", ablate=True),
    # a dose time equal to a grid time and to a stage time, and one ulp either side
    _case(4, "rk4", 16, 9, 1, edge=True), _case(8, "midpoint", 16, 9, 1, edge=True), _case(12, "rk4", 16, 9, 2, edge=True),
    _case(6, "euler", 16, 9, 1, edge=True), _case(6, "midpoint", 16, 9, 3, edge=True, hill="general"),
    # two patients per wave
    _case(4, "rk4", TWO_PER_WAVE, 2, 1), _case(6, "midpoint", TWO_PER_WAVE, 2, 2, need_theta=False),
]


def case_id(c):
    return "D%d-%s-B%d-T%d-K%d%s%s%s%s%s%s" % (c["D"], c["method"], c["B"], c["T"], c["K"], "-ablate" if c["ablate"] else "",
                                               "-hill" if c["hill"] == "general" else "", "" if c["need_theta"] else "-noth",
                                               "-perturb" if c["perturb"] else "", "" if c["grid"] == "uniform" else "-" + c["grid"],
                                               "-edge" if c["edge"] else "")


def _b(x):
    return "true" if x else "false"


def kernel(c):
    """The sweep kernel a backward of this case launches (the partial fold aside)."""
    return "hode::dose_bwd_kernel<%d, %d, %s, %s>" % (c["D"], METHODS.index(c["method"]), _b(c["ablate"]), _b(c["need_theta"]))


def all_kernels():
    return {"hode::dose_bwd_kernel<%d, %d, %s, %s>" % (D, m, _b(ab), _b(th))
            for D in DIMS for m in range(3) for ab in (False, True) for th in (False, True)}


def body(c):
    """Which rhs specialisation inside the kernel the case reaches: (Hill exponents == 2, one dose per patient)."""
    hill2 = c["ablate"] or c["hill"] == "two"
    return (hill2, hill2 and c["K"] == 1)


def zero_row(c):
    return c["B"] - 2 if c["B"] >= 5 else None


def late_row(c):
    return c["B"] - 1 if c["B"] >= 5 else None


def theta_names(ablate):
    from oracle.rhs import THETA_NAMES
    return list(THETA_NAMES) + (["theta_1", "theta_2"] if ablate else [])


def _ulp(x, up):
    return float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))


def edge_times(t, method):
    """Dose times on and one fp32 ulp either side of the times at which step 3 and its neighbour evaluate the rhs: the
    grid node t[3] (the first stage of step 3; with rk4 the last stage of step 2 as well) and midpoint's half step, both
    exact in fp32 and in float64, so `t >= tau` falls alike in both even at equality; and one ulp either side of rk4's
    third-step stages, which fp32 and float64 round differently by less than half an ulp (equality there would not be the
    same comparison in the reference)."""
    import time_grids as tg
    t0 = float(t[3])
    out = [t0, _ulp(t0, True), _ulp(t0, False)]
    stages = tg.stage_times32(t.numpy(), method, False)[3]
    if method == "midpoint":
        out += [float(stages[1]), _ulp(stages[1], True), _ulp(stages[1], False)]
    elif method == "rk4":
        out += [_ulp(stages[1], True), _ulp(stages[1], False), _ulp(stages[2], True), _ulp(stages[2], False)]
    return out


@functools.lru_cache(maxsize=None)
def _setup(cid):
    c = BY_ID[cid]
    from hode import synth
    from oracle.rhs import dose_schedule
    B, D, T, K = c["B"], c["D"], c["T"], c["K"]
    # synth places K distinct doses on the nodes 0 .. Tg - 2: a grid shorter than that keeps its first T nodes (a dose past
    # t[-1] then adds nothing)
    inp = synth.solver_inputs(B, max(T, K + 1, 2), D, seed=c["seed"], n_dose=K)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    dosage = dosage / K  # K decays of the patient's largest dose: kept at one dose's scale (tests/test_hip_kernel_variants.py)
    t = inp["t"][:T].clone()
    if c["grid"] != "uniform":
        import time_grids as tg
        t = tg.grid(c["grid"], T)
        times = tg.dose_times(tg.grid64(c["grid"], T), c["grid"], B, K, inside=True)
        dosage = dosage * 0.25  # the largest step is three times synth's 0.125 (tests/time_grids.py::_roche_inputs)
    times = times.to(torch.float32).reshape(B, K).clone()
    dosage = dosage.clone()
    if c["edge"]:
        edges = edge_times(t, c["method"])
        assert len(edges) < B - 2
        times[:len(edges), 0] = torch.tensor(edges, dtype=torch.float32)
    if zero_row(c) is not None:
        dosage[zero_row(c)] = 0.0
        times[late_row(c)] = float(t[-1]) + 0.25 + 0.125 * torch.arange(K, dtype=torch.float32)
    torch.manual_seed(c["seed"])
    f = RocheRHS(D, synth.STEP, ablate=c["ablate"], theta=THETA_GENERAL if c["hill"] == "general" else THETA_DEFAULT)
    if D > 4:
        with torch.no_grad():
            f.ml_net[0].weight.mul_(2.0)  # larger weights than default init so that the learned block matters
    theta = torch.stack([getattr(f, n).detach().reshape(()) for n in theta_names(c["ablate"])])
    cot = torch.randn(T, B, D, generator=torch.Generator().manual_seed(c["seed"] + 1))
    return dict(y0=inp["z0"], t=t, dosage=dosage, times=times, theta=theta, cot=cot, f=f,
                w=f.ml_net[0].weight.detach() if D > 4 else None, b=f.ml_net[0].bias.detach() if D > 4 else None)


def setup(c):
    """Inputs of a case, computed once and shared: y0 (B, D), t (T,), dosage (B,), times (B, K), theta, w, b, the cotangent
    cot (T, B, D) of h and the oracle rhs f.  Nothing may write into them."""
    return _setup(case_id(c))


@functools.lru_cache(maxsize=None)
def _oracle(cid, dtype):
    import copy
    from oracle.solvers import odeint as oracle_odeint
    c = BY_ID[cid]
    p = _setup(cid)
    f = copy.deepcopy(p["f"]).to(dtype)
    dosage = p["dosage"].to(dtype).clone().requires_grad_(True)
    f.dosage, f.times = dosage, p["times"].to(dtype)
    y = p["y0"].to(dtype).clone().requires_grad_(True)
    h = oracle_odeint(f, y, p["t"].to(dtype), method=c["method"], options={"perturb": c["perturb"]})
    (h * p["cot"].to(dtype)).sum().backward()
    zero = torch.zeros((), dtype=dtype)
    ref = dict(h=h.detach(), gy0=y.grad, gdosage=dosage.grad if dosage.grad is not None else torch.zeros_like(dosage),
               gth=torch.stack([getattr(f, n).grad if getattr(f, n).grad is not None else zero for n in theta_names(c["ablate"])]))
    if c["D"] > 4:
        lin = f.ml_net[0]  # a single output time: the rhs is never called and autograd leaves None
        ref["gw"] = lin.weight.grad if lin.weight.grad is not None else torch.zeros_like(lin.weight)
        ref["gb"] = lin.bias.grad if lin.bias.grad is not None else torch.zeros_like(lin.bias)
    return ref


def oracle(c, dtype=torch.float64):
    """h and the gradients of sum(h * cot) with respect to y0, dosage, theta, w, b by the oracle in `dtype`, once per case."""
    return _oracle(case_id(c), dtype)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


BY_ID = {case_id(c): c for c in CASES}
