"""The case table of the failure-reporting and patient-isolation tests: every fixed-grid Roche forward (rk_fwd_kernel,
split_fwd_kernel, mf_fwd_kernel of libhode.so and rk_fwd_kernel of libhode_roche_dims.so) at small shapes with one patient
poisoned.  tests/test_failure_cases.py (CPU) holds the table against the built kernel symbols and pins what a poisoned run
must give with oracle.solvers.odeint in float64; tests/test_hip_failures.py (GPU) runs it.  A plain helper module.

The cases are tests/kernel_variants.py's Roche entries (and one per compiled forward of tests/roche_dims_cases.py) with what selects
the instantiation and the rhs body kept -- D, method, ablate, lanes, tape, theta / Hill exponents, dose count -- and the
shape shrunk: T = 6 (and the no-step / one-step edges 1 and 2), B = 50 = 48 + 2 (a second, ragged block of the split layout,
a ragged fourth wave of the 16-patients-per-wave layout) and B = 5.  The poisoned row (0, 47, 48, B - 1), column (an expert
column, the dose column, the first and last learned column), value (NaN, +inf, -inf) and the output time that carries the
poisoned cotangent (0, T // 2, T - 1) rotate through the table as tests/dose_cases.py's axes do; no full product."""
import copy
import functools

import torch

import dose_cases
import kernel_variants as kv
import roche_dims_cases as rdc

T_MAIN, T_EDGES = 6, (1, 2)
BATCHES = (50, 5)
ROWS = (0, 47, 48)                      # and B - 1
EXPERT_COL, DOSE_COL = 1, 3
VALUES = (float("nan"), float("inf"), float("-inf"))
VALUE_NAMES = {"nan": VALUES[0], "+inf": VALUES[1], "-inf": VALUES[2]}
FAMILIES = ("rk_fwd_kernel", "split_fwd_kernel", "mf_fwd_kernel")
#: the keys of a kernel_variants case that select the forward's instantiation and rhs body (need_theta selects the
#: backward's only: every case here runs the adjoint with need_theta_grad on)
KEPT = ("D", "lanes", "method", "ablate", "tape", "theta", "hill", "n_dose", "neg_imm")
#: (T, B) of the cases beside each instantiation's first one, which keeps (T_MAIN, 50)
_SHAPES = ((6, 5), (2, 50), (6, 50), (1, 50), (2, 5), (6, 50), (1, 5))
#: the quiet patients of the false-positive batch (B >= 5): y0 all zeros, y0 all 1e-40 (subnormal), every dose after t[-1]
ZERO_ROW, TINY_ROW, LATE_ROW = 1, 2, 3
TINY = 1e-40


def rows(B):
    return tuple(r for r in ROWS if r < B - 1) + (B - 1,)


def cols(D):
    return (EXPERT_COL, DOSE_COL) + ((4, D - 1) if D > 4 else ())


def _launches_a_forward(c):
    return any(kv.family(k) in FAMILIES for k in kv.kernels(c))


def _fixed_cases():
    seen, base = set(), []
    for c in kv.CASES:
        if c["family"] != "roche" or not _launches_a_forward(c):
            continue
        key = tuple(c.get(k) for k in KEPT)
        if key not in seen:
            seen.add(key)
            base.append(dict({k: c[k] for k in KEPT if k in c}, lib="libhode"))
    # libhode_roche_dims.so: one case per compiled forward (size x layout x method x rhs), the rhs body rotating through them
    i = 0
    for D in rdc.DIMS:
        for lanes in rdc.LANES:
            for method in rdc.METHODS:
                for ablate in (False, True):
                    held = [x for x in rdc.FIXED_CASES if (x["D"], x["lanes"], x["method"], x["ablate"]) == (D, lanes, method, ablate)
                            and x["need_theta"]]
                    c = held[i % len(held)]
                    base.append(dict({k: c[k] for k in KEPT if k in c}, tape=False, lib="roche_dims"))  # no layout there keeps a tape
                    i += 1
    out, first = [], set()
    for i, c in enumerate(base):
        inst = (c["lib"], c["D"], c["lanes"], c["method"], c["ablate"], c["tape"])
        T, B = (T_MAIN, 50) if inst not in first else _SHAPES[i % len(_SHAPES)]
        first.add(inst)
        r, cl = rows(B), cols(c["D"])
        out.append(dict(c, T=T, B=B, row=r[i % len(r)], col=cl[(i // 2 + i) % len(cl)], value=tuple(VALUE_NAMES)[(i // 3 + i) % 3],
                        n=(0, T // 2, T - 1)[i % 3], seed=300 + i))
    # two patients per wave in the lane-per-patient layout
    out.append(dict(D=4, lanes=1, method="rk4", ablate=False, tape=True, theta="default", n_dose=1, lib="libhode", T=2,
                    B=dose_cases.TWO_PER_WAVE, row=dose_cases.TWO_PER_WAVE - 1, col=DOSE_COL, value="nan", n=1, seed=299))
    return out


def case_id(c):
    s = "%s-D%d-l%d-%s%s%s-%s%s-K%d-T%d-B%d-p%d.%d=%s-n%d" % (
        c["lib"], c["D"], c["lanes"], c["method"], "-ablate" if c["ablate"] else "", "" if c["tape"] else "-notape", c["theta"],
        ":" + c["hill"] if c.get("hill") else "", c["n_dose"], c["T"], c["B"], c["row"], c["col"], c["value"], c["n"])
    return s + ("-negimm" if c.get("neg_imm") else "")


def forward_kernel(c):
    """The forward kernel hode_rk_fwd launches for the case (csrc/hode_api.hip use_split / use_mf / choose_lpp,
    csrc/roche_dims/hode_roche_dims.hip rk_lpp).  The split forward runs at T = 1 too (only its backward needs a step);
    it writes a tape when the caller hands one (HODE_FLAG_TAPE: a backward follows, T >= 2) and the method has stages."""
    D, m, a = c["D"], kv.METHODS[c["method"]], kv._b(c["ablate"])
    if c["lib"] == "roche_dims":
        return "hode::rk_fwd_kernel<%d, %d, %d, %s>" % (D, rdc.rk_lpp(D, c["lanes"], c["B"]), m, a)
    if D in (8, 12) and c["lanes"] in (0, 48):
        return "hode::split_fwd_kernel<%d, %d, %s, %s>" % (D, m, a, kv._b(c["tape"] and m != kv.EULER and c["T"] >= 2))
    if D in (8, 12, 16) and c["lanes"] == 16:
        return "hode::mf_fwd_kernel<%d, %d, %s>" % (D, m, a)
    return "hode::rk_fwd_kernel<%d, %d, %d, %s>" % (D, kv.choose_lpp(D, c["lanes"], c["B"]), m, a)


def layout(c):
    return kv.family(forward_kernel(c)).split("_")[0]  # "rk" / "split" / "mf"


def has_both_backwards(c):
    """The split layout has a taped and a recomputing backward (euler has no stage to tape: one backward)."""
    return layout(c) == "split" and c["method"] != "euler" and c["T"] >= 2


CASES = _fixed_cases()
BY_ID = {case_id(c): c for c in CASES}
#: compiled forwards no call reaches (name -> reason): kernel_variants' own list, the forwards of it
UNREACHABLE = {k: v for k, v in kv.UNREACHABLE.items() if kv.family(k) in FAMILIES}

#: the NeuralODE fixed-grid kernels have no status word: isolation only.  Both layouts tests/test_hip_neural.py
#: parametrizes; the lane-per-patient kernels are compiled for D = 6, 8, 12 only, so that layout runs at its own smallest
#: and largest size instead of 4 and 14
NEURAL_CASES = [dict(D=D, layout=lay, method=method, B=50, T=6, row=row, col=col, value=value, n=n)
                for D, lay, method, row, col, value, n in (
                    (4, "matrix-cores", "rk4", 0, 0, "nan", 5), (14, "matrix-cores", "midpoint", 47, 13, "+inf", 3),
                    (14, "matrix-cores", "euler", 48, 4, "-inf", 1), (4, "matrix-cores", "midpoint", 49, 3, "nan", 3),
                    (6, "lane-per-patient", "rk4", 49, 5, "nan", 3), (12, "lane-per-patient", "midpoint", 0, 0, "+inf", 5),
                    (12, "lane-per-patient", "euler", 47, 11, "nan", 1), (6, "lane-per-patient", "midpoint", 48, 2, "-inf", 5),
                    # the cotangent of t[0]: it enters after the last step of the sweep
                    (14, "matrix-cores", "rk4", 48, 7, "nan", 0), (12, "lane-per-patient", "rk4", 49, 6, "+inf", 0))]


def neural_case_id(c):
    return "D%d-%s-%s-p%d.%d=%s-n%d" % (c["D"], c["layout"], c["method"], c["row"], c["col"], c["value"], c["n"])


# --------------------------------------------------------------------------------------------------------- inputs
def roche_problem(D, B, T, seed, ablate=False, theta=kv.THETA_DEFAULT, K=1, neg_imm=False):
    """Inputs of a Roche solve as the kernels read them: y0 (B, D), t (T,), dosage (B,), times (B, K), theta (16,), w, b,
    a cotangent cot (T, B, D) and the oracle rhs f (the dose schedule not yet set)."""
    from hode import synth
    from oracle.rhs import RocheRHS, dose_schedule
    # synth places K distinct doses on the nodes 0 .. Tg - 2: a grid shorter than that keeps its first T nodes
    inp = synth.solver_inputs(B, max(T, K + 1, 2), D, seed=seed, n_dose=K)
    if K > 1:
        inp["actions"] /= K  # K decays of the patient's largest dose kept at one dose's scale (tests/test_hip_kernel_variants.py)
    if neg_imm:
        inp["z0"][::2, 2] = -0.05 - inp["z0"][::2, 2]
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    torch.manual_seed(seed)
    f = RocheRHS(D, synth.STEP, ablate=ablate, theta=theta)
    if D > 4:
        with torch.no_grad():
            f.ml_net[0].weight.mul_(2.0)  # larger weights than default init so that the learned block matters
    names = dose_cases.theta_names(ablate)
    th = torch.zeros(16)
    th[:len(names)] = torch.stack([getattr(f, n).detach().reshape(()) for n in names])
    return dict(y0=inp["z0"], t=inp["t"][:T].clone(), dosage=dosage.clone(), times=times.to(torch.float32).reshape(B, K).clone(),
                theta=th, w=f.ml_net[0].weight.detach() if D > 4 else None, b=f.ml_net[0].bias.detach() if D > 4 else None,
                cot=torch.randn(T, B, D, generator=torch.Generator().manual_seed(seed + 1)), f=f)


def neural_problem(D, B, T, seed):
    """Inputs of a NeuralODE solve (tests/test_hip_neural.py's: z0 scaled by 30): y0, t, dosage, times, the four weights
    prm, a cotangent cot and the oracle rhs f with its dose schedule set."""
    from hode import synth
    from oracle.rhs import NeuralRHS, dose_schedule
    inp = synth.solver_inputs(B, max(T, 2), D, seed=seed)
    torch.manual_seed(seed)
    f = NeuralRHS(D, synth.STEP)
    f.set_action(inp["actions"])
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    prm = [p.detach().clone() for p in (f.ml_net[0].weight, f.ml_net[0].bias, f.ml_net[2].weight, f.ml_net[2].bias)]
    return dict(y0=inp["z0"] * 30.0, t=inp["t"][:T].clone(), dosage=dosage, times=times.to(torch.float32).reshape(B, 1), prm=prm,
                cot=torch.randn(T, B, D, generator=torch.Generator().manual_seed(seed + 1)), f=f)


@functools.lru_cache(maxsize=None)
def _setup(cid):
    c = BY_ID[cid]
    return roche_problem(c["D"], c["B"], c["T"], c["seed"], c["ablate"], kv.theta_of(c), c["n_dose"], bool(c.get("neg_imm")))


# ------------------------------------------------------------------------------- dt underflow of the dopri5 controllers
#: Finite start states on which the controller gives up on dt before it takes a step (tests/test_failure_cases.py fixes
#: them with tests/adaptive_eager.py in float32; tests/test_hip_failures.py runs them on the kernels).
#: "overflow": y0[0, 0] = 3e38 -- the Roche rhs' first derivative overflows fp32, d1 = inf, h0 = 0.01 d0 / d1 = 0 and dt_0 = 0.
#: "tolerance": rtol = 1e-30, atol = 0 -- (y0 / scale)^2 overflows, d0 = d1 = inf, h0 = inf / inf = NaN and dt_0 is NaN or 0.
#: Either way `t0 + dt > t0` fails at the first attempt: torchdiffeq's "underflow in dt".
UNDERFLOW_CASES = [dict(family="roche", D=8, lanes=1, how="overflow"), dict(family="roche", D=8, lanes=4, how="overflow"),
                   dict(family="roche", D=12, lanes=4, how="tolerance"), dict(family="roche", D=4, lanes=1, how="tolerance"),
                   dict(family="neural", D=8, lanes=0, how="tolerance"), dict(family="neural", D=14, lanes=0, how="tolerance")]
UNDERFLOW_B, UNDERFLOW_T = 5, 6


def underflow_id(c):
    return "%s-D%d-l%d-%s" % (c["family"], c["D"], c["lanes"], c["how"])


def underflow_problem(c):
    """(problem, rtol, atol) of an UNDERFLOW_CASES entry."""
    p = (roche_problem if c["family"] == "roche" else neural_problem)(c["D"], UNDERFLOW_B, UNDERFLOW_T, seed=500 + c["D"])
    if c["how"] == "overflow":
        p["y0"] = p["y0"].clone()
        p["y0"][0, 0] = 3e38
        return p, 1e-7, 1e-8
    return p, 1e-30, 0.0


def setup(c):
    """The clean inputs of a case, computed once and shared (nothing may write into them): y0 (B, D), t (T,), dosage (B,),
    times (B, K), theta (16,), w, b, the cotangent cot (T, B, D) and the oracle rhs f."""
    return _setup(case_id(c))


def poisoned_y0(c, y0=None):
    y0 = (setup(c)["y0"] if y0 is None else y0).clone()
    y0[c["row"], c["col"]] = VALUE_NAMES[c["value"]]
    return y0


def poisoned_cot(c, cot=None):
    cot = (setup(c)["cot"] if cot is None else cot).clone()
    cot[c["n"], c["row"], c["col"]] = VALUE_NAMES[c["value"]]
    return cot


def quiet(c):
    """The false-positive batch: the case's inputs with a patient whose y0 is all zeros, one whose y0 is all 1e-40 and one
    all of whose doses lie after t[-1].  (y0, times); B >= 5."""
    p = setup(c)
    y0, times = p["y0"].clone(), p["times"].clone()
    y0[ZERO_ROW], y0[TINY_ROW] = 0.0, TINY
    if c["n_dose"]:
        times[LATE_ROW] = float(p["t"][-1]) + 0.25 + 0.125 * torch.arange(c["n_dose"], dtype=torch.float32)
    return y0, times


def _odeint64(c, y0, times):
    from oracle.solvers import odeint as oracle_odeint
    p = setup(c)
    f = copy.deepcopy(p["f"]).double()
    f.dosage, f.times = p["dosage"].double(), times.double()
    with torch.no_grad():
        return oracle_odeint(f, y0.double(), p["t"].double(), method=c["method"])


@functools.lru_cache(maxsize=None)
def _oracle(cid, which):
    c = BY_ID[cid]
    p = setup(c)
    if which == "quiet":
        return _odeint64(c, *quiet(c))
    return _odeint64(c, poisoned_y0(c) if which == "poisoned" else p["y0"], p["times"])


def oracle(c, which="clean"):
    """h (T, B, D) of oracle.solvers.odeint in float64 on the case's "clean", "poisoned" or "quiet" inputs, once per case."""
    return _oracle(case_id(c), which)
