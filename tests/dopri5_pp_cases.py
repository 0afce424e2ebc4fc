"""The case table of the per-patient dopri5 kernels (libhode_dopri5_pp.so): every compiled instantiation is named by a case,
tests/test_dopri5_pp_host.py holds the table against the library's kernel symbols and tests/test_hip_dopri5_pp.py runs
every case.  Inputs are hode.synth.solver_inputs and oracle.rhs.RocheRHS, as in tests/test_hip_dopri5.py.  No GPU here.

GRID_CASES puts the same kernels on the non-uniform and offset grids of tests/time_grids.py (synth's grid is uniform, starts
at 0 and has its doses on nodes), AUDIT_CASES are the launches whose step CONTROLLER tests/dopri5_pp_audit.py audits in
float64 at tolerances loose enough for the error estimate to be more than roundoff."""
import copy

import torch

from oracle.rhs import RocheRHS, THETA_DEFAULT

DIMS = (4, 6, 8, 12)
RTOL, ATOL = 1e-7, 1e-8  # the reference's values (model.py:1079-1080)
#: Hill exponents other than 2: the general-pow body of the rhs (values of test_dopri5_owner_layout_kernel_variants)
THETA_GENERAL = (3.0, 1.5, 0.8, 1.3, 0.7, 0.9, 1.1, 0.6, 1.2, 0.5, 1.4, 0.75, 0.65)


def _case(D, B, T, K=1, ablate=False, hill="two", need_theta=True):
    return {"D": D, "B": B, "T": T, "K": K, "ablate": ablate, "hill": hill, "need_theta": need_theta, "seed": 40 + D + B}


#: a covering subset, not the product: B in {1, 3, 21, 70} (70 = one past a whole wave), T 2 .. 20 and T = 1, one and two
#: doses, ablate, general Hill exponents, and every (D, ablate) without the expert-parameter gradient
CASES = [
    _case(12, 70, 20), _case(8, 21, 12, K=2), _case(6, 3, 7), _case(4, 1, 2), _case(12, 1, 9), _case(4, 70, 5, K=2),
    _case(12, 3, 1), _case(6, 21, 1),
    _case(12, 3, 6, ablate=True), _case(8, 21, 5, K=2, ablate=True), _case(6, 1, 8, ablate=True), _case(4, 3, 20, ablate=True),
    _case(8, 3, 6, hill="general"), _case(12, 3, 5, K=2, hill="general"), _case(4, 3, 6, hill="general"),
] + [_case(D, 3, 5, K=1 + (D == 8), ablate=ab, need_theta=False) for D in DIMS for ab in (False, True)]


GRID_T = 12  # tests/time_grids.py: the clustered grid has 12 nodes; the offset grids are cut to as many
GRIDS = ("clustered", "offset+", "offset-")


def _grid_case(grid, D, B, K, ablate=False, hill="two", need_theta=True):
    """A case on a grid of tests/time_grids.py.  Its patients are a slice `first : first + B` of time_grids._roche_inputs'
    77; on the offset grids `first` is chosen so that the replayed patients (subset(B)) hold the dose slot before t[0] and
    the one on t[0] (dose_times: patient p's first dose takes slot p mod 23; slot 22 lies before t[0], slot 0 on it)."""
    first = 0 if grid == "clustered" else {3: 22, 70: 5}[B]
    return dict(_case(D, B, GRID_T, K, ablate, hill, need_theta), grid=grid, first=first)


#: a covering subset again: every D on every grid, B in {1, 3, 70}, one to three doses, and ablate, the general Hill
#: exponents and the sweep without the expert-parameter gradient on every grid.  B = 1 stays on the clustered grid: one
#: patient cannot hold both the dose before t[0] and the dose on it
GRID_CASES = [
    _grid_case("clustered", 12, 70, 3), _grid_case("clustered", 8, 3, 2, ablate=True),
    _grid_case("clustered", 6, 1, 1, hill="general"), _grid_case("clustered", 4, 3, 2, need_theta=False),
    _grid_case("clustered", 12, 3, 1, ablate=True, need_theta=False), _grid_case("clustered", 8, 70, 1),
    _grid_case("offset+", 12, 3, 1, hill="general"), _grid_case("offset+", 8, 70, 2),
    _grid_case("offset+", 6, 3, 3, ablate=True), _grid_case("offset+", 4, 3, 3, need_theta=False),
    _grid_case("offset+", 4, 70, 2, ablate=True),
    _grid_case("offset-", 12, 3, 2, ablate=True), _grid_case("offset-", 8, 3, 3, hill="general"),
    _grid_case("offset-", 6, 70, 1, need_theta=False), _grid_case("offset-", 4, 3, 2),
    _grid_case("offset-", 12, 70, 3, hill="general"),
]


def case_id(c):
    return "%sD%d-B%d-T%d-K%d%s%s%s" % (c["grid"] + "-" if "grid" in c else "", c["D"], c["B"], c["T"], c["K"],
                                         "-ablate" if c["ablate"] else "", "-hill" if c["hill"] == "general" else "",
                                         "" if c["need_theta"] else "-noth")


def _b(x):
    return "true" if x else "false"


def kernels(c):
    """The kernels a forward + backward of this case launches (the partial fold aside)."""
    return {"hode::pp_fwd_kernel<%d, %s>" % (c["D"], _b(c["ablate"])),
            "hode::pp_bwd_kernel<%d, %s, %s>" % (c["D"], _b(c["ablate"]), _b(c["need_theta"]))}


def bodies(c):
    """Which rhs specialisation inside the kernels the case reaches: (Hill exponents == 2, one dose per patient)."""
    hill2 = c["ablate"] or c["hill"] == "two"
    return (hill2, hill2 and c["K"] == 1)


def all_kernels():
    return {"hode::pp_fwd_kernel<%d, %s>" % (D, _b(ab)) for D in DIMS for ab in (False, True)} | \
        {"hode::pp_bwd_kernel<%d, %s, %s>" % (D, _b(ab), _b(th)) for D in DIMS for ab in (False, True) for th in (False, True)}


def setup(c, seed=None):
    """(inputs, rhs) of a case: z0 (B, D), actions (T, B, 1), t (T,); the learned block's weight doubled as in
    tests/test_hip_dopri5.py::_setup so that it matters."""
    if "grid" in c:
        return _grid_setup(c)
    from hode import synth
    seed = c["seed"] if seed is None else seed
    T = max(c["T"], 2)
    inp = synth.solver_inputs(c["B"], T, c["D"], seed=seed, n_dose=c["K"])
    if c["T"] == 1:  # a single output time: nothing to integrate; the dose (at index 0 <= T - 2) stays
        inp = {"z0": inp["z0"], "actions": inp["actions"][:1], "t": inp["t"][:1]}
    torch.manual_seed(seed)
    f = RocheRHS(c["D"], synth.STEP, ablate=c["ablate"], theta=THETA_GENERAL if c["hill"] == "general" else THETA_DEFAULT)
    if c["D"] > 4:
        with torch.no_grad():
            f.ml_net[0].weight.mul_(2.0)
    return inp, f


def _grid_setup(c):
    """(inputs, rhs) of a grid case: time_grids._roche_inputs (state, a quarter of synth's dose amounts, weights, the dose
    times of time_grids.dose_times(inside=True)) sliced to the case's patients.  The inputs carry the dose schedule itself
    ("dosage" (B,), "times" (B, K)) instead of an action tensor: these dose times are no multiples of a step size."""
    import time_grids as tg
    p = tg._roche_inputs(c["D"], c["ablate"], c["K"], c["grid"], c["T"])  # cached and shared: nothing below writes into it
    rows = slice(c["first"], c["first"] + c["B"])
    inp = {"z0": p["y0"][rows].clone(), "t": p["t"].clone(), "dosage": p["dosage"][rows].clone(), "times": p["times"][rows].clone()}
    assert inp["z0"].shape[0] == c["B"]
    f = copy.deepcopy(p["f"])
    if c["hill"] == "general":
        from oracle.rhs import THETA_NAMES
        with torch.no_grad():
            for name, v in zip(THETA_NAMES, THETA_GENERAL):
                getattr(f, name).fill_(v)
    if "stiff" in c:
        inp["z0"][c["stiff"][0]] *= c["stiff"][1]
    return inp, f


def schedule(inp, f):
    """(dosage (B,), dose_times (B, K)) of a case's inputs: their own, or the action tensor's."""
    if "dosage" in inp:
        return inp["dosage"], inp["times"]
    from oracle.rhs import dose_schedule
    return dose_schedule(inp["actions"], f.step_size)


# ------------------------------------------------------------------------------------------------ the controller audit
#: two (rtol, atol) pairs, neither the default, with rtol / atol = 10 and 0.1.  The states are below 0.1: under LOOSE
#: rtol * |y| and atol are of one size for the largest components, under ABS atol decides every component, so
#: swapping rtol and atol changes both
LOOSE, ABS = (1e-4, 1e-5), (3e-5, 3e-4)


def _audit_case(grid, D, K, tol, stiff=None, hill="two"):
    c = dict(_grid_case(grid, D, 70, K, hill=hill), rtol=tol[0], atol=tol[1])
    if stiff is not None:
        c["stiff"] = stiff
    return c


STIFF = 23  # a patient of subset(70) whose start state is scaled up, so that Hairer's first step is rejected

#: the launches whose controller is audited on the patients of subset(70)
AUDIT_CASES = [
    _audit_case("clustered", 4, 1, LOOSE), _audit_case("clustered", 12, 3, ABS, stiff=(STIFF, 1500.0)),
    _audit_case("clustered", 8, 2, LOOSE),
    _audit_case("offset+", 4, 2, LOOSE), _audit_case("offset+", 12, 1, ABS), _audit_case("offset+", 6, 3, LOOSE),
    _audit_case("offset-", 4, 3, LOOSE, stiff=(STIFF, 4000.0)), _audit_case("offset-", 12, 2, ABS),
    _audit_case("offset-", 8, 1, ABS),
]


#: measured, not chosen: the fp32 oracle free-running on the audited patients of AUDIT_CASES, audited as if it were the
#: device (tests/test_dopri5_pp_host.py repeats the measurement and holds it to HEADROOM = 0.5 of the constants).  The
#: factor 8 is the room for the device's powf, div_f32 and fma contraction, a few ulp per operation away from torch's CPU
#: fp32; a safety factor of 0.8 moves every unclamped step by 11 %, half of Hairer's step the first by 50 %, and a wrong
#: norm count or tolerance vector moves the steps by per cent (tests/test_dopri5_pp_host.py: each fails the audit)
MEASURED_RATIO_DIST = 8.78e-5   # largest |ratio32 - ratio64| / max(1, ratio64) over all 770 attempts
#: largest relative distance of an accepted dt from the interval float64 allows it, at HEADROOM of the margin: one step
#: after a roundoff-level ratio whose chain ends 0.07 % below those of the five starts it is followed from; Hairer's first
#: step in fp32 is within 1.1e-5 of float64's
MEASURED_DT_DIST = 6.71e-4
RATIO_MARGIN = 8 * MEASURED_RATIO_DIST
DT_RTOL = 8 * MEASURED_DT_DIST


def audit_id(c):
    return "%s-rtol%g-atol%g%s" % (case_id(c), c["rtol"], c["atol"], "-stiff" if "stiff" in c else "")


def subset(B):
    """The patients whose rows are replayed in float64 (all of them up to 5; else both ends of both waves and one inside)."""
    return list(range(B)) if B <= 5 else sorted({0, B // 3, min(63, B - 2), min(64, B - 1), B - 1})
