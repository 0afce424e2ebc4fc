"""The case table of the per-patient dopri5 kernels (libhode_dopri5_pp.so): every compiled instantiation is named by a case,
tests/test_dopri5_pp_host.py holds the table against the library's kernel symbols and tests/test_hip_dopri5_pp.py runs
every case.  Inputs are hode.synth.solver_inputs and oracle.rhs.RocheRHS, as in tests/test_hip_dopri5.py.  No GPU here."""
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


def case_id(c):
    return "D%d-B%d-T%d-K%d%s%s%s" % (c["D"], c["B"], c["T"], c["K"], "-ablate" if c["ablate"] else "",
                                       "-hill" if c["hill"] == "general" else "", "" if c["need_theta"] else "-noth")


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


def subset(B):
    """The patients whose rows are replayed in float64 (all of them up to 5; else both ends of both waves and one inside)."""
    return list(range(B)) if B <= 5 else sorted({0, B // 3, min(63, B - 2), min(64, B - 1), B - 1})
