"""Guard (no GPU) of tests/failure_cases.py, the table tests/test_hip_failures.py runs: every compiled forward of the three
fixed-grid Roche families, in libhode.so and in libhode_roche_dims.so, is named by a failure case or by a listed reason; and
the expected answer of every poisoned run is pinned to oracle.solvers.odeint in float64, not to the kernels: the final state
is non-finite in exactly the poisoned patient, every other patient is bit-equal to the clean run, and the quiet patients of
the false-positive batch (y0 = 0, y0 = 1e-40, every dose after t[-1]) stay finite."""
import pytest
import torch

import build_hip
import failure_cases as fc
import kernel_variants as kv
import roche_dims_cases as rdc
from test_kernel_variant_coverage import compiled_kernel_names


@pytest.mark.parametrize("lib", ["libhode", "roche_dims"])
def test_every_compiled_forward_is_named_by_a_failure_case(lib):
    """Both libraries: every `.kd` symbol of the three families is the forward of a case, or listed with its reason."""
    row = build_hip.LIBRARIES["libhode.so" if lib == "libhode" else "libhode_roche_dims.so"]
    compiled = {n for n in compiled_kernel_names(row.obj) if kv.family(n) in fc.FAMILIES}
    named = {fc.forward_kernel(c) for c in fc.CASES if c["lib"] == lib}
    unreachable = set(fc.UNREACHABLE) if lib == "libhode" else set()
    assert named <= compiled, sorted(named - compiled)
    assert unreachable <= compiled and not unreachable & named
    missing = sorted(compiled - named - unreachable)
    assert not missing, "%d compiled forwards no failure case names:\n  %s" % (len(missing), "\n  ".join(missing))
    if lib == "roche_dims":
        want = {k for k in rdc.expected_kernels() if kv.family(k) in fc.FAMILIES}
        assert compiled == want and len(compiled) == len(rdc.DIMS) * 2 * 3 * 2  # size x layout (1, 4 lanes) x method x rhs
    else:
        assert {kv.family(n) for n in compiled} == set(fc.FAMILIES)


def test_every_instantiation_body_pair_of_libhode_is_named():
    pairs = {(fc.forward_kernel(c), kv.roche_body(c["ablate"], *kv.theta_of(c)[:2], c["n_dose"])) for c in fc.CASES if c["lib"] == "libhode"}
    names = {n for n, _ in pairs}
    assert {(n, b) for n in names for b in kv.bodies(n)} == pairs


def test_the_table_is_well_formed():
    ids = [fc.case_id(c) for c in fc.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 300
    shapes = {(c["T"], c["B"]) for c in fc.CASES}
    assert {t for t, _ in shapes} == {1, 2, 6} and {b for _, b in shapes} == {5, 50, 1027}
    by_layout = {}
    for c in fc.CASES:
        assert c["row"] in fc.rows(c["B"]) and c["col"] in fc.cols(c["D"]) and c["n"] in (0, c["T"] // 2, c["T"] - 1), c
        by_layout.setdefault(fc.layout(c) + ("-dims-l%d" % c["lanes"] if c["lib"] == "roche_dims" else ""), []).append(c)
    assert set(by_layout) == {"rk", "split", "mf", "rk-dims-l1", "rk-dims-l4"}
    for lay, cs in by_layout.items():  # every axis value reaches every layout, the shape edges included
        big = [c for c in cs if c["B"] == 50]
        assert {c["row"] for c in big} == {0, 47, 48, 49}, lay
        assert {c["value"] for c in cs} == set(fc.VALUE_NAMES), lay
        assert {c["col"] for c in cs if c["D"] > 4} >= {1, 3, 4}, lay
        assert any(c["col"] == c["D"] - 1 for c in cs if c["D"] > 4), lay
        if "dims" not in lay:  # tests/test_hip_roche_dims.py runs the edge shapes of that library (EDGE_SHAPES)
            assert {c["T"] for c in cs} == {1, 2, 6} and {c["B"] for c in cs} >= {5, 50}, lay
    assert any(c["B"] == 1027 and c["lanes"] == 1 and c["D"] == 4 and c["T"] == 2 for c in fc.CASES)
    # the first case of every instantiation keeps the full shape
    full = {fc.forward_kernel(c) for c in fc.CASES if (c["T"], c["B"]) == (6, 50)}
    assert {fc.forward_kernel(c) for c in fc.CASES if c["B"] != 1027} <= full | {fc.forward_kernel(c) for c in fc.CASES if c["T"] == 1}
    assert {fc.forward_kernel(c) for c in fc.CASES if c["T"] >= 2 and c["B"] != 1027} <= full
    for c in fc.NEURAL_CASES:
        assert c["row"] in fc.rows(c["B"]) and 0 <= c["col"] < c["D"]
    assert {c["layout"] for c in fc.NEURAL_CASES if c["n"] == 0} == {"matrix-cores", "lane-per-patient"}
    assert {(c["D"], c["layout"]) for c in fc.NEURAL_CASES} == {(4, "matrix-cores"), (14, "matrix-cores"), (6, "lane-per-patient"),
                                                               (12, "lane-per-patient")}


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_float64_oracle_on_the_poisoned_inputs(c):
    clean, bad = fc.oracle(c, "clean"), fc.oracle(c, "poisoned")
    p = c["row"]
    assert bool(torch.isfinite(clean).all())
    finite_rows = torch.isfinite(bad[-1]).all(dim=-1)
    want = torch.ones(c["B"], dtype=torch.bool)
    want[p] = False
    assert torch.equal(finite_rows, want), (~finite_rows).nonzero().flatten().tolist()
    others = want.nonzero().flatten()
    assert torch.equal(bad[:, others], clean[:, others])
    # no non-finite value appears and is gone again: a patient whose final state is finite is finite at every output time
    assert bool(torch.isfinite(bad[:, others]).all())
    if c["B"] >= 5:
        quiet = fc.oracle(c, "quiet")
        assert bool(torch.isfinite(quiet).all())


@pytest.mark.parametrize("c", fc.UNDERFLOW_CASES, ids=fc.underflow_id)
def test_the_underflow_constructions_end_in_dt_underflow_in_the_eager_restatement(c):
    """tests/adaptive_eager.py (torchdiffeq's semantics written out) in float32 on each construction: a finite start state,
    and the controller gives up on dt -- "underflow in dt" or "non-finite error ratio", both torchdiffeq's "underflow in dt
    nan" -- within 200 attempts, without ever flagging the state."""
    import warnings

    import adaptive_eager
    import hode
    p, rtol, atol = fc.underflow_problem(c)
    assert p["y0"].dtype == torch.float32 and bool(torch.isfinite(p["y0"]).all())
    f = p["f"]
    if c["family"] == "roche":
        f.dosage, f.times = p["dosage"], p["times"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's inf / inf
        with pytest.raises(hode.HodeError, match="underflow in dt|non-finite error ratio"):
            adaptive_eager.odeint_dopri5(f, p["y0"], p["t"], rtol=rtol, atol=atol, max_num_steps=200)
