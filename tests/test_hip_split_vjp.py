"""The split adjoint's stage VJP at D = 12, rk4, lanes_per_patient = 48, against the float64 oracle.  GPU only.

The learned waves form v = W_LL^T u from per-lane partial products over their OWN two rows of W_LL (the weights held rotated
per quad lane) and a two-round reduce-scatter over the quad, and the cotangent algebra between the stage VJPs keeps one fma on
the chain (csrc/hode_rk_split.hip).  What can go wrong there and nowhere else:

* the seams of the layout: a workgroup holds 48 patients, a learned wave 16, so N = 1, 17, 47, 49, 101 put the batch's end inside
  a wave, one short of a workgroup, one past it, and inside the third; T = 2 .. 9 covers every residue of the loops unrolled by
  two and by three and the prologue's special cases;
* a mis-rotated weight: with a dense W_LL a wrong entry averages into the rel-L2, so the placement cases give W_LL exactly one
  non-zero per row, at column (i + k) mod 8 with eight distinct magnitudes: over k = 0 .. 7 every (i, j) is exercised once and a
  swapped entry is a wrong component of grad_y0 and a missing entry of grad_w;
* tape against tape-less: both builds share the VJP and must agree bit for bit.

Helpers, reference and bound are those of tests/test_hip_kernel_variants.py: oracle.solvers.odeint on oracle.rhs in fp64 on the
fp32 inputs, gradients rel-L2 <= GRAD_TOL."""
import functools

import pytest
import torch

import kernel_variants as kv
import time_grids as tg
from test_hip_kernel_variants import _dev, _grad_ok, _rel, _roche_plan, _roche_setup, _theta_names

pytestmark = pytest.mark.gpu

D, METHOD, LANES = 12, "rk4", 48
SEAMS = ((1, 2), (17, 3), (47, 4), (49, 5), (101, 9))
GRID_CASE = dict(family="roche", D=D, lanes=LANES, method=METHOD, ablate=False, need_theta=True, tape=True, perturb=False,
                 n_dose=1, grid="offset+", T=6)
WLL_MAGNITUDES = (0.9, -1.3, 0.6, 1.7, -0.8, 1.1, -1.5, 0.7)  # one per row of W_LL, pairwise different in size


def placement_wll(k):
    """W_LL (8 x 8) with exactly one non-zero per row: row i holds WLL_MAGNITUDES[i] at column (i + k) mod 8."""
    w = torch.zeros(D - 4, D - 4)
    for i in range(D - 4):
        w[i, (i + k) % (D - 4)] = WLL_MAGNITUDES[i]
    return w


@functools.lru_cache(maxsize=None)
def _problem(N, T, k=None):
    """Inputs of one case as _roche_plan takes them and their fp64 gradients (shared by the tape and tape-less runs)."""
    from oracle.rhs import dose_schedule
    inp, f = _roche_setup(D, False, N, T, seed=700 + N + 31 * T + (0 if k is None else 1 + k))
    if k is not None:
        with torch.no_grad():
            f.ml_net[0].weight[:, 4:] = placement_wll(k)  # the expert columns stay random
    dosage, times = dose_schedule(inp["actions"], f.step_size)
    cot = torch.randn(T, N, D, generator=torch.Generator().manual_seed(N + T))
    theta = torch.stack([getattr(f, n).detach().reshape(()) for n in _theta_names(False)])
    p = dict(y0=inp["z0"], t=inp["t"], dosage=dosage, times=times, theta=theta, w=f.ml_net[0].weight.detach(),
             b=f.ml_net[0].bias.detach(), cot=cot, f=f)
    ref = tg.roche_solve_cpu(p, METHOD, False, False)
    for name, v in ref.items():
        assert torch.isfinite(v).all(), name
    return p, ref


def _run(p, tape, perturb=False):
    assert kv.roche_layout(D, LANES, p["t"].numel()) == "split"
    return _roche_plan(p, _dev(), METHOD, False, LANES, True, tape, perturb=perturb)


def _check(got, ref, keys, record_property, tag):
    for k in keys:
        record_property("err_%s_%s" % (k, tag), _grad_ok(k, got[k], ref[k]))


@pytest.mark.parametrize("N,T", SEAMS, ids=["N%d_T%d" % s for s in SEAMS])
def test_seams_against_fp64_and_tape_against_tapeless(N, T, record_property):
    p, ref = _problem(N, T)
    got = {tape: _run(p, tape) for tape in (True, False)}
    for tape in (True, False):
        _check(got[tape], ref, ("gy0", "gw", "gb", "gth"), record_property, "tape" if tape else "notape")
    for k in got[True]:
        assert torch.equal(got[True][k], got[False][k]), (k, _rel(got[True][k], got[False][k]))


def test_placement_cases_cover_every_entry_of_wll_once():
    seen = sum((placement_wll(k) != 0).int() for k in range(D - 4))
    assert torch.equal(seen, torch.ones(D - 4, D - 4, dtype=torch.int32))
    assert len({abs(m) for m in WLL_MAGNITUDES}) == D - 4


@pytest.mark.parametrize("k", range(D - 4))
def test_rotated_weight_placement(k, record_property):
    p, ref = _problem(5, 2, k)
    assert torch.equal(p["w"][:, 4:], placement_wll(k))
    assert float(ref["gw"][:, 4:].abs().min()) > 0  # every entry of grad W_LL carries signal: u_i Y_j is dense
    for tape in (True, False):
        _check(_run(p, tape), ref, ("gy0", "gw"), record_property, "tape" if tape else "notape")


def test_offset_nonuniform_grid(record_property):
    p, ref = tg.roche_inputs(GRID_CASE), tg.roche_ref(GRID_CASE)
    dts = {round(float(x), 6) for x in p["t"][1:] - p["t"][:-1]}
    assert float(p["t"][0]) != 0.0 and len(dts) == GRID_CASE["T"] - 1
    got = {tape: _run(p, tape) for tape in (True, False)}
    for tape in (True, False):
        _check(got[tape], ref, ("gy0", "gw", "gb", "gth"), record_property, "tape" if tape else "notape")
    for k in got[True]:
        assert torch.equal(got[True][k], got[False][k]), (k, _rel(got[True][k], got[False][k]))
