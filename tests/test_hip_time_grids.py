"""Every solver kernel that takes a time grid on non-uniform and offset grids, against the float64 oracle.  GPU only.

One test per entry of tests/time_grids.py's CASES (tests/test_time_grid_cases.py checks the table on the CPU: exact grids,
fp32 / fp64 stage times on the same side of every dose time, inputs that tell a neighbour's dt from the right one, the fp32
oracle within half of every bound).  Every other GPU file feeds the kernels a uniform grid from 0 or an integer, where dt is
one number and the step size or stage time of step n +- 1 gives the right answer.

The side libraries that serve the ragged latent sizes are separately compiled instantiations and have families of their own:
real_dims (libhode_real_dims.so), real_step (libhode_real_step.so: per-interval rows of the (N, S + 1) grid table, a clipped
last sub-step, bit-identity with the chained kernels at S = 1 and across run lengths) and neural_odd / neural_odd_dopri5
(libhode_neural_odd.so).  Each of their tests asserts which library served the call.

Helpers, references and tolerances are those of tests/test_hip_kernel_variants.py: oracle.solvers.odeint on oracle.rhs in
fp64 on the fp32 inputs, the fp64 tape replay for dopri5, tests/neural_real_eager.py; trajectory _traj_ok, gradients
rel-L2 1e-4 (2e-4 for the real-data neural ODEs), grad_theta per component, h[0] == y0 bit for bit."""
import copy

import pytest
import torch

import kernel_variants as kv
import time_grids as tg
from reference_checks import NEURAL_DOPRI5_TRAJ_TOL, NEURAL_REAL_GRAD_TOL
from test_hip_kernel_variants import (NEURAL_GRADS, _dev, _dp_gpu, _grad_ok, _neural_gpu, _neural_gpu_tape_backward, _neural_real,
                                      _real_gpu, _real_gpu_tape_backward, _rel, _roche_plan, _roche_setup, _same_as_with_theta,
                                      _tape_same_as_onchip, _theta_components_ok, _traj_ok)

pytestmark = pytest.mark.gpu


def _err_h(h, ref):
    return (h.double().cpu() - ref).abs().max().item() / (1 + ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------- Roche fixed grid
@pytest.mark.parametrize("case", tg.family("roche"), ids=tg.case_id)
def test_roche_time_grid(case, record_property):
    """rk_* (lanes 1 / 4), split_* (lanes 48 / 0) and mf_* (lanes 16) on the ragged and offset grids, doses on nodes, inside
    steps and before t[0]; need_theta=False against need_theta=True and, on the split layout, tape against no tape as
    test_roche_fixed_grid and test_hip_rk hold them."""
    dev = _dev()
    D, method, ablate, lanes = case["D"], case["method"], case["ablate"], case["lanes"]
    p, ref = tg.roche_inputs(case), tg.roche_ref(case)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    got = _roche_plan(p, dev, method, ablate, lanes, case["need_theta"], case["tape"], perturb=case["perturb"])
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in ("gy0", "gw", "gb", "gth"):
        if k in got:
            record_property("err_" + k, _grad_ok(k, got[k], ref[k]))
    if "gth" in got:
        record_property("err_gth_comp", _theta_components_ok(got["gth"], ref["gth"]))
    split = kv.roche_layout(D, lanes, case["T"]) == "split"
    if not case["need_theta"]:
        with_th = _roche_plan(p, dev, method, ablate, lanes, True, case["tape"], perturb=case["perturb"])
        assert torch.equal(got["h"], with_th["h"])
        for k in ("gy0", "gw", "gb"):
            if k in got:
                _same_as_with_theta(got[k], with_th[k], split or ablate, k)
    if split:
        # the backward with the stage tape reads the numbers the tape-less one recomputes, in the same order: bit-identical
        # (test_hip_rk.test_split_tape_matches_recompute holds the uniform grid to the same)
        other = _roche_plan(p, dev, method, ablate, lanes, case["need_theta"], not case["tape"], perturb=case["perturb"])
        for k in got:
            assert torch.equal(got[k], other[k]), ("tape", k, _rel(got[k], other[k]))


# ------------------------------------------------------------------------------------------------- NeuralODE fixed grid
@pytest.mark.parametrize("case", tg.family("neural"), ids=tg.case_id)
def test_neural_time_grid(case, record_property):
    dev = _dev()
    method, perturb = case["method"], case["perturb"]
    p = tg.neural_inputs(case)
    ref = tg.neural_solve_cpu(p, method, perturb)
    tape = not case["onchip"] and case["layout"] == "mf"
    got = _neural_gpu_tape_backward(p, method, perturb, dev) if tape \
        else _neural_gpu(p, method, perturb, dev, kv.neural_lanes(case))
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in NEURAL_GRADS:
        err = _rel(got[k], ref[k]) if float(ref[k].abs().max()) > 0 else float(got[k].abs().max())
        record_property("err_" + k, err)
        assert err <= 1e-4, (k, err)
    if tape:
        _tape_same_as_onchip(got, _neural_gpu(p, method, perturb, dev), method, record_property)


# --------------------------------------------------------------------------------------------------------------- dopri5
def _tape_covers(case, tape, t):
    """From the kernel's own tape: on the clustered grid an accepted step covered >= 3 output times and >= 2 covered none."""
    counts = [hi - lo for lo, hi in tape["j"]]  # first / one-past-last output index interpolated inside each accepted step
    assert sum(counts) == len(t) - 1, counts
    if case["grid"] == "clustered":
        assert max(counts) >= 3 and sum(1 for n in counts if n == 0) >= 2, counts
    return counts


@pytest.mark.parametrize("case", tg.family("dopri5"), ids=tg.case_id)
def test_dopri5_time_grid(case, record_property):
    """dp_fwd_kernel's dense-output loop with several output times in one accepted step and none in others (clustered), and
    the whole solve from t[0] = 2.5 (offset+: every dose is already decaying), against the fp64 replay of the kernel's own
    tape; bounds as test_dopri5_backward."""
    from hode import adaptive
    from test_hip_dopri5 import _replay
    dev = _dev()
    D, ablate, T = case["D"], case["ablate"], case["T"]
    t = tg.grid(case["grid"], T)
    inp, f = _roche_setup(D, ablate, kv.DOPRI5_N, T, seed=40 + D + 5 * ablate, n_dose=case["n_dose"], t=t)
    inp["cot"] = torch.randn(T, kv.DOPRI5_N, D, generator=torch.Generator().manual_seed(3))
    adaptive.keep_workspace = True
    try:
        got, tape = _dp_gpu(inp, f, dev, case["lanes"], case["need_theta"], case["detach"])
        other, _ = _dp_gpu(inp, f, dev, case["lanes"], not case["need_theta"], case["detach"])
    finally:
        adaptive.keep_workspace = False
    assert len(tape["t"]) > 1 and tape["t"][0] == float(t[0])
    record_property("outputs_per_step_max", max(_tape_covers(case, tape, t)))
    assert torch.equal(got["h"][0], inp["z0"])
    first = (not case["detach"]) and bool(tape["init"]["first_accepted"])
    ref = _replay(inp, f, 1e-7, 1e-8, inp["cot"], tape, first, double=True)
    for k, v in ref.items():
        if k != "sigma":
            assert torch.isfinite(v).all(), k
    ref32 = _replay(inp, f, 1e-7, 1e-8, inp["cot"], tape, first) if first else None
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    with_th = got if case["need_theta"] else other
    for k in ("gy0", "gw", "gb", "gth"):
        if k not in with_th:
            continue
        g = got[k] if k in got else with_th[k]
        rk = ref["gtheta" if k == "gth" else k]
        tol = max(1e-4, 2.0 * _rel(ref32["gtheta" if k == "gth" else k], rk)) if first else 1e-4
        record_property("err_" + k, _grad_ok(k, g, rk, tol))
        if k != "gth":
            _same_as_with_theta(got[k], other[k], False, k)
    floor = 2.0 * (ref32["gtheta"] - ref["gtheta"]).abs() if first else None
    record_property("err_gth_comp", _theta_components_ok(with_th["gth"], ref["gtheta"], floor))


@pytest.mark.parametrize("case", tg.family("neural_dopri5"), ids=tg.case_id)
def test_neural_dopri5_time_grid(case, record_property):
    """ndp_* on the clustered and offset+ grids against oracle.solvers.odeint_dopri5_replay in fp64 along the run's own tape
    (test_neural_dopri5's bounds)."""
    _neural_dopri5_on_grid(case, record_property)


def _neural_dopri5_on_grid(case, record_property):
    from hode import adaptive
    from oracle.solvers import odeint_dopri5_replay
    from test_hip_neural import _neural_case, _neural_hip_dopri5
    dev = _dev()
    D, B, T = case["D"], case["B"], case["T"]
    rtol, atol = 1e-6, 1e-8
    inp, f = _neural_case(B, T, D, seed=D + B)
    inp["t"] = t = tg.grid(case["grid"], T)
    cot = torch.randn(T, B, D, generator=torch.Generator().manual_seed(D))
    adaptive.keep_workspace = True
    try:
        got = _neural_hip_dopri5(inp, f, dev, cot, rtol, atol, detach=case["detach"])
        tape = adaptive.read_tape()
    finally:
        adaptive.keep_workspace = False
    assert got["stats"]["n_accepted"] > 1 and tape["t"][0] == float(t[0])
    record_property("outputs_per_step_max", max(_tape_covers(case, tape, t)))
    assert torch.equal(got["h"][0], inp["z0"])
    first = (not case["detach"]) and bool(tape["init"]["first_accepted"])
    f64 = copy.deepcopy(f).double()
    f64.dosage, f64.times = f.dosage.double(), f.times.double()
    y64 = inp["z0"].double().requires_grad_(True)
    hr = odeint_dopri5_replay(f64, y64, t.double(), rtol, atol, list(zip(tape["t"], tape["dt"])), first)
    (hr * cot.double()).sum().backward()
    err = (got["h"].double() - hr.detach()).abs().max().item()
    record_property("err_h", err / (1 + hr.abs().max().item()))
    assert err <= NEURAL_DOPRI5_TRAJ_TOL * (1 + hr.abs().max().item()), err
    n = f64.ml_net
    for k, a, b in zip(NEURAL_GRADS, got["g"], [y64.grad, n[0].weight.grad, n[0].bias.grad, n[2].weight.grad, n[2].bias.grad]):
        e = _rel(a, b)
        record_property("err_" + k, e)
        assert e <= 1e-4, (k, case["detach"], e)


# ------------------------------------------------------------------------------------------------------ real-data Roche
@pytest.mark.parametrize("case", tg.family("real"), ids=tg.case_id)
def test_real_time_grid(case, record_property):
    """real_kernel and real_mf_kernel (on-chip and tape-writing backward): the dose row is floor(t), on grids whose nodes lie
    on both sides of integer times and, from t[0] = 2.5, past the last action row."""
    dev = _dev()
    H, method = case["H"], case["method"]
    p, ref = tg.real_problem(case)
    got = _real_gpu(p, H, method, dev) if case["onchip"] else _real_gpu_tape_backward(p, H, method, dev)
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in ("gy0", "gw", "gth"):
        e = _rel(got[k], ref[k])
        record_property("err_" + k, e)
        assert e <= 1e-4, (k, e)


# ---------------------------------------------------------------- real-data Roche at the ragged sizes (libhode_real_dims.so)
@pytest.mark.parametrize("case", tg.family("real_dims"), ids=tg.case_id)
def test_real_dims_time_grid(case, record_property):
    """real_dims_kernel<HT, method, fwd / bwd> (the on-chip backward, the only one the library has) and its folds: step sizes
    that differ within one call, stages of one step on both sides of an integer time, rows past the last action row and,
    from -1.0, negative stage times; rk4 also without perturb (the last stage exactly on t1)."""
    from hode import _real_dims_lib as RD
    dev = _dev()
    H, method = case["H"], case["method"]
    assert RD.real_solver_library(case["D"]) is RD.side_library()
    p, ref = tg.real_problem(case)
    assert p["y0"].shape == (case["B"], case["D"]) and p["perturb"] == case["perturb"]
    got = _real_gpu(p, H, method, dev)
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in ("gy0", "gw", "gth"):
        e = _rel(got[k], ref[k])
        record_property("err_" + k, e)
        assert e <= 1e-4, (k, e)


# ------------------------------------------------------------------------------- one-step-ahead (libhode_real_step.so)
STEP_GRADS = ("ginit", "gw", "gth")


def _real_step_gpu(p, case, dev, C=None):
    """hode.real_step.real_step_solve + autograd on the case's grid, with its step_size and run length (C overrides)."""
    from hode.real_step import real_step_solve
    wflat = p["wflat"].to(dev).requires_grad_(True)
    theta = p["theta"].to(dev).requires_grad_(True)
    init = p["init"].to(dev).requires_grad_(True)
    h = real_step_solve(init, theta, wflat, p["t"].to(dev), p["a"][..., 0].to(dev), case["H"], method=case["method"],
                        perturb=case["perturb"], step_size=p["step_size"], intervals_per_wave=case["C"] if C is None else C)
    (h * p["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), ginit=init.grad, gw=wflat.grad, gth=theta.grad)


def _real_step_ok(got, ref, record_property=None, keys=STEP_GRADS):
    if record_property is not None:
        record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in keys:
        assert torch.isfinite(got[k]).all(), k
        e = _rel(got[k], ref[k]) if float(ref[k].abs().max()) > 0 else float(got[k].abs().max())
        if record_property is not None:
            record_property("err_" + k, e)
        assert e <= 1e-4, (k, e)


@pytest.mark.parametrize("case", tg.family("real_step"), ids=tg.case_id)
def test_real_step_time_grid(case, record_property):
    """real_step_dose_kernel, real_step_kernel<HT, method, fwd / bwd> and the folds against one fp64 oracle solve per interval:
    intervals of different lengths (every row of the (N, S + 1) table is its own), on sub2 / sub3 a clipped last sub-step
    of another length in every interval, from the starts 0.0, 2.5 and -1.0."""
    from hode import _real_step_lib as RS
    from hode.real_step import interval_grids
    dev = _dev()
    p, ref = tg.real_step_inputs(case), tg.real_step_ref(case)
    assert interval_grids(p["t"], p["step_size"]).shape == (case["N"], case["S"] + 1)
    got = _real_step_gpu(p, case, dev)
    assert RS.LIBRARY.handle is not None  # real_step_solve has no other library to call: it is loaded by now
    assert got["h"].shape == (case["N"] + 1, case["B"], case["D"]) and got["ginit"].shape == p["init"].shape
    assert bool((got["h"][0] == 0).all())
    _real_step_ok(got, ref, record_property)


@pytest.mark.parametrize("case", [c for c in tg.family("real_step") if c["grid"] == "ragged"][:3], ids=tg.case_id)
def test_real_step_matches_the_chained_kernels_on_intervals_that_differ(case):
    """S = 1 on the ragged grid from each start: h[i + 1] and grad_init[i] are real_solve(init[i], t[i : i + 2]) bit for bit --
    libhode_real_dims.so at D <= 19, libhode.so at 20 --, interval by interval
    (test_hip_real_step.test_one_step_matches_the_chained_kernels_interval_by_interval where no two intervals are alike)."""
    import hode
    from hode import _real_dims_lib as RD
    from hode.real import real_solve
    dev = _dev()
    assert case["S"] == 1
    p = tg.real_step_inputs(case)
    got = _real_step_gpu(p, case, dev)
    t, act, cot = p["t"].to(dev), p["a"][..., 0].to(dev), p["cot"].to(dev)
    assert RD.real_solver_library(case["D"]) is (hode.lib() if case["D"] == 20 else RD.side_library())
    gw = torch.zeros_like(got["gw"])
    for i in range(case["N"]):
        y0 = p["init"][i].to(dev).requires_grad_(True)
        wflat = p["wflat"].to(dev).requires_grad_(True)
        hc = real_solve(y0, p["theta"].to(dev), wflat, t[i:i + 2], act, case["H"], method=case["method"], perturb=case["perturb"])
        (hc[1] * cot[i + 1]).sum().backward()
        same_h, same_g = torch.equal(hc[1].detach(), got["h"][i + 1]), torch.equal(y0.grad, got["ginit"][i])
        assert same_h and same_g, (i, same_h, same_g)
        gw += wflat.grad
    assert _rel(got["gw"], gw) <= 1e-4


@pytest.mark.parametrize("case", [next(c for c in tg.family("real_step") if c["grid"] == g and c["N"] == 7 and c["B"] == 37)
                                  for g in ("sub2", "sub3")], ids=tg.case_id)
def test_real_step_run_length_changes_no_state_on_sub_step_grids(case):
    """h and grad_init do not depend on how the intervals are cut into runs (C = 0, 1, 2, 3, N, N + 2) where every interval
    has a row and a clipped sub-step of its own; the folded gradients change in their summation order only and are held to
    the fp64 bound for each C."""
    dev = _dev()
    p, ref = tg.real_step_inputs(case), tg.real_step_ref(case)
    N = case["N"]
    default = _real_step_gpu(p, case, dev, C=0)
    for C in (0, 1, 2, 3, N, N + 2):
        forced = _real_step_gpu(p, case, dev, C=C)
        assert torch.equal(forced["h"], default["h"]) and torch.equal(forced["ginit"], default["ginit"]), C
        _real_step_ok(forced, ref)


# ------------------------------------------------------------------- NeuralODE at the odd sizes (libhode_neural_odd.so)
def _served_by_the_odd_library(D):
    from hode import _lib as L, _neural_odd_lib as NO
    lib = NO.neural_solver_library(D)
    assert isinstance(lib, NO._AsLibhode) and lib is not L.lib()


@pytest.mark.parametrize("case", tg.family("neural_odd"), ids=tg.case_id)
def test_neural_odd_time_grid(case, record_property):
    """neural_mf_fwd_kernel<D, method> and neural_mf_bwd_kernel<D, method, true> at D = 5, 7, .., 15: two and more different
    step sizes in one call, a grid across zero from -1.0, impulse doses on nodes and before t[0]."""
    dev = _dev()
    method, perturb = case["method"], case["perturb"]
    _served_by_the_odd_library(case["D"])
    p = tg.neural_inputs(case)
    ref = tg.neural_solve_cpu(p, method, perturb)
    got = _neural_gpu(p, method, perturb, dev)
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    record_property("err_h", _err_h(got["h"], ref["h"]))
    _traj_ok(got["h"], ref["h"])
    for k in NEURAL_GRADS:
        err = _rel(got[k], ref[k]) if float(ref[k].abs().max()) > 0 else float(got[k].abs().max())
        record_property("err_" + k, err)
        assert err <= 1e-4, (k, err)


@pytest.mark.parametrize("case", tg.family("neural_odd_dopri5"), ids=tg.case_id)
def test_neural_odd_dopri5_time_grid(case, record_property):
    """ndp_*<D> at the odd sizes: the dense-output loop with several output times inside one accepted step and accepted steps
    that cover none (clustered), and the whole solve from t[0] = 2.5 (offset+), against the fp64 replay of the run's own tape."""
    _served_by_the_odd_library(case["D"])
    _neural_dopri5_on_grid(case, record_property)


# ------------------------------------------------------------------------------------------------------- neural real
@pytest.mark.parametrize("case", tg.family("neural_real"), ids=tg.case_id)
def test_neural_real_time_grid(case, record_property):
    """neural_real_* through hode.odeint on the grid itself (no step_size): host stage_rows on a ragged grid, negative rows
    on the grid from -1, rows past the action's end."""
    t = tg.grid(case["grid"], case["T"])
    h, hc, got, want = _neural_real(case["kind"], case["D"], case["method"], case["H"], case["B"], case["perturb"], None, _dev(),
                                    Ta=tg.REAL_TA[case["grid"]], seed=case["D"] + case["H"], t=t)
    y0 = tg.neural_real_inputs(case)[0]
    assert torch.equal(h[0].detach().cpu(), y0)
    record_property("err_h", _err_h(h.detach(), hc.detach()))
    _traj_ok(h, hc)
    for name, g, w in zip(("y0", "w1", "b1", "w2", "b2"), got, want):
        record_property("err_g" + name, _rel(g, w))
        assert _rel(g, w) < NEURAL_REAL_GRAD_TOL, (name, _rel(g, w))
