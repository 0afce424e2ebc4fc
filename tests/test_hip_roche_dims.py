"""The hybrid decoder at the latent sizes libhode.so does not hold (libhode_roche_dims.so), on the GPU.

Fixed grid: one test per entry of tests/roche_dims_cases.py -- every compiled (D, layout, method, rhs, theta-gradient)
kernel with every rhs body it holds -- against the float64 oracle at the bounds tests/test_hip_kernel_variants.py holds the
Roche cases to (TRAJ_TOL * (1 + max|ref|), rel-L2 GRAD_TOL, grad_theta per component), imported from there; the targeted
cases (perturb, several doses, a dose on a stage time, non-uniform and offset grids as tests/time_grids.py builds them,
B = 1, T = 1, T = 2, negative-base Hill exponents) at the sizes with the most padding; and the padding test: every tensor at
the very end of its allocation and 4-byte aligned only, a poisoned guard around the workspace, bit-identity with the same
call on ordinary tensors.  dopri5: the table's cases against the fp64 tape replay, as test_dopri5_backward.  Model level:
RocheExpertDecoder / VariationalInference / the training loop / evaluate at sizes only the side library serves, and g16's
inputs through the kernels."""
import copy
import os

import numpy as np
import pytest
import torch

import kernel_variants as kv
import roche_dims_cases as cases
import time_grids as tg
from test_hip_kernel_variants import (_dev, _dp_case, _grad_ok, _problem_key, _ref_finite, _rel, _roche_problem, _same_as_with_theta,
                                      _theta_components_ok, _traj_ok)

pytestmark = pytest.mark.gpu


def _library(D):
    from hode import _roche_dims_lib as RL
    lib = RL.roche_solver_library(D)
    assert lib is not __import__("hode").lib()
    return lib


def _solve(p, dev, method, ablate, lanes, need_theta, perturb=False):
    """hode.roche_solve + backward through autograd on the side library."""
    import hode
    from hode import _lib as L
    theta = torch.zeros(L.N_THETA)
    n = p["theta"].numel()
    theta[:n] = p["theta"]
    theta = theta.to(dev).requires_grad_(need_theta)
    y0 = p["y0"].to(dev).requires_grad_(True)
    w, b = p["w"].to(dev).requires_grad_(True), p["b"].to(dev).requires_grad_(True)
    h = hode.roche_solve(y0, theta, w, b, p["t"].to(dev), p["dosage"].to(dev), p["times"].to(dev), method=method, ablate=ablate,
                         perturb=perturb, lanes_per_patient=lanes, library=_library(p["y0"].shape[1]))
    (h * p["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = dict(h=h.detach().clone(), gy0=y0.grad.clone(), gw=w.grad.clone(), gb=b.grad.clone())
    if need_theta:
        out["gth"] = theta.grad[:n].clone()
    return out


def _check(got, ref, p, record_property=None):
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    _traj_ok(got["h"], ref["h"])
    errs = {"h": (got["h"].double().cpu() - ref["h"]).abs().max().item() / (1 + ref["h"].abs().max().item())}
    for k in ("gy0", "gw", "gb", "gth"):
        if k in got:
            errs[k] = _grad_ok(k, got[k], ref[k])
    if "gth" in got:
        errs["gth_comp"] = _theta_components_ok(got["gth"], ref["gth"])
    if record_property is not None:
        for k, v in errs.items():
            record_property("err_" + k, v)
    return errs


# ------------------------------------------------------------------------------------------ fixed grid: the whole table
@pytest.mark.parametrize("case", cases.FIXED_CASES, ids=cases.case_id)
def test_fixed_grid_against_fp64(case, record_property):
    dev = _dev()
    D, method, ablate = case["D"], case["method"], case["ablate"]
    p, ref = _roche_problem(D, method, ablate, _problem_key(case))
    _ref_finite(case, ref)
    got = _solve(p, dev, method, ablate, case["lanes"], case["need_theta"])
    record_property("body", kv.body(case))
    _check(got, ref, p, record_property)
    if not case["need_theta"]:
        with_th = _solve(p, dev, method, ablate, case["lanes"], True)
        assert torch.equal(got["h"], with_th["h"])
        # Two instantiations: nothing makes the compiler contract the shared products into the same fmas in both (it does
        # not at D = 5 with the ablate rhs, where grad_b moves by one ulp), so the theta work may move the other gradients
        # by rounding only -- tests/test_hip_kernel_variants.py's rel-L2 1e-6 for that situation, never bit identity
        for k in ("gy0", "gw", "gb"):
            _same_as_with_theta(got[k], with_th[k], False, k)


@pytest.mark.parametrize("D", cases.DIMS)
def test_the_default_layout_is_one_of_the_two(D):
    """lanes_per_patient = 0 gives, bit for bit, what the layout the library chooses gives when it is asked for."""
    dev = _dev()
    p, ref = _roche_problem(D, "rk4", False)
    got = _solve(p, dev, "rk4", False, 0, True)
    _check(got, ref, p)
    same = _solve(p, dev, "rk4", False, cases.rk_lpp(D, 0), True)
    for k in got:
        assert torch.equal(got[k], same[k]), k


# ----------------------------------------------------------------------------------------------- fixed grid: targeted
def _grid_problem(D, ablate, n_dose, grid, T, method, perturb):
    return tg._roche_inputs(D, ablate, n_dose, grid, T), tg._roche_ref(D, ablate, n_dose, grid, T, method, perturb)


@pytest.mark.parametrize("lanes", cases.LANES)
@pytest.mark.parametrize("grid,perturb,n_dose,method", [("ragged", False, 1, "rk4"), ("ragged", True, 2, "rk4"), ("offset+", True, 1, "midpoint"),
                                                        ("offset-", False, 3, "euler"), ("offset+", False, 2, "rk4")])
@pytest.mark.parametrize("D", cases.TARGETED_DIMS)
def test_time_grids_perturb_and_doses_on_stage_times(D, grid, perturb, n_dose, method, lanes):
    """tests/time_grids.py's problems at the new sizes: non-uniform and offset grids, doses on nodes (a dose exactly on the
    first stage time of a step; with perturb that stage moves one ulp past it), inside steps and before t[0], several doses
    per patient."""
    dev = _dev()
    p, ref = _grid_problem(D, False, n_dose, grid, 8, method, perturb)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    # a dose sits exactly on a grid node that starts a step
    assert bool((p["times"][:, :, None] == p["t"][None, None, :-1]).any())
    _check(_solve(p, dev, method, False, lanes, True, perturb=perturb), ref, p)


@pytest.mark.parametrize("lanes", cases.LANES)
@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("B,T", cases.EDGE_SHAPES)
@pytest.mark.parametrize("D", cases.TARGETED_DIMS)
def test_edge_shapes(D, B, T, method, lanes):
    """One patient (every other lane of the wave is dead), T = 1 (no step: h = y0, grad_y0 = grad_h[0], zero parameter
    gradients) and T = 2 (one step)."""
    dev = _dev()
    full = tg._roche_inputs(D, False, 1, "ragged", 8)
    p = dict(full, y0=full["y0"][:B].clone(), dosage=full["dosage"][:B].clone(), times=full["times"][:B].clone(),
             t=full["t"][:T].clone(), cot=full["cot"][:T, :B].clone())
    got = _solve(p, dev, method, False, lanes, True)
    if T == 1:
        assert torch.equal(got["h"][0].cpu(), p["y0"]) and torch.equal(got["gy0"].cpu(), p["cot"][0])
        for k in ("gw", "gb", "gth"):
            assert float(got[k].abs().max()) == 0.0, k
    else:
        _check(got, tg.roche_solve_cpu(p, method, False, False), p)


def _tiled(p, B):
    """The problem's inputs repeated along the batch to B patients (every 77th patient is the same one)."""
    reps = -(-B // p["y0"].shape[0])
    return dict(p, y0=p["y0"].repeat(reps, 1)[:B].clone(), dosage=p["dosage"].repeat(reps)[:B].clone(),
                times=p["times"].repeat(reps, 1)[:B].clone(), cot=p["cot"].repeat(1, reps, 1)[:, :B].clone())


@pytest.mark.parametrize("lanes", cases.LANES)
@pytest.mark.parametrize("D", cases.TARGETED_DIMS)
def test_several_patients_per_wave(D, lanes):
    """At 77 patients the grid has one patient per wave (the host spreads a small batch over the SIMDs); MANY_N puts three on
    a wave and one on the last: the per-wave fold over patients and the dead lanes of a ragged last wave."""
    dev = _dev()
    B = cases.MANY_N
    assert cases.patients_per_wave(B, lanes) == 3 and B % 3 == 1
    p = _tiled(tg._roche_inputs(D, False, 1, "ragged", 8), B)
    _check(_solve(p, dev, "rk4", False, lanes, True), tg.roche_solve_cpu(p, "rk4", False, False), p)


@pytest.mark.parametrize("lanes", cases.LANES)
@pytest.mark.parametrize("D", cases.TARGETED_DIMS)
def test_negative_base_hill_exponents(D, lanes):
    """Hill 3 and 1 with a negative Immunity: finite trajectory, NaN in d / d HillCure exactly where the oracle has it."""
    dev = _dev()
    case = dict(family="roche", D=D, theta="general", hill=kv.NEG_BASE_HILL, n_dose=2, neg_imm=True, ablate=False)
    p, ref = _roche_problem(D, "midpoint", False, _problem_key(case))
    _ref_finite(case, ref)
    _check(_solve(p, dev, "midpoint", False, lanes, True), ref, p)


# ------------------------------------------------------------------------------------------------------------ padding
GUARD = 4096  # floats of poison before and after the partial workspace


def _at_end(x, dev, slack=3):
    """x at the very end of an allocation of its own, 4-byte aligned only where the size allows it: the storage is the
    tensor plus `slack` leading floats, so the last element is the last of the allocation."""
    buf = torch.empty(slack + x.numel(), device=dev, dtype=torch.float32)
    view = buf[slack:].view(x.shape)
    view.copy_(x)
    return view


@pytest.mark.parametrize("need_theta", [True, False])
@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("B", [cases.N, cases.MANY_N])
@pytest.mark.parametrize("D", [5, 15])
def test_padding_reads_and_writes_nothing(D, B, method, need_theta):
    """Through the C ABI, ragged quad layout: w1, b1, y0, h, grad_h, grad_y0 and the partial workspace each end their
    allocation and are 4-byte aligned only; the workspace lies between two poisoned guards that must come back unchanged;
    and every output equals, bit for bit, the same call on ordinary 16-byte aligned tensors.  A padding slot that wrote
    through the (lane * MR + r) * D + i formula would land in the bias / theta part of the row or in the guard; one that read
    would see other bytes in the two runs."""
    import ctypes as C
    from hode import _lib as L, _roche_dims_lib as RL
    dev = _dev()
    lib = RL.lib()
    p = _tiled(_roche_problem(D, method, False)[0], B)
    T, M = cases.T, D - 4
    theta = torch.zeros(L.N_THETA)
    theta[: p["theta"].numel()] = p["theta"]
    fixed = dict(t=p["t"].to(dev), dosage=p["dosage"].to(dev), times=p["times"].to(dev), theta=theta.to(dev))
    POISON = 1.2345e30

    def run(odd):
        put = (lambda x: _at_end(x, dev)) if odd else (lambda x: x.to(dev).clone())
        y0, w, b, cot = put(p["y0"]), put(p["w"]), put(p["b"]), put(p["cot"])
        h, gy0 = put(torch.zeros(T, B, D)), put(torch.zeros(B, D))
        gw, gb, gth = torch.zeros(M, D, device=dev), torch.zeros(M, device=dev), torch.zeros(L.N_THETA, device=dev)
        if odd:
            assert all(x.data_ptr() % 16 != 0 for x in (y0, h, cot, gy0)) and w.data_ptr() % 16 != 0
        d = L.new_solve_desc()
        d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.n_dose = L.RHS_ROCHE, L.METHODS[method], B, D, T, 1
        d.lanes_per_patient, d.need_theta_grad = 4, int(need_theta)
        d.t, d.y0, d.dosage, d.dose_times, d.theta = (fixed["t"].data_ptr(), y0.data_ptr(), fixed["dosage"].data_ptr(),
                                                      fixed["times"].data_ptr(), fixed["theta"].data_ptr())
        d.w1, d.b1, d.h = w.data_ptr(), b.data_ptr(), h.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        RL.check(lib.hode_roche_dims_rk_fwd(d, stream), "rk_fwd")
        nbytes = lib.hode_roche_dims_workspace_bytes(d, L.WS_RK_BWD)
        assert nbytes == cases.n_waves(B, 4) * (M * D + M + 15) * 4
        n = nbytes // 4
        arena = torch.full((GUARD + n + GUARD,), POISON, device=dev)
        d.grad_h, d.grad_y0, d.grad_w1, d.grad_b1, d.grad_theta = cot.data_ptr(), gy0.data_ptr(), gw.data_ptr(), gb.data_ptr(), gth.data_ptr()
        d.workspace, d.workspace_bytes = arena[GUARD:].data_ptr(), nbytes
        d.flags = L.FLAG_OVERWRITE_GRADS
        RL.check(lib.hode_roche_dims_rk_bwd(d, stream), "rk_bwd")
        torch.cuda.synchronize()
        assert bool((arena[:GUARD] == POISON).all()) and bool((arena[GUARD + n:] == POISON).all()), "guard overwritten"
        rows = arena[GUARD:GUARD + n].view(-1, M * D + M + 15)
        assert bool((rows != POISON).all()), "a slot of the partial row was not written"
        return dict(h=h.clone(), gy0=gy0.clone(), gw=gw, gb=gb, gth=gth)

    plain, odd = run(False), run(True)
    for k in plain:
        assert torch.equal(plain[k], odd[k]), (k, _rel(odd[k], plain[k]))
    if not need_theta:
        assert float(plain["gth"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------- dopri5
@pytest.fixture
def side_dopri5(monkeypatch):
    """test_hip_kernel_variants._dp_gpu calls adaptive.roche_dopri5 without `library`: hand it the caller's choice."""
    from hode import adaptive
    from hode._roche_dims_lib import roche_solver_library
    plain = adaptive.roche_dopri5

    def with_library(y0, *args, **kw):
        return plain(y0, *args, library=roche_solver_library(y0.shape[-1]), **kw)
    monkeypatch.setattr(adaptive, "roche_dopri5", with_library)


@pytest.mark.parametrize("case", cases.DOPRI5_CASES, ids=cases.case_id)
def test_dopri5_against_the_tape_replay(case, record_property, side_dopri5):
    """As test_hip_kernel_variants.test_dopri5_backward, bounds included: the oracle's step algebra replayed in fp64 along
    the kernel's own tape (read_tape through the side library); first step detached -> rel-L2 1e-4, attached -> 1e-4 or
    twice the fp32 replay's own distance from fp64.  The detached
    cases carry no doses (tests/roche_dims_cases.py::_dopri5_cases says why and gives the figures measured with one)."""
    from test_hip_dopri5 import _replay
    dev = _dev()
    got, other, tape, inp, f = _dp_case(case, dev)
    assert len(tape["t"]) > 1 and tape["t"][0] == 0.0
    first = (not case["detach"]) and bool(tape["init"]["first_accepted"])
    ref = _replay(inp, f, 1e-7, 1e-8, inp["cot"], tape, first, double=True)
    for k, v in ref.items():
        if k != "sigma":
            assert torch.isfinite(v).all(), k
    ref32 = _replay(inp, f, 1e-7, 1e-8, inp["cot"], tape, first) if first else None
    _traj_ok(got["h"], ref["h"])
    with_th = got if case["need_theta"] else other
    record_property("body", kv.body(case))
    for k in ("gy0", "gw", "gb", "gth"):
        g = got[k] if k in got else with_th[k]
        rk = ref["gtheta" if k == "gth" else k]
        tol = max(1e-4, 2.0 * _rel(ref32["gtheta" if k == "gth" else k], rk)) if first else 1e-4
        record_property("err_" + k, _grad_ok(k, g, rk, tol))
        if k != "gth":
            _same_as_with_theta(got[k], other[k], False, k)
    floor = 2.0 * (ref32["gtheta"] - ref["gtheta"]).abs() if first else None
    record_property("err_gth_comp", _theta_components_ok(with_th["gth"], ref["gtheta"], floor))


@pytest.mark.parametrize("D", [7, 10, 16])
def test_dopri5_under_no_grad_takes_the_tape_less_path(D):
    """HODE_FLAG_NO_TAPE through the side library: same trajectory bit for bit, two state rows instead of the tape."""
    import model
    from hode import adaptive, synth
    dev = _dev()
    obs, T, B, step = 40, 20, 64, synth.STEP
    torch.manual_seed(3)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * step, step, method="dopri5", device=dev)
    sol = synth.solver_inputs(B, T, D, seed=8)
    z0, a = sol["z0"].to(dev), sol["actions"].to(dev)
    _, h_grad = dec(z0, a)
    st_grad = dict(adaptive.last_stats)
    with torch.no_grad():
        _, h_eval = dec(z0, a)
    st_eval = dict(adaptive.last_stats)
    assert st_grad["no_tape"] is False and st_eval["no_tape"] is True
    assert st_grad["workspace_bytes"] >= (16 * T + 64) * B * D * 4
    assert st_eval["workspace_bytes"] <= 24 * (1 << 20) + 64 * B * D * 4 + (1 << 16)
    assert st_eval["n_accepted"] == st_grad["n_accepted"] and torch.equal(h_grad.detach(), h_eval)


# -------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("method", ["rk4", "dopri5"])
@pytest.mark.parametrize("obs,D", [(40, 7), (40, 10)])
def test_vi_loss_and_grads_match_cpu_oracle(method, obs, D):
    """tests/test_hip_model.py::test_vi_loss_and_grads_match_cpu_oracle at sizes only the side library serves, at the bounds
    it holds D = 8 to."""
    import model
    from hode import adaptive, synth
    from oracle import vi as ovi
    from oracle.encoder import EncoderLSTMOracle
    from test_hip_model import odeint_h
    dev = _dev()
    T, B, step = 20, 48, synth.STEP
    torch.manual_seed(1)
    enc = model.EncoderLSTM(obs + 1, obs * 2, D, device=dev)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * step, step, method=method, device=dev)
    vi = model.VariationalInference(enc, dec, elbo=False)
    enc_o = EncoderLSTMOracle(obs + 1, obs * 2, D)
    dec_o = ovi.DecoderOracle(obs, D, (T - 1) * step, step, method=method)
    enc_o.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    dec_o.load_state_dict({k: v.cpu() for k, v in dec.state_dict().items()})
    sol = synth.solver_inputs(B, T, D, seed=3)
    ob = synth.observation_inputs(B, T, obs, seed=3)
    data = {"measurements": ob["measurements"], "actions": sol["actions"], "masks": ob["masks"]}
    adaptive.keep_workspace = method == "dopri5"
    try:
        loss = vi.loss({k: v.to(dev) for k, v in data.items()})
        loss.backward()
        if method == "dopri5":
            from oracle.solvers import odeint_dopri5_replay
            tape = adaptive.read_tape()
            pairs, first = list(zip(tape["t"], tape["dt"])), bool(tape["init"]["first_accepted"])
            dec_o.solve = lambda f, y0, t: odeint_dopri5_replay(f, y0, t, 1e-7, 1e-8, pairs, first)
    finally:
        adaptive.keep_workspace = False
    loss_o = ovi.vi_loss(enc_o, dec_o, data, elbo=False)
    loss_o.backward()
    tol_h, tol_g = 3e-5, 2e-3
    assert abs(loss.item() - loss_o.item()) <= 2e-4 * abs(loss_o.item())
    assert (vi.h_hat.detach().cpu() - odeint_h(dec_o, enc_o, data)).abs().max().item() <= tol_h * 10
    names = [n for n, _ in list(enc.named_parameters()) + list(dec.named_parameters())]
    g_hip = [p.grad for p in list(enc.parameters()) + list(dec.parameters())]
    g32 = [None if p.grad is None else p.grad.clone() for p in list(enc_o.parameters()) + list(dec_o.parameters())]
    noise = [0.0] * len(g32)
    if method == "dopri5":  # the fp64 oracle along the same tape is the yardstick, as in test_hip_model.py
        enc_o.double(); dec_o.double()
        for p in list(enc_o.parameters()) + list(dec_o.parameters()):
            p.grad = None
        data64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items()}
        ovi.vi_loss(enc_o, dec_o, data64, elbo=False).backward()
        g64 = [p.grad for p in list(enc_o.parameters()) + list(dec_o.parameters())]
        noise = [0.0 if a is None or b is None else _rel(a, b) for a, b in zip(g32, g64)]
    else:
        g64 = g32
    for n, g, go, nz in zip(names, g_hip, g64, noise):
        if go is None:
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        assert g is not None, n
        if float(go.abs().max()) < 1e-12:
            continue
        assert _rel(g, go) <= max(tol_g, 2.0 * nz), (n, _rel(g, go), nz)


@pytest.mark.parametrize("ablate", [False, True])
def test_training_loop_and_evaluate_at_10(tmp_path, ablate):
    """Two iterations of variational_training_loop and evaluate with the hybrid decoder (and its ablation) at D = 10."""
    import model
    import training_utils
    from hode import synth
    from hode.batches import DeviceFolds
    dev = _dev()
    T, obs, D = 16, 40, 10
    folds = DeviceFolds.synthetic(192, T, obs, D, 32, 32, dev, seed=4)
    torch.manual_seed(1)
    enc = model.EncoderLSTM(obs + 1, obs * 2, D, device=dev)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * synth.STEP, synth.STEP, method="rk4", ablate=ablate, device=dev)
    vi = model.VariationalInference(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density)
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.output_function.parameters()) + list(dec.ode.ml_net.parameters()), lr=1e-3)
    w0 = dec.ode.ml_net[0].weight.detach().clone()
    vi, best, _ = training_utils.variational_training_loop(2, folds, vi, 64, opt, 2, path=str(tmp_path) + "/")
    assert best < 1e9 and not torch.equal(dec.ode.ml_net[0].weight.detach(), w0)
    out = training_utils.evaluate(vi, folds, 16, 8, mc_itr=5)
    assert len(out) == 6 and all(v == v for v in out)


def test_a_size_nobody_serves_raises_before_any_launch():
    import hode
    import model
    from hode import synth
    dev = _dev()
    dec = model.RocheExpertDecoder(40, 17, 1, 1.0, synth.STEP, method="rk4", device=dev)
    sol = synth.solver_inputs(4, 9, 17, seed=1)
    with pytest.raises(hode.HodeConfigError, match="libhode_roche_dims.so"):
        dec(sol["z0"].to(dev), sol["actions"].to(dev))


# ------------------------------------------------------------------------------------------------------ g16's inputs
@pytest.mark.parametrize("lanes", [0, 4, 1])
def test_g16_roche_rhs_values_and_vjps_through_one_euler_step(golden_dir, lanes):
    """The reference's RocheODE at D in 5, 7, 10, 15, 16 (tests/golden/make_golden_roche_dims.py), read off one euler step
    of the kernels as tests/test_hip_golden.py reads G1, at its bounds."""
    import model
    from test_hip_golden import _euler_rhs, _load_sd
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g16_roche_dims.npz"), allow_pickle=False)
    for ci in range(int(g["n_cases"])):
        pre = "c%d_" % ci
        D, ablate, T, B = [int(v) for v in g[pre + "meta"]]
        step = float(g[pre + "step"])
        ode = model.RocheODE(D, 1, (T - 1) * step, step, ablate=bool(ablate), device=dev)
        _load_sd(ode, g, pre + "sd_")
        ode.lanes_per_patient = lanes
        ode.set_action(torch.from_numpy(g[pre + "action"]).to(dev))
        np.testing.assert_array_equal(ode.times.cpu().numpy(), g[pre + "times"])
        np.testing.assert_array_equal(ode.dosage.cpu().numpy(), g[pre + "dosage"])
        y, cot = torch.from_numpy(g[pre + "y"]), torch.from_numpy(g[pre + "cot"])
        for ti, t in enumerate(g[pre + "t"]):
            f, gy, gp = _euler_rhs(ode, y, t, cot, dev)
            want = g[pre + "f"][ti]
            assert np.array_equal(np.isnan(f), np.isnan(want)), (ci, ti)
            tol = 3e-7 * (1.0 + np.abs(y.numpy()) + np.abs(np.nan_to_num(want)))
            assert np.all(np.abs(np.nan_to_num(f) - np.nan_to_num(want)) <= tol), (ci, ti, np.abs(f - want).max())
            wgy = g[pre + "gy"][ti]
            ok = ~np.isnan(wgy)
            assert np.all(np.abs(gy[ok] - wgy[ok]) <= 2e-6 * (1.0 + np.abs(cot.numpy()[ok]) + np.abs(wgy[ok]))), (ci, ti)
            for n, got in gp.items():
                w = g[pre + "g_" + n.replace(".", "__")][ti]
                if np.isnan(w).any():
                    continue       # d pow(x, a) / da at a negative base: NaN in the reference's sum over patients
                if got is None:
                    assert np.abs(w).max() == 0.0, (ci, ti, n)
                    continue
                assert np.abs(got.numpy() - w).max() <= 3e-5 * (1.0 + np.abs(w).max()), (ci, ti, n)
