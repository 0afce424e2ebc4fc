"""The dose-gradient adjoint (libhode_dose.so, hode.dose, model._RocheDoseGrad) on the GPU against oracle.rhs.RocheRHS in
float64 under oracle.solvers.odeint with `dosage` a leaf: every case of tests/dose_cases.py (every compiled kernel, every rhs
body, perturb, non-uniform and offset grids, dose times on and one ulp either side of grid and stage times, a patient with
dosage 0, a patient dosed after t[-1]) within GRAD_TOL rel-L2 for gdosage, gy0, gtheta, gw and gb, h bit for bit the plain
lane-per-patient call's; lane independence, sentinels, repeats and the tensors autograd really hands the binding bit for bit;
and RocheExpertDecoder with ode.dose_grad = True against the float64 oracle decoder.  GPU only."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import dose_cases as cases
import model
import reference_checks as rc

GRAD_TOL = rc.GRAD_TOL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _theta16(theta):
    return torch.cat([theta, theta.new_zeros(16 - theta.numel())])


def _inputs(c, dev):
    """The case's inputs on the device (copies: the shared ones stay as they are)."""
    p = cases.setup(c)
    out = {k: p[k].to(dev) for k in ("y0", "t", "dosage", "times", "cot")}
    out["theta"] = _theta16(p["theta"]).to(dev)
    out["w"] = p["w"].to(dev) if p["w"] is not None else None
    out["b"] = p["b"].to(dev) if p["b"] is not None else None
    return out


def _plain_forward(c, q):
    import hode
    with torch.no_grad():
        return hode.roche_solve(q["y0"], q["theta"], q["w"], q["b"], q["t"], q["dosage"], q["times"], method=c["method"],
                                ablate=c["ablate"], perturb=c["perturb"], lanes_per_patient=1)


def _backward(c, q, h, grad_h=None, **over):
    from hode import dose
    a = dict(q, **over)
    return dose.dose_backward(a.get("h", h), a["theta"], a["w"], a["b"], a["t"], a["dosage"], a["times"],
                              a["cot"] if grad_h is None else grad_h, method=c["method"], ablate=c["ablate"], perturb=c["perturb"],
                              need_theta=c["need_theta"])


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# --------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_gradients_match_the_float64_oracle(c):
    dev = _dev()
    q, ref = _inputs(c, dev), cases.oracle(c)
    leaves = {k: q[k].clone().requires_grad_(True) for k in ("y0", "dosage") + (("w", "b") if c["D"] > 4 else ())}
    theta = q["theta"].clone().requires_grad_(c["need_theta"])
    times, t = q["times"].clone().requires_grad_(True), q["t"].clone().requires_grad_(True)
    h = model._RocheDoseGrad.apply(leaves["y0"], theta, leaves.get("w"), leaves.get("b"), t, leaves["dosage"], times, c["method"],
                                   c["ablate"], c["perturb"], False, None)
    assert torch.equal(h, _plain_forward(c, q))  # bit for bit the plain lane-per-patient call
    (h * q["cot"]).sum().backward()
    torch.cuda.synchronize()
    assert times.grad is None and t.grad is None
    names = cases.theta_names(c["ablate"])
    got = {"gy0": leaves["y0"].grad, "gdosage": leaves["dosage"].grad, "gth": theta.grad[:len(names)] if c["need_theta"] else None,
           "gw": leaves["w"].grad if c["D"] > 4 else None, "gb": leaves["b"].grad if c["D"] > 4 else None}
    if not c["need_theta"]:
        assert theta.grad is None
    errs = {}
    for k, g in got.items():
        if g is None:
            continue
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
        if float(ref[k].norm()) == 0.0:
            assert not g.any(), k  # exactly 0 where the reference is (gdosage under ablate and with a single output time)
            continue
        errs[k] = cases.rel_l2(g, ref[k])
    print("%s: rel-L2 %s" % (cases.case_id(c), ", ".join("%s %.2e" % kv for kv in errs.items())))
    gd = got["gdosage"].cpu()
    if c["ablate"] or c["T"] == 1:
        assert not gd.any()
    else:
        assert "gdosage" in errs and float(gd[cases.late_row(c)]) == 0.0 and float(gd[cases.zero_row(c)]) != 0.0
    assert all(e <= GRAD_TOL for e in errs.values()), errs


# ---------------------------------------------------------------------------------------- properties, bit for bit
PROPERTY_CASES = [c for c in cases.CASES if cases.case_id(c) in (
    "D12-rk4-B65-T9-K3", "D8-midpoint-B64-T9-K1-hill", "D6-euler-B64-T9-K2-perturb", "D4-rk4-B1027-T2-K1")]


def test_the_property_cases_are_in_the_table():
    assert len(PROPERTY_CASES) == 4 and {c["D"] for c in PROPERTY_CASES} == set(cases.DIMS)


@pytest.mark.parametrize("c", PROPERTY_CASES, ids=cases.case_id)
def test_two_runs_are_bit_identical(c):
    q = _inputs(c, _dev())
    h = _plain_forward(c, q)
    first, second = _backward(c, q, h), _backward(c, q, h)
    assert all(_same(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("c", PROPERTY_CASES[:3], ids=cases.case_id)
def test_a_patient_alone_is_the_same_patient_in_row_0_and_in_row_64_of_65(c):
    """Lane independence: no tolerance.  gy0 and gdosage of one patient do not depend on who else is in the batch."""
    dev = _dev()
    q = _inputs(c, dev)
    for src in (0, 7):
        one = {k: (v[src:src + 1] if k in ("y0", "dosage", "times") else v[:, src:src + 1] if k == "cot" else v) for k, v in q.items()}
        g1 = _backward(c, one, _plain_forward(c, one))
        for row in (0, 64):
            idx = torch.arange(65, device=dev) % q["y0"].shape[0]
            idx[row] = src
            many = {k: (v[idx] if k in ("y0", "dosage", "times") else v[:, idx] if k == "cot" else v) for k, v in q.items()}
            h = _plain_forward(c, many)
            assert torch.equal(h[:, row], _plain_forward(c, one)[:, 0])
            g65 = _backward(c, many, h)
            assert torch.equal(g65[0][row], g1[0][0]) and torch.equal(g65[4][row], g1[4][0]), (src, row)


@pytest.mark.parametrize("c", PROPERTY_CASES, ids=cases.case_id)
def test_the_tensors_autograd_hands_the_binding(c):
    """An expanded grad_h, slices at byte offsets 4 and 8 and fp64 inputs give the bits of the plain call."""
    dev = _dev()
    q = _inputs(c, dev)
    h = _plain_forward(c, q)
    row = q["cot"][:1].contiguous()
    want = _backward(c, q, h, grad_h=row.expand_as(q["cot"]).contiguous())
    got = _backward(c, q, h, grad_h=row.expand_as(q["cot"]))
    assert not row.expand_as(q["cot"]).is_contiguous() or c["T"] == 1
    assert all(_same(a, b) for a, b in zip(got, want))
    want = _backward(c, q, h)

    def shifted(x, floats):
        if x is None:
            return None
        buf = torch.zeros(x.numel() + 4, device=dev, dtype=x.dtype)
        view = buf[floats:floats + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 * floats and view.is_contiguous()
        return view
    for floats in (1, 2):
        moved = {k: shifted(v, floats) for k, v in q.items()}
        got = _backward(c, moved, shifted(h, floats))
        assert all(_same(a, b) for a, b in zip(got, want)), floats
    wide = {k: (v.double() if v is not None else None) for k, v in q.items()}
    got = _backward(c, wide, h.double())
    assert all(g is None or g.dtype == torch.float32 for g in got) and all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("c", PROPERTY_CASES, ids=cases.case_id)
def test_sentinels_around_every_output_and_the_workspace(c):
    """The library called through its descriptor with guard zones around gdosage, gy0, the parameter gradients and the
    workspace: nothing outside an output is written, nothing past the last partial row inside the workspace either, and the
    results are those of hode.dose.dose_backward."""
    from hode import _dose_lib as DL
    from hode import _lib as L
    from hode.solver import _stream
    dev = _dev()
    q = _inputs(c, dev)
    h = _plain_forward(c, q)
    want = _backward(c, q, h)
    B, D, T, K = c["B"], c["D"], c["T"], c["K"]
    PAD, MARK = 64, -7.25

    def guarded(n, fill):
        buf = torch.full((n + 2 * PAD,), MARK, device=dev, dtype=torch.float32)
        buf[PAD:PAD + n] = fill
        return buf

    def intact(buf, n):
        return bool((buf[:PAD] == MARK).all()) and bool((buf[PAD + n:] == MARK).all())
    lib = DL.lib()
    d = DL.new_desc()
    d.rhs_kind = L.RHS_ROCHE_ABLATE if c["ablate"] else L.RHS_ROCHE
    d.method, d.perturb = L.METHODS[c["method"]], int(c["perturb"])
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.need_theta_grad = B, D, T, K, int(c["need_theta"])
    nbytes = lib.hode_dose_workspace_bytes(ctypes.byref(d))
    waves = -(-B // (-(-B // 1024)))
    P = (D - 4) * D + (D - 4) + 15
    assert nbytes == -(-waves * P * 4 // 256) * 256
    sizes = {"gy0": B * D, "gdos": B, "gw": (D - 4) * D, "gb": D - 4, "gth": 16, "ws": nbytes // 4}
    bufs = {k: guarded(n, MARK if k in ("gy0", "gdos", "ws") else 0.0) for k, n in sizes.items()}
    cot = q["cot"].contiguous()
    d.t, d.h, d.dosage, d.dose_times, d.theta = q["t"].data_ptr(), h.data_ptr(), q["dosage"].data_ptr(), q["times"].data_ptr(), q["theta"].data_ptr()
    d.w1, d.b1 = (q["w"].data_ptr(), q["b"].data_ptr()) if D > 4 else (0, 0)
    d.grad_h = cot.data_ptr()
    at = {k: v.data_ptr() + 4 * PAD for k, v in bufs.items()}
    d.grad_y0, d.grad_dosage, d.grad_theta = at["gy0"], at["gdos"], at["gth"]
    d.grad_w1, d.grad_b1 = (at["gw"], at["gb"]) if D > 4 else (0, 0)
    d.workspace, d.workspace_bytes = at["ws"], nbytes
    DL.check(lib.hode_dose_bwd(ctypes.byref(d), _stream()), "hode_dose_bwd")
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert intact(bufs[k], n), k
    ws = bufs["ws"][PAD:PAD + nbytes // 4]
    assert bool((ws[waves * P:] == MARK).all()) and not bool((ws[:waves * P] == MARK).any())
    assert torch.equal(bufs["gy0"][PAD:PAD + B * D].view(B, D), want[0]) and torch.equal(bufs["gdos"][PAD:PAD + B], want[4])
    if D > 4:
        assert torch.equal(bufs["gw"][PAD:PAD + sizes["gw"]].view(D - 4, D), want[2]) and torch.equal(bufs["gb"][PAD:PAD + D - 4], want[3])
    if c["need_theta"]:
        assert torch.equal(bufs["gth"][PAD:PAD + 16], want[1])
    else:
        assert not bufs["gth"][PAD:PAD + 16].any()


@pytest.mark.parametrize("c", PROPERTY_CASES[1:3], ids=cases.case_id)
def test_the_status_word_reports_a_non_finite_gradient_of_a_live_patient(c):
    """The library through its descriptor with a status word: 0 for finite gradients, a patient's largest finite cotangent
    included; HODE_STATUS_NONFINITE for an inf or a NaN in one patient's cotangent, at the last output time (it enters lam first)
    and at the first (it enters last), whichever row holds it."""
    from hode import _dose_lib as DL
    from hode import _lib as L
    from hode.solver import _stream
    dev = _dev()
    q = _inputs(c, dev)
    h = _plain_forward(c, q)
    B, D, T, K = c["B"], c["D"], c["T"], c["K"]
    lib = DL.lib()

    def status_of(cot):
        d = DL.new_desc()
        d.rhs_kind = L.RHS_ROCHE_ABLATE if c["ablate"] else L.RHS_ROCHE
        d.method, d.perturb = L.METHODS[c["method"]], int(c["perturb"])
        d.batch, d.latent_dim, d.n_times, d.n_dose, d.need_theta_grad = B, D, T, K, int(c["need_theta"])
        nbytes = lib.hode_dose_workspace_bytes(ctypes.byref(d))
        outs = {k: torch.zeros(n, device=dev) for k, n in (("gy0", B * D), ("gdos", B), ("gw", (D - 4) * D), ("gb", D - 4), ("gth", 16),
                                                            ("ws", nbytes // 4))}
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        d.t, d.h, d.dosage, d.dose_times, d.theta = q["t"].data_ptr(), h.data_ptr(), q["dosage"].data_ptr(), q["times"].data_ptr(), q["theta"].data_ptr()
        d.w1, d.b1, d.grad_h = q["w"].data_ptr(), q["b"].data_ptr(), cot.data_ptr()
        d.grad_y0, d.grad_dosage, d.grad_theta = outs["gy0"].data_ptr(), outs["gdos"].data_ptr(), outs["gth"].data_ptr()
        d.grad_w1, d.grad_b1, d.workspace, d.workspace_bytes = outs["gw"].data_ptr(), outs["gb"].data_ptr(), outs["ws"].data_ptr(), nbytes
        d.status = status.data_ptr()
        DL.check(lib.hode_dose_bwd(ctypes.byref(d), _stream()), "hode_dose_bwd")
        torch.cuda.synchronize()
        return int(status), outs

    code, outs = status_of(q["cot"].contiguous())
    assert code == 0 and all(bool(torch.isfinite(v).all()) for v in outs.values())
    big = torch.zeros_like(q["cot"])
    big[0, 3, 0] = torch.finfo(torch.float32).max  # enters lam last: gy0[3, 0] is the largest finite float, and is finite
    code, outs = status_of(big)
    assert code == 0 and float(outs["gy0"].view(B, D)[3, 0]) == torch.finfo(torch.float32).max
    for bad in (float("inf"), float("-inf"), float("nan")):
        for n, row, col in ((T - 1, 0, 0), (0, B - 1, D - 1), (T // 2, 5, 3)):
            cot = q["cot"].clone()
            cot[n, row, col] = bad
            code, outs = status_of(cot)
            assert code == L.STATUS_NONFINITE, (bad, n, row, col)
            assert not bool(torch.isfinite(outs["gy0"].view(B, D)[row]).all()), (bad, n, row, col)


def test_gy0_and_the_parameter_gradients_against_the_plain_adjoint():
    """DESIGN.md says whether gy0 is bit-identical to rk_bwd_kernel<D, 1, ...>: measured here, held to GRAD_TOL.  Both sides
    run rk_bwd_body, and still not every case is bit-identical: D12-rk4-B65-T9-K3 and D8-midpoint-B64-T9-K1-hill are (gy0, gw,
    gb); D6-euler-B64-T9-K2-perturb has gw and gb bit-identical and gy0 not (the stage dose is dosage times the unit
    schedule, a product the compiler contracts differently from DoseSched::at's own)."""
    import hode
    dev = _dev()
    for c in PROPERTY_CASES[:3]:
        q = _inputs(c, dev)
        y0 = q["y0"].clone().requires_grad_(True)
        w, b = q["w"].clone().requires_grad_(True), q["b"].clone().requires_grad_(True)
        theta = q["theta"].clone().requires_grad_(c["need_theta"])
        h = hode.roche_solve(y0, theta, w, b, q["t"], q["dosage"], q["times"], method=c["method"], ablate=c["ablate"],
                             perturb=c["perturb"], lanes_per_patient=1)
        (h * q["cot"]).sum().backward()
        got = _backward(c, q, h.detach())
        print("%s: gy0 bit-identical to the plain lane-per-patient adjoint: %s, gw: %s, gb: %s"
              % (cases.case_id(c), torch.equal(got[0], y0.grad), torch.equal(got[2], w.grad), torch.equal(got[3], b.grad)))
        assert cases.rel_l2(got[0], y0.grad) <= GRAD_TOL and cases.rel_l2(got[2], w.grad) <= GRAD_TOL and cases.rel_l2(got[3], b.grad) <= GRAD_TOL


# ------------------------------------------------------------------------------------------------------ model level
def _decoder_problem(dev):
    from hode import synth
    from oracle import vi as ovi
    T, B, D, obs, step = 12, 9, 8, 5, synth.STEP
    torch.manual_seed(5)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * step, step, method="rk4", device=dev)
    with torch.no_grad():
        dec.ode.ml_net[0].weight.mul_(2.0)
    dec_o = ovi.DecoderOracle(obs, D, (T - 1) * step, step, method="rk4")
    dec_o.load_state_dict({k: v.cpu() for k, v in dec.state_dict().items()})
    dec_o.double()
    inp = synth.solver_inputs(B, T, D, seed=9, n_dose=2)
    a = inp["actions"] / 2
    hit = a[..., 0] != 0
    for p in (0, 4):  # two patients with two EQUAL doses: the gradient still goes to one entry
        a[hit[:, p], p, 0] = 1.75
    cot = torch.randn(T, B, obs, generator=torch.Generator().manual_seed(6))
    return dec, dec_o, inp["z0"], a, cot


def _run(dec, z0, a, cot, switch):
    dec.ode.dose_grad = switch
    dec.ode.lanes_per_patient = 1
    for p in dec.parameters():
        p.grad = None
    act = a.clone().requires_grad_(True)
    x_hat, _ = dec(z0, act)
    loss = (x_hat * cot).sum()
    loss.backward()
    return loss.detach(), act.grad, {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}


def test_decoder_action_gradient_matches_the_float64_oracle_decoder():
    """Fails on the parent commit, where action.grad is None."""
    dev = _dev()
    dec, dec_o, z0, a, cot = _decoder_problem(dev)
    loss, ga, gp = _run(dec, z0.to(dev), a.to(dev), cot.to(dev), True)
    assert ga is not None, "action.grad is None: the solve returned no gradient for the dosage"
    torch.cuda.synchronize()
    act_o = a.double().requires_grad_(True)
    x_o, _ = dec_o(z0.double(), act_o)
    loss_o = (x_o * cot.double()).sum()
    loss_o.backward()
    B = a.shape[1]
    ga = ga.cpu()[..., 0]
    assert int((ga != 0).sum()) == B and bool(((ga != 0).sum(0) == 1).all())  # non-zero exactly at one entry per patient ...
    hot = (ga != 0).float().argmax(dim=0)
    assert torch.equal(a[hot, torch.arange(B), 0], a[..., 0].max(dim=0)[0])   # ... which holds the patient's maximum
    assert torch.equal((a[..., 0][:, [0, 4]] == 1.75).sum(0), torch.tensor([2, 2]))
    ref = act_o.grad[..., 0].sum(0)  # the oracle's torch.max routes to one entry too; per patient it is the same number
    assert int((act_o.grad != 0).sum()) == B
    err = cases.rel_l2(ga.sum(0), ref)
    print("decoder: action.grad rel-L2 %.2e, loss %.6e vs %.6e" % (err, float(loss), float(loss_o)))
    assert err <= GRAD_TOL, err
    # the loss and every parameter gradient: the same run with the switch off
    loss_off, ga_off, gp_off = _run(dec, z0.to(dev), a.to(dev), cot.to(dev), False)
    assert ga_off is None  # off: nothing behaves differently
    assert abs(float(loss) - float(loss_off)) <= GRAD_TOL * abs(float(loss_off)) and set(gp) == set(gp_off)
    for n in gp:
        if float(gp_off[n].norm()) == 0.0:
            assert not gp[n].any(), n
            continue
        assert cases.rel_l2(gp[n], gp_off[n]) <= GRAD_TOL, (n, cases.rel_l2(gp[n], gp_off[n]))


def test_decoder_with_step_size_and_perturb_options():
    """The solve stays the callable of substep.solve_with_step_size: sub-stepped and perturbed solves carry the gradient too."""
    import hode
    from oracle.solvers import odeint as oracle_odeint
    dev = _dev()
    dec, dec_o, z0, a, cot = _decoder_problem(dev)
    dec.ode.dose_grad = True
    for options in ({"step_size": dec.step_size / 2}, {"perturb": True}):
        act = a.to(dev).requires_grad_(True)
        dec.ode.set_action(act)
        h = hode.odeint(dec.ode, z0.to(dev), dec.t, method="midpoint", options=dict(options))
        (h * cot.to(dev)[..., :1]).sum().backward()
        act_o = a.double().requires_grad_(True)
        dec_o.ode.set_action(act_o)
        h_o = oracle_odeint(dec_o.ode, z0.double(), dec_o.t.double(), method="midpoint", options=dict(options))
        (h_o * cot.double()[..., :1]).sum().backward()
        err = cases.rel_l2(act.grad[..., 0].sum(0), act_o.grad[..., 0].sum(0))
        print("decoder %s: action.grad rel-L2 %.2e" % (options, err))
        assert err <= GRAD_TOL, (options, err)
