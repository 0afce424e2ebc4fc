"""Dose-table gradients of the real-data hybrid solve (libhode_real_dose.so, model._RocheRealDoseGrad,
RocheODEReal.dose_grad) against the float64 oracle with the action a leaf, against the plain backward of
libhode_real_dims.so, with sentinels around every output, under the tensors autograd really hands the binding, and at the
model level.  GPU only.  Cases, inputs and oracle: tests/real_dose_cases.py.

Bounds: gradients rel-L2 1e-4, the bound tests/test_hip_real.py and tests/test_hip_real_dims.py hold this arithmetic to
(the oracle's own fp32 run stays below a tenth of it: tests/test_real_dose_host.py); h is bit for bit real_solve's; model
level (test_config5_mirror_loss_matches_cpu_oracle_pipeline): loss 1e-4 relative, gradients rel-L2 2e-3."""
import copy
import ctypes

import pytest
import torch

import real_dose_cases as cases

pytestmark = pytest.mark.gpu
SENTINEL = -7.75e8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _on(p, dev):
    return dict(y0=p["y0"].to(dev), theta=p["theta"].to(dev), wflat=p["wflat"].to(dev), t=p["t"].to(dev),
                act=p["a"][..., 0].contiguous().to(dev), cot=p["cot"].to(dev))


def _solve(c, q, act, dose, leaves=True):
    """h on the case's output times through hode.substep, as RocheODEReal.hode_solve calls it: `dose` = the autograd function
    with the dose-table gradient, else the plain real_solve."""
    import model
    from hode import real, substep
    y0, theta, wflat = ((q[k].detach().clone().requires_grad_(True) if leaves else q[k]) for k in ("y0", "theta", "wflat"))
    if dose:
        fn = lambda grid: model._RocheRealDoseGrad.apply(y0, theta, wflat, grid, act, c["H"], c["method"], c["perturb"])  # noqa: E731
    else:
        fn = lambda grid: real.real_solve(y0, theta, wflat, grid, act, c["H"], method=c["method"], perturb=c["perturb"])  # noqa: E731
    return substep.solve_with_step_size(fn, q["t"], c["step_size"]), (y0, theta, wflat)


def _run(c, q, dose=True, act=None):
    """Forward + backward of sum(h * cot): dict(h, gact (None for the plain solve), gy0, gw, gth)."""
    act = q["act"].detach().clone().requires_grad_(True) if act is None else act
    h, (y0, theta, wflat) = _solve(c, q, act, dose)
    (h * q["cot"]).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), gact=act.grad if act.is_leaf else None, gy0=y0.grad, gw=wflat.grad, gth=theta.grad)


def _assert_vs_oracle(c, got, ref):
    what = cases.case_id(c)
    rels = {k: cases.rel_l2(got[k], ref[k]) for k in ("gy0", "gw", "gth")}
    zero = ref["gact"] == 0
    if not cases.never_dosed(c):
        rels["gact"] = cases.rel_l2(got["gact"], ref["gact"])
    print("%s: rel-L2 %s; exact zeros of the oracle: %d of %d" % (what, ", ".join("%s %.3e" % kv for kv in rels.items()),
                                                                  int(zero.sum()), zero.numel()))
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("h", "gact", "gy0", "gw", "gth")), what
    assert got["gact"].shape == ref["gact"].shape
    for k, v in rels.items():
        assert v <= cases.GRAD_TOL, (what, k, v)
    # exact zeros where the oracle has exact zeros (action rows at or after the last stage time; a grid that never reaches hour 1)
    assert bool((got["gact"].cpu()[zero] == 0).all()), what
    if cases.never_dosed(c):
        assert bool(zero.all())


# ---------------------------------------------------------------------------------------- 1. per case, against the oracle
@pytest.mark.parametrize("c", cases.CASES + cases.ZERO_CASES, ids=cases.case_id)
def test_gradients_vs_float64_oracle_and_h_is_real_solves(c):
    dev = _dev()
    _, p = cases.inputs(c)
    ref = cases.oracle(c)
    q = _on(p, dev)
    got = _run(c, q)
    plain = _run(c, q, dose=False)
    assert plain["gact"] is None
    assert torch.equal(got["h"], plain["h"]), "h is not bit for bit real_solve's"
    _assert_vs_oracle(c, got, ref)
    if c["grid"] == "unit":
        assert bool((got["gact"][-2:] == 0).all())  # hours 11 and 12
    if c["zero"]:
        col = got["gact"][:, cases.ZERO_PATIENT]
        assert not q["act"][:, cases.ZERO_PATIENT].any() and float(col.abs().max()) > 0
        assert cases.rel_l2(col, ref["gact"][:, cases.ZERO_PATIENT]) <= cases.GRAD_TOL
    if c["D"] in cases.PLAIN_DIMS:  # the plain backward of libhode_real_dims.so on the same inputs: inside the family bound of each other
        same = {k: bool(torch.equal(got[k], plain[k])) for k in ("gy0", "gw", "gth")}
        print("bit-identical to libhode_real_dims.so's backward: %s" % same)
        for k in ("gy0", "gw", "gth"):
            assert cases.rel_l2(got[k], plain[k]) <= cases.GRAD_TOL, (k, cases.rel_l2(got[k], plain[k]))


# ------------------------------------------------------------------------------------------------------------ 2. padding
def _guarded(n, dev, pad=64, fill=SENTINEL):
    whole = torch.full((n + 2 * pad,), SENTINEL, device=dev, dtype=torch.float32)
    inner = whole[pad:pad + n]
    inner.fill_(fill)
    return whole, inner


PADDING_CASES = [c for c in cases.CASES if (c["D"], c["H"], c["B"], c["grid"], c["step_size"]) in
                 ((5, 1, 17, "unit", None), (19, 43, 1, "unit", None), (20, 64, 16, "unit", None), (8, 43, 37, "offset+", None))]


@pytest.mark.parametrize("c", PADDING_CASES, ids=cases.case_id)
def test_nothing_is_written_outside_the_outputs_and_every_element_of_grad_act_is_written(c):
    """grad_act, grad_y0, the flat weight gradient and the workspace inside sentinel-filled buffers, through the C ABI (the
    binding allocates exact-size tensors); grad_act poisoned with NaN before the launch: every sentinel survives, every
    element inside is overwritten, and the values are the binding's."""
    dev = _dev()
    from hode import _lib as L, _real_dose_lib as DL
    from hode.real import real_solve
    from hode.real_dose import real_dose_backward
    assert len(PADDING_CASES) == 4
    _, p = cases.inputs(c)
    q = _on(p, dev)
    D, H, B, Ta, T = c["D"], c["H"], c["B"], cases.n_action_rows(c), q["t"].numel()
    with torch.no_grad():
        h = real_solve(q["y0"], q["theta"], q["wflat"], q["t"], q["act"], H, method=c["method"], perturb=c["perturb"])
    want = real_dose_backward(h, q["theta"], q["wflat"], q["t"], q["act"], q["cot"], H, method=c["method"], perturb=c["perturb"])
    lib = DL.lib()
    ga_all, ga = _guarded(Ta * B, dev, fill=float("nan"))
    gy_all, gy0 = _guarded(B * D, dev)
    gw_all, gw = _guarded(q["wflat"].numel(), dev, fill=0.0)   # the backward accumulates into it
    gth = torch.zeros(3, device=dev)
    d = DL.new_desc()
    d.method, d.perturb = L.METHODS[c["method"]], int(c["perturb"])
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times = B, D, H, T, Ta
    d.t, d.h, d.act, d.theta, d.wflat, d.grad_h = (x.data_ptr() for x in (q["t"], h, q["act"], q["theta"], q["wflat"], q["cot"]))
    d.grad_y0, d.grad_act, d.grad_wflat, d.grad_theta = gy0.data_ptr(), ga.data_ptr(), gw.data_ptr(), gth.data_ptr()
    n = lib.hode_real_dose_workspace_bytes(ctypes.byref(d))
    assert n > 0 and n % 256 == 0
    ws_all, ws = _guarded(n // 4, dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    assert ws.data_ptr() % 16 == 0
    DL.check(lib.hode_real_dose_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "hode_real_dose_bwd")
    torch.cuda.synchronize()
    pad = 64
    for name, whole in (("grad_act", ga_all), ("grad_y0", gy_all), ("grad_w", gw_all), ("workspace", ws_all)):
        assert bool((whole[:pad] == SENTINEL).all()) and bool((whole[-pad:] == SENTINEL).all()), name
    assert bool(torch.isfinite(ga).all()), "an element of grad_act was not written"
    assert bool(torch.isfinite(gy0).all()) and bool(torch.isfinite(gw).all())
    assert torch.equal(gy0.view(B, D), want[0]) and torch.equal(gth, want[1])
    assert torch.equal(gw, want[2]) and torch.equal(ga.view(Ta, B), want[3])


# --------------------------------------------------------------------------------------------- 3. repeats and isolation
ISOLATION_CASE = cases._c(9, 17, 37, "midpoint")
ISOLATION_RK4 = cases._c(19, 64, 37, "rk4")


@pytest.mark.parametrize("c", [ISOLATION_CASE, ISOLATION_RK4], ids=cases.case_id)
def test_two_repeats_are_bit_identical(c):
    dev = _dev()
    q = _on(cases.inputs(c)[1], dev)
    a, b = _run(c, q), _run(c, q)
    for k in ("gact", "gy0", "gw", "gth"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("c", [ISOLATION_CASE, ISOLATION_RK4], ids=cases.case_id)
def test_patient_0_alone_is_the_patient_at_any_position_of_a_batch(c):
    dev = _dev()
    q = _on(cases.inputs(c)[1], dev)
    assert c["B"] == 37
    solo = _run(c, dict(q, y0=q["y0"][:1], act=q["act"][:, :1].contiguous(), cot=q["cot"][:, :1].contiguous()))
    for pos in (0, 15, 16, 36):
        perm = list(range(37))
        perm[0], perm[pos] = perm[pos], perm[0]
        got = _run(c, dict(q, y0=q["y0"][perm], act=q["act"][:, perm].contiguous(), cot=q["cot"][:, perm].contiguous()))
        assert torch.equal(got["gact"][:, pos], solo["gact"][:, 0]), pos
        assert torch.equal(got["gy0"][pos], solo["gy0"][0]), pos


@pytest.mark.parametrize("c", [ISOLATION_CASE, ISOLATION_RK4], ids=cases.case_id)
def test_a_nan_start_state_stays_with_its_patient(c):
    dev = _dev()
    q = _on(cases.inputs(c)[1], dev)
    clean = _run(c, q)
    for bad in (0, 17, 36):
        y0 = q["y0"].clone()
        y0[bad] = float("nan")
        got = _run(c, dict(q, y0=y0))
        keep = [i for i in range(c["B"]) if i != bad]
        assert torch.equal(got["gact"][:, keep], clean["gact"][:, keep]), bad
        assert torch.equal(got["gy0"][keep], clean["gy0"][keep]), bad
        assert not bool(torch.isfinite(got["gy0"][bad]).all())


# ----------------------------------------------------------------------- 4. the tensors autograd really hands the binding
PRES_CASE = cases._c(12, 43, 33, "midpoint")


def _reference(c, q, cot):
    """The contiguous call: (h, (grad_y0, grad_theta, grad_wflat, grad_act))."""
    from hode.real import real_solve
    from hode.real_dose import real_dose_backward
    with torch.no_grad():
        h = real_solve(q["y0"], q["theta"], q["wflat"], q["t"], q["act"], c["H"], method=c["method"], perturb=c["perturb"])
    out = real_dose_backward(h, q["theta"], q["wflat"], q["t"], q["act"], cot.contiguous(), c["H"], method=c["method"], perturb=c["perturb"])
    torch.cuda.synchronize()
    return h, out


def _assert_same(got, want):
    for k, w in zip(("gy0", "gth", "gw", "gact"), want):
        assert torch.equal(got[k], w), k


def test_an_expanded_cotangent():
    dev = _dev()
    c = PRES_CASE
    q = _on(cases.inputs(c)[1], dev)
    act = q["act"].clone().requires_grad_(True)
    h, (y0, theta, wflat) = _solve(c, q, act, True)
    row = q["cot"][0]
    (h.sum(0) * row).sum().backward()   # grad_h = row expanded over time: stride 0
    torch.cuda.synchronize()
    _assert_same(dict(gy0=y0.grad, gth=theta.grad, gw=wflat.grad, gact=act.grad), _reference(c, q, row[None].expand_as(q["cot"]))[1])


def test_a_strided_grad_h():
    dev = _dev()
    c = PRES_CASE
    q = _on(cases.inputs(c)[1], dev)
    act = q["act"].clone().requires_grad_(True)
    h, (y0, theta, wflat) = _solve(c, q, act, True)
    cot_bt = q["cot"].permute(1, 0, 2).contiguous()
    (h.permute(1, 0, 2) * cot_bt).sum().backward()   # grad_h arrives as a permuted view of a (B, T, D) tensor
    torch.cuda.synchronize()
    _assert_same(dict(gy0=y0.grad, gth=theta.grad, gw=wflat.grad, gact=act.grad), _reference(c, q, q["cot"])[1])


def test_a_side_stream():
    dev = _dev()
    c = PRES_CASE
    q = _on(cases.inputs(c)[1], dev)
    want = _reference(c, q, q["cot"])[1]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(c, q)
    side.synchronize()
    _assert_same(got, want)


def test_a_non_leaf_action():
    dev = _dev()
    c = PRES_CASE
    q = _on(cases.inputs(c)[1], dev)
    want = _reference(c, q, q["cot"])[1]
    leaf = (q["act"] / 2).clone().requires_grad_(True)
    got = _run(c, q, act=2 * leaf)
    assert torch.equal(2 * leaf.detach(), q["act"])
    got["gact"] = leaf.grad
    _assert_same(got, want[:3] + (2 * want[3],))


def test_the_binding_refuses_what_it_does_not_serve():
    dev = _dev()
    import hode
    from hode.real_dose import real_dose_backward
    c = PRES_CASE
    q = _on(cases.inputs(c)[1], dev)
    h, _ = _reference(c, q, q["cot"])
    args = (h, q["theta"], q["wflat"], q["t"], q["act"], q["cot"], c["H"])
    with pytest.raises(hode.HodeConfigError, match="not a fixed-grid method"):
        real_dose_backward(*args, method="dopri5")
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        real_dose_backward(h.cpu(), *args[1:])
    with pytest.raises(hode.HodeConfigError, match=r"wflat \(\d+,\) expected"):
        real_dose_backward(h, q["theta"], q["wflat"][:-1], *args[3:])


# -------------------------------------------------------------------------------------------------------- 5. model level
def _decoders(D, ode_step_div, dev):
    """A hybrid DecoderReal on the GPU and its CPU float64 copy on the oracle solver; DDW-shaped inputs."""
    import model
    from oracle.solvers import odeint as oracle_odeint
    obs, act, stat, T, t0, B = 24, 1, 11, 40, 24, 33
    hidden = int((obs + act + stat) * 1.2)
    assert hidden == 43
    torch.manual_seed(3 + D)
    cpu = torch.device("cpu")
    dec_c = model.DecoderReal(obs, D, act, stat, hidden, T, 1, method="midpoint", ode_step_size=1.0 / ode_step_div, ode_type="hybrid",
                              t0=t0, device=cpu)
    dec_g = copy.deepcopy(dec_c).to(dev)
    dec_g.device = dec_g.ode.device = dev
    dec_g.t = dec_g.t.to(dev)
    dec_g.options["step_t"] = dec_g.t
    dec_g._odeint = model.hode.odeint
    dec_c = dec_c.double()
    dec_c.t = dec_c.t.double()
    dec_c.options["step_t"] = dec_c.t
    dec_c._odeint = oracle_odeint
    gen = torch.Generator().manual_seed(4)
    data = dict(x=torch.randn(T - t0, B, obs, generator=gen), mask=(torch.rand(T - t0, B, obs, generator=gen) < 0.5).float(),
                a=(torch.rand(T, B, 1, generator=gen) < 0.1).float() * torch.rand(T, B, 1, generator=gen),
                s=torch.rand(T, B, stat, generator=gen), init=torch.randn(B, D, generator=gen) * 0.3)
    return dec_g, dec_c, data


def _loss(dec, data, dev, dtype, needs_grad=True):
    """Masked squared error of x_hat with the action a leaf: (loss, x_hat, action)."""
    import warnings
    d = {k: v.to(device=dev, dtype=dtype) for k, v in data.items()}
    a = d["a"].requires_grad_(needs_grad)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # the oracle warns about step_t like torchdiffeq
        x_hat = dec(d["init"], a, d["s"])[0]
    loss = ((x_hat - d["x"]) ** 2 * d["mask"]).sum() / d["x"].shape[1]
    return loss, x_hat, a


@pytest.mark.parametrize("ode_step_div", cases.MODEL_STEP_DIVS)
@pytest.mark.parametrize("D", cases.MODEL_DIMS)
def test_decoder_real_fills_action_grad(D, ode_step_div):
    """decoder.ode.dose_grad = True is all a user sets: action.grad and the parameter gradients against the same decoder in
    float64 on the CPU with the oracle solver."""
    dev = _dev()
    dec_g, dec_c, data = _decoders(D, ode_step_div, dev)
    dec_g.ode.dose_grad = True
    lg, _, ag = _loss(dec_g, data, dev, torch.float32)
    lg.backward()
    torch.cuda.synchronize()
    assert ag.grad is not None, "the action received no gradient"
    lc, _, ac = _loss(dec_c, data, torch.device("cpu"), torch.float64)
    lc.backward()
    print("loss gpu %.8e cpu %.8e; action.grad rel-L2 %.3e, non-zero %.2f" % (lg.item(), lc.item(), cases.rel_l2(ag.grad, ac.grad),
                                                                              float((ag.grad != 0).float().mean())))
    assert abs(lg.item() - lc.item()) <= 1e-4 * abs(lc.item())
    assert ag.grad.shape == ac.grad.shape and bool(torch.isfinite(ag.grad).all()) and float(ac.grad.norm()) > 0
    assert cases.rel_l2(ag.grad, ac.grad) <= 2e-3
    assert bool((ag.grad.cpu()[ac.grad == 0] == 0).all())
    checked = 0
    for (n, pg), (_, pc) in zip(dec_g.named_parameters(), dec_c.named_parameters()):
        if pc.grad is None or float(pc.grad.abs().max()) < 1e-10:
            continue
        print("%s rel-L2 %.3e" % (n, cases.rel_l2(pg.grad, pc.grad)))
        assert cases.rel_l2(pg.grad, pc.grad) <= 2e-3, (n, cases.rel_l2(pg.grad, pc.grad))
        checked += 1
    assert checked > 10


@pytest.mark.parametrize("D", cases.MODEL_DIMS)
def test_with_the_switch_off_nothing_changes(D):
    dev = _dev()
    dec_g, _, data = _decoders(D, 2, dev)
    assert dec_g.ode.dose_grad is False
    l_off, x_off, a_off = _loss(dec_g, data, dev, torch.float32)
    l_off.backward()
    g_off = [p.grad.clone() for p in dec_g.parameters() if p.grad is not None]
    assert a_off.grad is None
    dec_g.zero_grad(set_to_none=True)
    dec_g.ode.dose_grad = True
    l_on, x_on, a_on = _loss(dec_g, data, dev, torch.float32)
    l_on.backward()
    torch.cuda.synchronize()
    assert a_on.grad is not None and torch.equal(x_on, x_off)
    g_on = [p.grad for p in dec_g.parameters() if p.grad is not None]
    assert len(g_on) == len(g_off)
    print("parameter gradients bit-identical to the plain backward: %s" % [bool(torch.equal(a, b)) for a, b in zip(g_on, g_off)])
    # switch on, no grad asked of the action: the plain path, bit for bit
    dec_g.zero_grad(set_to_none=True)
    l_no, x_no, a_no = _loss(dec_g, data, dev, torch.float32, needs_grad=False)
    l_no.backward()
    torch.cuda.synchronize()
    assert a_no.grad is None and torch.equal(x_no, x_off)
    for a, b in zip([p.grad for p in dec_g.parameters() if p.grad is not None], g_off):
        assert torch.equal(a, b)
