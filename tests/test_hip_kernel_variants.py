"""Every compiled instantiation of the solver and decoder kernel families against a float64 reference.  GPU only.

One test per entry of tests/kernel_variants.py's CASES (tests/test_kernel_variant_coverage.py checks that the table reaches
every instantiation the build contains).  References: the eager restatements (tests/seqdec_eager.py,
tests/neural_real_eager.py) and oracle.rhs + oracle.solvers, with parameters, state, grid and dose times cast to double
from the exact fp32 values the kernels read (the grids are dyadic / integral, so no fp64 stage time falls on the other
side of a dose time than its fp32 twin).  Tolerances as the rest of the suite: trajectory 2e-5 (1 + max|h|), gradients
rel-L2 1e-4 (2e-4 for the real-data neural ODEs).

need_theta=False (theta not a leaf: frozen expert parameters, bench.py's inputs) selects its own backward instantiations;
their grad_y0 / grad_w / grad_b are checked against fp64 and against the same call with need_theta=True (_same_as_with_theta):
the theta accumulation is separate work that feeds nothing else.

The Roche and dopri5 cases also name the rhs body each kernel runs (kv.body): the theta vector and the number of dose times
per patient are part of the problem, and grad_theta is compared per component as well as a vector."""
import copy
import functools
import warnings

import pytest
import torch

import kernel_variants as kv
import neural_real_eager

pytestmark = pytest.mark.gpu

OBS, ACT, STAT, HIDDEN = 24, 1, 11, 43


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _traj_ok(h, ref):
    h, ref = h.detach().double().cpu(), ref.detach().double().cpu()
    assert h.shape == ref.shape
    err = (h - ref).abs().max().item()
    assert err <= 2e-5 * (1 + ref.abs().max().item()), err


def _family(name):
    return [c for c in kv.CASES if c["family"] == name]


def _same_as_with_theta(a, b, exact, what):
    """need_theta=False against need_theta=True.  Bit-identical where the two instantiations compile the shared work
    identically: the split layout (the theta work runs on a wave of its own) and the fixed-grid kernels of the ablate rhs
    (its theta terms are products the state VJP does not share).  The lane / MFMA kernels of the full Roche rhs share
    subexpressions between the state VJP and the theta VJP (dis * imm^HillCure, the Hill fraction of the pathogen term);
    without the theta consumers the compiler contracts them into different fmas, which moves grad_y0 / grad_w / grad_b by
    an ulp or two (rel-L2 ~ 4e-8 measured); the dopri5 backward does the same for both rhs kinds (8e-8 at D = 4, ablate).
    There the check is rel-L2 <= 1e-6: far below the 1e-4 fp64 tolerance, far above rounding noise, and any real coupling
    of the theta work into the other gradients breaks it."""
    if exact:
        assert torch.equal(a, b), (what, _rel(a, b))
    else:
        assert _rel(a, b) <= 1e-6, (what, _rel(a, b))


# ------------------------------------------------------------------------------------------------------------ seqdec
@pytest.mark.parametrize("case", _family("seqdec"), ids=kv.case_id)
def test_seqdec(case):
    """model.DecoderRealBenchmark (tlstm / gruode) vs tests/seqdec_eager.py in fp64 (the comparison of test_hip_seqdec)."""
    from test_hip_seqdec import _compare_with_eager, _inputs
    dev = _dev()
    Ta = case["t0"] + 1 if case["t0"] >= 20 else 20
    dec, init, a, s, cot = _inputs(case["kind"], case["D"], case["B"], Ta, case["t0"], 1000 + 10 * case["D"] + case["B"], dev)
    if case["t0"] == Ta - 1:
        assert dec.t.numel() == 1
    _compare_with_eager(dec, init, a, s, cot)


# ------------------------------------------------------------------------------------------------------- neural-real
def _neural_real(kind, D, method, H, B, perturb, div, dev, t0=3, t_end=9, Ta=7, seed=0):
    import hode
    import model
    gen = torch.Generator().manual_seed(seed)
    cls = model.NeuralODEReal if kind == "neural" else model.NeuralODEReal2nd
    torch.manual_seed(seed)
    ode = cls(D, ACT, STAT, H, t_end, 1, device=dev)
    y0 = torch.randn(B, D, generator=gen) * 0.5
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen) * 2
    t = torch.arange(t0 - 1, t_end, 1.0)
    cot = torch.randn(t.numel(), B, D, generator=gen)
    ode.set_action_static(a.to(dev), None)
    yg = y0.to(dev).requires_grad_(True)
    h = hode.odeint(ode, yg, t.to(dev), method=method, options={"step_size": 1.0 / div, "perturb": perturb})
    (h * cot.to(dev)).sum().backward()
    got = [yg.grad] + [p.grad for p in ode.ml_net.parameters()]
    ps = [p.detach().cpu().double().requires_grad_(True) for p in ode.ml_net.parameters()]
    yc = y0.double().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hc, _ = neural_real_eager.solve(kind, yc, *ps, a.double(), t.double(), method, step_size=1.0 / div, perturb=perturb)
    (hc * cot.double()).sum().backward()
    return h, hc, got, [yc.grad] + [p.grad for p in ps]


@pytest.mark.parametrize("case", _family("neural_real"), ids=kv.case_id)
def test_neural_real(case):
    h, hc, got, want = _neural_real(case["kind"], case["D"], case["method"], case["H"], case["B"], case["perturb"],
                                    case["div"], _dev(), seed=case["D"] + case["H"])
    _traj_ok(h, hc)
    for name, g, w in zip(("y0", "w1", "b1", "w2", "b2"), got, want):
        assert _rel(g, w) < 2e-4, (name, _rel(g, w))


@pytest.mark.parametrize("kind,D", [("neural", 16), ("2nd", 32)])
def test_neural_real_decoder_loss(kind, D):
    """DecoderReal (readout included) in the new tile classes: sum(x_hat * cot) and every gradient against fp64."""
    import model
    dev = _dev()
    gen = torch.Generator().manual_seed(D)
    torch.manual_seed(D)
    B, TMAX, t0 = 37, 16, 8
    dec = model.DecoderReal(OBS, D, ACT, STAT, 17, TMAX, 1, t0=t0, method="rk4", ode_step_size=0.5, ode_type=kind, device=dev)
    init = torch.randn(B, D, generator=gen) * 0.5
    a = (torch.rand(TMAX, B, 1, generator=gen) < 0.3).float() * torch.rand(TMAX, B, 1, generator=gen)
    ig = init.to(dev).requires_grad_(True)
    x_hat, h = dec(ig, a.to(dev), None)
    cot = torch.randn(*x_hat.shape, generator=gen)
    (x_hat * cot.to(dev)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in dec.state_dict().items()}
    i64 = init.double().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xr, hr, _ = neural_real_eager.decoder(kind, sd, i64, a.double(), dec.t.cpu().double(), "rk4", 0.5)
    (xr * cot.double()).sum().backward()
    _traj_ok(h, hr)
    _traj_ok(x_hat, xr)
    assert _rel(ig.grad, i64.grad) < 2e-4
    for n, p in dec.named_parameters():
        assert _rel(p.grad, sd[n].grad) < 2e-4, n


# -------------------------------------------------------------------------------------------------- real (config 5)
def _real_flat(f):
    ps = [f.dx1_net[0].weight, f.dx1_net[0].bias, f.dx1_net[2].weight, f.dx1_net[2].bias,
          f.dx2_net[0].weight, f.dx2_net[0].bias, f.dx2_net[2].weight, f.dx2_net[2].bias]
    if f.ml_dim > 0:
        ps += [f.lin_hh.weight, f.lin_hz.weight, f.lin_hr.weight]
    return ps


@functools.lru_cache(maxsize=None)
def _real_problem(D, H, method, perturb=True, B=37, Ta=12, t0=4):
    """Inputs and the fp64 oracle (h, grad_y0, flat weight gradient, theta gradient) of sum(h * cot)."""
    from oracle.rhs import RocheRealRHS
    from oracle.solvers import odeint as oracle_odeint
    gen = torch.Generator().manual_seed(D + H)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.2).float() * torch.rand(Ta, B, 1, generator=gen)
    t = torch.arange(t0 - 1, Ta, 1, dtype=torch.float32)
    y0 = torch.randn(B, D, generator=gen) * 0.3
    cot = torch.randn(t.numel(), B, D, generator=gen)
    f64 = copy.deepcopy(f).double()
    f64.set_action_static(a.double())
    y64 = y0.double().requires_grad_(True)
    ho = oracle_odeint(f64, y64, t.double(), method=method, options={"perturb": perturb, "step_size": 1.0})
    (ho * cot.double()).sum().backward()
    ref = dict(h=ho.detach(), gy0=y64.grad, gw=torch.cat([p.grad.reshape(-1) for p in _real_flat(f64)]),
               gth=torch.stack([f64.k_immunity.grad, f64.kel.grad, f64.kel2.grad]))
    wflat = torch.cat([p.detach().reshape(-1) for p in _real_flat(f)])
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return dict(y0=y0, a=a, t=t, cot=cot, wflat=wflat, theta=theta, perturb=perturb), ref


def _real_gpu(p, H, method, dev):
    from hode.real import real_solve
    wflat = p["wflat"].to(dev).requires_grad_(True)
    theta = p["theta"].to(dev).requires_grad_(True)
    y0 = p["y0"].to(dev).requires_grad_(True)
    h = real_solve(y0, theta, wflat, p["t"].to(dev), p["a"][..., 0].to(dev), H, method=method, perturb=p["perturb"])
    (h * p["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), gy0=y0.grad, gw=wflat.grad, gth=theta.grad)


def _real_gpu_tape_backward(p, H, method, dev):
    """The matrix-core backward without grad_w1 (C ABI): the variant that writes the GEMM operand tape instead of folding
    the weight gradients on chip.  The tape is contracted into the flat weight gradient exactly as hode/real.py does for
    the tape-writing kernels (hode.real.contract_tape), so a wrong tape row, stride or hidden-row bound shows in gw."""
    import hode
    from hode import _lib as L
    from hode.real import _desc, contract_tape, real_solve
    lib = hode.lib()
    y0, wflat, theta = p["y0"].to(dev), p["wflat"].to(dev), p["theta"].to(dev)
    t, act = p["t"].to(dev), p["a"][..., 0].contiguous().to(dev)
    h = real_solve(y0, theta, wflat, t, act, H, method=method, perturb=p["perturb"]).detach()
    gh = p["cot"].to(dev).contiguous()
    gy0 = torch.empty_like(y0)
    gth = torch.zeros(L.N_THETA, device=dev)
    d = _desc(h[0], t, act, theta, wflat, h, L.METHODS[method], p["perturb"], H)
    d.grad_h, d.grad_y0, d.grad_theta = gh.data_ptr(), gy0.data_ptr(), gth.data_ptr()
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    L.check(lib.hode_rk_bwd(d, torch.cuda.current_stream().cuda_stream), "hode_rk_bwd[real, tape]")
    gw = contract_tape(ws, t.numel(), y0.shape[0], y0.shape[1], H, L.METHODS[method])
    torch.cuda.synchronize()
    return dict(h=h, gy0=gy0, gw=gw, gth=gth[:3])


@pytest.mark.parametrize("case", _family("real"), ids=kv.case_id)
def test_real(case, monkeypatch):
    monkeypatch.delenv("HODE_REAL_LAYOUT", raising=False)
    dev = _dev()
    D, H, method = case["D"], case["H"], case["method"]
    p, ref = _real_problem(D, H, method)
    got = _real_gpu(p, H, method, dev) if case["onchip"] else _real_gpu_tape_backward(p, H, method, dev)
    _traj_ok(got["h"], ref["h"])
    for k in ("gy0", "gw", "gth"):
        assert _rel(got[k], ref[k]) <= 1e-4, (k, _rel(got[k], ref[k]))
    if D == 20 and H > 64:
        # past the matrix-core range the default takes hode_real.hip: the same numbers as forcing that layout
        monkeypatch.setenv("HODE_REAL_LAYOUT", "t")
        forced = _real_gpu(p, H, method, dev)
        for k in ("h", "gy0", "gw", "gth"):
            assert torch.equal(got[k], forced[k]), k


# ------------------------------------------------------------------------------------------- Roche fixed grid (all layouts)
# Every Roche kernel runs one of three rhs bodies per launch (kv.roche_body): hill2_k1 (both Hill exponents exactly 2, one
# dose per patient), hill2_kn (exponents 2, a loop over K dose times) and general (powf, and log_f32 in the Hill-exponent
# gradients).  Each case's body is kv.body(case); theta, K and the inputs are part of the fp64 problem's key.
def _theta_names(ablate):
    from oracle.rhs import THETA_NAMES
    return list(THETA_NAMES) + (["theta_1", "theta_2"] if ablate else [])


def _roche_setup(D, ablate, N, T, seed, theta=kv.THETA_DEFAULT, n_dose=1, neg_imm=False):
    from hode import synth
    from oracle.rhs import RocheRHS
    inp = synth.solver_inputs(N, T, D, seed=seed, n_dose=n_dose)
    if n_dose > 1:  # Dose(t) sums K decays of the patient's largest dose: keep it at one dose's scale, or the -Dose2 * ir
        inp["actions"] /= n_dose  # term drives ir below zero inside a stage and ir ** HillPatho's log (grad theta) is NaN
    if neg_imm:  # every other patient starts with a negative Immunity (the base of imm ** HillCure)
        inp["z0"][::2, 2] = -0.05 - inp["z0"][::2, 2]
    torch.manual_seed(seed)
    f = RocheRHS(D, synth.STEP, ablate=ablate, theta=theta)
    if D > 4:
        with torch.no_grad():  # larger weights than default init so that the learned block matters
            f.ml_net[0].weight.mul_(2.0)
    return inp, f


def _problem_key(case):
    return (case.get("theta", "default"), case.get("hill"), case["n_dose"], bool(case.get("neg_imm")))


@functools.lru_cache(maxsize=None)
def _roche_problem(D, method, ablate, key=("default", None, 1, False)):
    """Inputs and the fp64 oracle of sum(h * cot) for one (D, method, rhs, theta, K): shared by every layout and flag.
    theta is the fp32 vector the kernels read, cast to double by the oracle's .double()."""
    from oracle.rhs import dose_schedule
    from oracle.solvers import odeint as oracle_odeint
    th_name, hill, n_dose, neg_imm = key
    theta = kv.theta_of(dict(theta=th_name, hill=hill))
    N, T = kv.ROCHE_N, kv.ROCHE_T
    inp, f = _roche_setup(D, ablate, N, T, seed=100 + D + 7 * ablate, theta=theta, n_dose=n_dose, neg_imm=neg_imm)
    cot = torch.randn(T, N, D, generator=torch.Generator().manual_seed(D))
    f.set_action(inp["actions"])
    f64 = copy.deepcopy(f).double()
    f64.dosage, f64.times = f.dosage.double(), f.times.double()
    y64 = inp["z0"].double().requires_grad_(True)
    h = oracle_odeint(f64, y64, inp["t"].double(), method=method)
    (h * cot.double()).sum().backward()
    zero = torch.zeros((), dtype=torch.float64)
    ref = dict(h=h.detach(), gy0=y64.grad,
               gth=torch.stack([getattr(f64, n).grad if getattr(f64, n).grad is not None else zero for n in _theta_names(ablate)]))
    if D > 4:
        ref["gw"], ref["gb"] = f64.ml_net[0].weight.grad, f64.ml_net[0].bias.grad
    dosage, times = dose_schedule(inp["actions"], f.step_size)
    assert times.shape[1] == n_dose
    theta = torch.stack([getattr(f, n).detach().reshape(()) for n in _theta_names(ablate)])
    w = f.ml_net[0].weight.detach() if D > 4 else None
    b = f.ml_net[0].bias.detach() if D > 4 else None
    return dict(y0=inp["z0"], t=inp["t"], dosage=dosage, times=times, theta=theta, w=w, b=b, cot=cot), ref


def _roche_plan(p, dev, method, ablate, lanes, need_theta, tape):
    from hode import _lib as L
    from hode.plan import RocheRKPlan
    theta = torch.zeros(L.N_THETA)
    theta[: p["theta"].numel()] = p["theta"]
    opt = lambda x: None if x is None else x.to(dev)  # noqa: E731
    plan = RocheRKPlan(p["y0"].to(dev), theta.to(dev), opt(p["w"]), opt(p["b"]), p["t"].to(dev), p["dosage"].to(dev),
                       p["times"].to(dev), method=method, ablate=ablate, lanes_per_patient=lanes,
                       need_theta_grad=need_theta, tape=tape)
    plan.grad_h.copy_(p["cot"])
    plan.forward()
    gy0, _ = plan.backward()
    torch.cuda.synchronize()
    out = dict(h=plan.h.clone(), gy0=gy0.clone())
    if plan.grad_w is not None:
        out["gw"], out["gb"] = plan.grad_w.clone(), plan.grad_b.clone()
    if need_theta:
        out["gth"] = plan.grad_theta[: p["theta"].numel()].clone()
    return out


def _ref_finite(case, ref):
    """The fp64 reference is finite everywhere, except in the negative-base case: there HillCure's gradient is
    x ** p * log(x) with x < 0 (torch pow_backward_exponent), NaN, while the trajectory and every other gradient stay finite."""
    for k, v in ref.items():
        if case.get("neg_imm") and k == "gth":
            assert torch.isnan(v[0]) and torch.isfinite(v[2:]).all(), v
        else:
            assert torch.isfinite(v).all(), (k, v)


def _grad_ok(k, g, r, tol=1e-4):
    """rel-L2 against the fp64 reference; a NaN the reference has (negative base, _ref_finite) the kernel must have at
    exactly the same positions, and the rest is compared as usual."""
    g, r = g.double().flatten().cpu(), r.double().flatten().cpu()
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(g), nan), (k, g, r)
    err = _rel(g[~nan], r[~nan])
    assert err <= tol, (k, err)
    return err


def _theta_components_ok(g, r, floor=None):
    """grad_theta per component: |g_i - r_i| <= 1e-4 |r_i| + 1e-6 ||r||_2.  The Hill-exponent components are a small part
    of ||r|| (grad kel dominates it), so the vector rel-L2 alone would let an error in them through.  The fp32 CPU oracle
    on the fixed-grid problems of this file (every D, method, theta, K) sits at most 0.08 of this bound from fp64.
    `floor` (per component) widens it where the fp32 evaluation of the same graph is itself further away (dopri5 with the
    first step size attached, see test_dopri5_backward)."""
    g, r = g.double().flatten().cpu(), r.double().flatten().cpu()
    ok = torch.isfinite(r)
    g, r = g[ok], r[ok]
    bound = 1e-4 * r.abs() + 1e-6 * r.norm()
    if floor is not None:
        bound = torch.maximum(bound, floor[ok])
    bad = ((g - r).abs() > bound).nonzero().flatten().tolist()
    assert not bad, [(i, float(g[i]), float(r[i]), float(bound[i])) for i in bad]
    return float(((g - r).abs() / bound).max()) if r.numel() else 0.0


HILL_ULP_TOL = 1e-5  # rel-L2 between the general body at HillCure = 2 + 2^-22 and the x * x body at 2.0


@pytest.mark.parametrize("case", _family("roche"), ids=kv.case_id)
def test_roche_fixed_grid(case, monkeypatch, record_property):
    monkeypatch.delenv("HODE_RK_LAYOUT", raising=False)  # lanes = 0 must take the layout kv.roche_layout restates
    dev = _dev()
    D, method, ablate = case["D"], case["method"], case["ablate"]
    p, ref = _roche_problem(D, method, ablate, _problem_key(case))
    _ref_finite(case, ref)
    got = _roche_plan(p, dev, method, ablate, case["lanes"], case["need_theta"], case["tape"])
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    _traj_ok(got["h"], ref["h"])
    record_property("body", kv.body(case))
    record_property("err_h", (got["h"].double().cpu() - ref["h"]).abs().max().item() / (1 + ref["h"].abs().max().item()))
    for k in ("gy0", "gw", "gb", "gth"):
        if k in got:
            record_property("err_" + k, _grad_ok(k, got[k], ref[k]))
    if "gth" in got:
        record_property("err_gth_comp", _theta_components_ok(got["gth"], ref["gth"]))
    if not case["need_theta"]:
        with_th = _roche_plan(p, dev, method, ablate, case["lanes"], True, case["tape"])
        assert torch.equal(got["h"], with_th["h"])
        split = kv.roche_layout(D, case["lanes"], kv.ROCHE_T) == "split"
        for k in ("gy0", "gw", "gb"):
            if k in got:
                _same_as_with_theta(got[k], with_th[k], split or ablate, k)
    if case["theta"] == "hill_ulp":
        # the same call with HillCure exactly 2 runs the x * x body: continuous across the switch
        p2 = dict(p, theta=p["theta"].clone())
        p2["theta"][0] = 2.0
        assert kv.roche_body(ablate, float(p2["theta"][0]), float(p2["theta"][1]), case["n_dose"]) == "hill2_k1"
        at2 = _roche_plan(p2, dev, method, ablate, case["lanes"], case["need_theta"], case["tape"])
        for k in got:
            assert _rel(got[k], at2[k]) <= HILL_ULP_TOL, (k, _rel(got[k], at2[k]))


# ------------------------------------------------------------------------------------------------------------ dopri5
def _dp_gpu(inp, f, dev, lanes, need_theta, detach=True):
    from hode import adaptive
    from hode.solver import pack_theta
    from oracle.rhs import dose_schedule
    scal = [getattr(f, n).detach().clone().to(dev).requires_grad_(need_theta) for n in _theta_names(f.ablate)]
    y0 = inp["z0"].to(dev).requires_grad_(True)
    w = b = None
    if f.ml_dim > 0:
        w = f.ml_net[0].weight.detach().clone().to(dev).requires_grad_(True)
        b = f.ml_net[0].bias.detach().clone().to(dev).requires_grad_(True)
    dosage, times = dose_schedule(inp["actions"], f.step_size)
    h = adaptive.roche_dopri5(y0, pack_theta(scal, dev), w, b, inp["t"].to(dev), dosage.to(dev), times.to(dev), rtol=1e-7,
                              atol=1e-8, ablate=f.ablate, lanes_per_patient=lanes, detach_first_step=detach)
    tape = adaptive.read_tape()
    (h * inp["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = dict(h=h.detach().cpu(), gy0=y0.grad.cpu())
    if w is not None:
        out["gw"], out["gb"] = w.grad.cpu(), b.grad.cpu()
    if need_theta:
        out["gth"] = torch.stack([s.grad for s in scal]).cpu()
    return out, tape


def _dp_case(case, dev, hill_cure=None):
    """One dopri5 case: (the need_theta call, the other need_theta call, tape, inputs, rhs)."""
    from hode import adaptive
    D, ablate = case["D"], case["ablate"]
    theta = kv.theta_of(case)
    if hill_cure is not None:
        theta = (hill_cure,) + theta[1:]
    inp, f = _roche_setup(D, ablate, kv.DOPRI5_N, kv.DOPRI5_T, seed=40 + D + 5 * ablate, theta=theta, n_dose=case["n_dose"])
    inp["cot"] = torch.randn(kv.DOPRI5_T, kv.DOPRI5_N, D, generator=torch.Generator().manual_seed(3))
    adaptive.keep_workspace = True
    try:
        got, tape = _dp_gpu(inp, f, dev, case["lanes"], case["need_theta"], case["detach"])
        other, _ = _dp_gpu(inp, f, dev, case["lanes"], not case["need_theta"], case["detach"])
    finally:
        adaptive.keep_workspace = False
    return got, other, tape, inp, f


@pytest.mark.parametrize("case", _family("dopri5"), ids=kv.case_id)
def test_dopri5_backward(case, record_property):
    """The dopri5 forward (dp_fwd_kernel, all three phases), the backward sweep (dp_bwd_kernel) and, with the first step
    size attached, its backward (dp_initbwd_kernel passes 1 and 2) against the oracle's dopri5 step algebra replayed in
    fp64 along the kernel's own tape (test_hip_dopri5's tape-replay oracle), grad_theta included; and need_theta=False
    against need_theta=True.

    First step detached: every gradient to rel-L2 1e-4.  Attached: d loss / d dt_0 is a cancellation-heavy fp32 sum (the
    fp32 evaluation of the same graph on the same tape sits 1e-5 .. 7e-4 from fp64, test_hip_dopri5's case (b)), so there a
    gradient is held to 1e-4 or to twice the fp32 replay's own distance from fp64 where that is larger, per vector and per
    theta component."""
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
    record_property("err_h", (got["h"].double() - ref["h"]).abs().max().item() / (1 + ref["h"].abs().max().item()))
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
    if case["theta"] == "hill_ulp":
        at2, _, tape2, _, _ = _dp_case(case, dev, hill_cure=2.0)
        assert len(tape2["t"]) == len(tape["t"])
        for k in got:
            assert _rel(got[k], at2[k]) <= HILL_ULP_TOL, (k, _rel(got[k], at2[k]))
