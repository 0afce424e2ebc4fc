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
from reference_checks import (GRAD_TOL, LSTM_C_TOL, LSTM_H_TOL, NEURAL_DOPRI5_TRAJ_TOL, NEURAL_REAL_GRAD_TOL, READOUT_MLP_GRAD_TOL,
                              READOUT_TOL, TRAJ_TOL)

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
    assert err <= TRAJ_TOL * (1 + ref.abs().max().item()), err


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
def _neural_real(kind, D, method, H, B, perturb, div, dev, t0=3, t_end=9, Ta=7, seed=0, t=None):
    """`t`: the output grid (default arange(t0 - 1, t_end)); div = None solves on the grid itself (no step_size option)."""
    import hode
    import model
    gen = torch.Generator().manual_seed(seed)
    cls = model.NeuralODEReal if kind == "neural" else model.NeuralODEReal2nd
    torch.manual_seed(seed)
    ode = cls(D, ACT, STAT, H, t_end, 1, device=dev)
    y0 = torch.randn(B, D, generator=gen) * 0.5
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen) * 2
    t = torch.arange(t0 - 1, t_end, 1.0) if t is None else t
    step = None if div is None else 1.0 / div
    cot = torch.randn(t.numel(), B, D, generator=gen)
    ode.set_action_static(a.to(dev), None)
    yg = y0.to(dev).requires_grad_(True)
    h = hode.odeint(ode, yg, t.to(dev), method=method, options=dict({"perturb": perturb}, **({} if step is None else {"step_size": step})))
    (h * cot.to(dev)).sum().backward()
    got = [yg.grad] + [p.grad for p in ode.ml_net.parameters()]
    ps = [p.detach().cpu().double().requires_grad_(True) for p in ode.ml_net.parameters()]
    yc = y0.double().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hc, _ = neural_real_eager.solve(kind, yc, *ps, a.double(), t.double(), method, step_size=step, perturb=perturb)
    (hc * cot.double()).sum().backward()
    return h, hc, got, [yc.grad] + [p.grad for p in ps]


@pytest.mark.parametrize("case", _family("neural_real"), ids=kv.case_id)
def test_neural_real(case):
    h, hc, got, want = _neural_real(case["kind"], case["D"], case["method"], case["H"], case["B"], case["perturb"],
                                    case["div"], _dev(), seed=case["D"] + case["H"])
    _traj_ok(h, hc)
    for name, g, w in zip(("y0", "w1", "b1", "w2", "b2"), got, want):
        assert _rel(g, w) < NEURAL_REAL_GRAD_TOL, (name, _rel(g, w))


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
def _real_problem(D, H, method, perturb=True, B=37, Ta=12, t0=4, t=None):
    """Inputs and the fp64 oracle (h, grad_y0, flat weight gradient, theta gradient) of sum(h * cot).  `t`: the grid as a
    tuple (default arange(t0 - 1, Ta), solved with step_size 1); a given grid is the solver grid itself."""
    from oracle.rhs import RocheRealRHS
    from oracle.solvers import odeint as oracle_odeint
    gen = torch.Generator().manual_seed(D + H)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.2).float() * torch.rand(Ta, B, 1, generator=gen)
    opts = {"perturb": perturb} if t is not None else {"perturb": perturb, "step_size": 1.0}
    t = torch.arange(t0 - 1, Ta, 1, dtype=torch.float32) if t is None else torch.tensor(t, dtype=torch.float32)
    y0 = torch.randn(B, D, generator=gen) * 0.3
    cot = torch.randn(t.numel(), B, D, generator=gen)
    f64 = copy.deepcopy(f).double()
    f64.set_action_static(a.double())
    y64 = y0.double().requires_grad_(True)
    ho = oracle_odeint(f64, y64, t.double(), method=method, options=opts)
    (ho * cot.double()).sum().backward()
    ref = dict(h=ho.detach(), gy0=y64.grad, gw=torch.cat([p.grad.reshape(-1) for p in _real_flat(f64)]),
               gth=torch.stack([f64.k_immunity.grad, f64.kel.grad, f64.kel2.grad]))
    wflat = torch.cat([p.detach().reshape(-1) for p in _real_flat(f)])
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return dict(y0=y0, a=a, t=t, cot=cot, wflat=wflat, theta=theta, perturb=perturb), ref


def _real_gpu(p, H, method, dev, lanes=0):
    from hode.real import real_solve
    wflat = p["wflat"].to(dev).requires_grad_(True)
    theta = p["theta"].to(dev).requires_grad_(True)
    y0 = p["y0"].to(dev).requires_grad_(True)
    h = real_solve(y0, theta, wflat, p["t"].to(dev), p["a"][..., 0].to(dev), H, method=method, perturb=p["perturb"],
                   lanes_per_patient=lanes)
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
def test_real(case):
    dev = _dev()
    D, H, method = case["D"], case["H"], case["method"]
    p, ref = _real_problem(D, H, method)
    got = _real_gpu(p, H, method, dev) if case["onchip"] else _real_gpu_tape_backward(p, H, method, dev)
    _traj_ok(got["h"], ref["h"])
    for k in ("gy0", "gw", "gth"):
        assert _rel(got[k], ref[k]) <= 1e-4, (k, _rel(got[k], ref[k]))
    if D == 20 and H > 64:
        # past the matrix-core range the default takes hode_real.hip: the same numbers as forcing that layout
        forced = _real_gpu(p, H, method, dev, lanes=1)
        for k in ("h", "gy0", "gw", "gth"):
            assert torch.equal(got[k], forced[k]), k


# ------------------------------------------------------------------------------------------- Roche fixed grid (all layouts)
# Every Roche kernel runs one of three rhs bodies per launch (kv.roche_body): hill2_k1 (both Hill exponents exactly 2, one
# dose per patient), hill2_kn (exponents 2, a loop over K dose times) and general (powf, and log_f32 in the Hill-exponent
# gradients).  Each case's body is kv.body(case); theta, K and the inputs are part of the fp64 problem's key.
def _theta_names(ablate):
    from oracle.rhs import THETA_NAMES
    return list(THETA_NAMES) + (["theta_1", "theta_2"] if ablate else [])


def _roche_setup(D, ablate, N, T, seed, theta=kv.THETA_DEFAULT, n_dose=1, neg_imm=False, t=None):
    from hode import synth
    from oracle.rhs import RocheRHS
    inp = synth.solver_inputs(N, T, D, seed=seed, n_dose=n_dose)
    if t is not None:  # another output grid than synth.grid(T)
        assert t.numel() == T
        inp["t"] = t
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


def _roche_plan(p, dev, method, ablate, lanes, need_theta, tape, perturb=False):
    from hode import _lib as L
    from hode.plan import RocheRKPlan
    theta = torch.zeros(L.N_THETA)
    theta[: p["theta"].numel()] = p["theta"]
    opt = lambda x: None if x is None else x.to(dev)  # noqa: E731
    plan = RocheRKPlan(p["y0"].to(dev), theta.to(dev), opt(p["w"]), opt(p["b"]), p["t"].to(dev), p["dosage"].to(dev),
                       p["times"].to(dev), method=method, ablate=ablate, lanes_per_patient=lanes,
                       need_theta_grad=need_theta, tape=tape, perturb=perturb)
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


def _grad_ok(k, g, r, tol=GRAD_TOL):
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
def test_roche_fixed_grid(case, record_property):
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


# ------------------------------------------------------------------------------------------ NeuralODE rhs, fixed grid
def _neural_problem(case):
    """Inputs of one fixed-grid NeuralODE case: grid t = k * 3/8 (exact fp32), dose times (B, K) as fp32 values the kernel
    compares exactly -- on the grid ("grid"), two equal ones ("dup": the impulse counts twice) or on the rk4 1/3 stage
    t0 + dt/3 ("third") -- and an fp64 NeuralRHS on the same values."""
    from oracle.rhs import NeuralRHS
    D, B, T, K = case["D"], case["B"], case["T"], case["n_dose"]
    gen = torch.Generator().manual_seed(D * 1000 + B + 7 * T)
    torch.manual_seed(D + B)
    f = NeuralRHS(D, kv.NEURAL_STEP)
    with torch.no_grad():
        f.ml_net[2].weight.mul_(2.0)
    t = torch.arange(T, dtype=torch.float32) * kv.NEURAL_STEP
    y0 = torch.randn(B, D, generator=gen) * 0.5
    dosage = 0.5 + torch.rand(B, generator=gen) * 2
    idx = torch.randint(0, T, (B, K), generator=gen)
    times = t[idx] if K else torch.zeros(B, 0)
    if case["dose"] == "dup":
        times[:, 1] = times[:, 0]
    elif case["dose"] == "third":
        step = torch.arange(B) % (T - 1)
        times[:, 0] = t[step] + 0.125
        # the fp32 stage time of the kernel (add_rn(t0, mul_rn(dt, 1/3f))) and the oracle's fp64 t0 + dt * (1/3) both hit it
        t0, dt = t[step], t[step + 1] - t[step]
        s32 = t0 + dt * torch.tensor(1.0 / 3.0, dtype=torch.float32)
        assert torch.equal(s32, times[:, 0])
        assert torch.equal(t0.double() + dt.double() * (1 / 3), times[:, 0].double())
    cot = torch.randn(T, B, D, generator=gen)
    return dict(f=f, t=t, y0=y0, dosage=dosage, times=times, cot=cot)


def _neural_ref(p, method, perturb):
    from oracle.solvers import odeint as oracle_odeint
    f64 = copy.deepcopy(p["f"]).double()
    f64.dosage, f64.times = p["dosage"].double(), p["times"].double()
    y64 = p["y0"].double().requires_grad_(True)
    h = oracle_odeint(f64, y64, p["t"].double(), method=method, options={"perturb": perturb})
    (h * p["cot"].double()).sum().backward()
    n = f64.ml_net
    g = [q.grad if q.grad is not None else torch.zeros_like(q) for q in (n[0].weight, n[0].bias, n[2].weight, n[2].bias)]
    return dict(h=h.detach(), gy0=y64.grad, gw1=g[0], gb1=g[1], gw2=g[2], gb2=g[3])  # T = 1: no step, zero weight gradients


def _neural_params(p, dev):
    n = p["f"].ml_net
    return [x.detach().clone().to(dev).requires_grad_(True) for x in (n[0].weight, n[0].bias, n[2].weight, n[2].bias)]


def _neural_gpu(p, method, perturb, dev, lanes=0):
    """hode.neural.neural_solve + autograd: the on-chip backward (mf) or the tape backward of the lane layout."""
    from hode.neural import neural_solve
    prm = _neural_params(p, dev)
    y0 = p["y0"].to(dev).requires_grad_(True)
    h = neural_solve(y0, *prm, p["t"].to(dev), p["dosage"].to(dev), p["times"].to(dev), method=method, perturb=perturb,
                     lanes_per_patient=lanes)
    (h * p["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), gy0=y0.grad, gw1=prm[0].grad, gb1=prm[1].grad, gw2=prm[2].grad, gb2=prm[3].grad)


def _neural_gpu_tape_backward(p, method, perturb, dev):
    """The matrix-core backward without grad_w1 (C ABI): neural_mf_bwd_kernel<D, M, false> writes the operand tapes, which
    hode.neural.contract_tape contracts exactly as the lane layout's backward does."""
    import hode
    from hode import _lib as L
    from hode.neural import _desc, contract_tape, neural_solve
    lib = hode.lib()
    w1, b1, w2, b2 = (x.detach() for x in _neural_params(p, dev))
    y0, t, dos, tms = p["y0"].to(dev), p["t"].to(dev), p["dosage"].to(dev), p["times"].to(dev).contiguous()
    h = neural_solve(y0, w1, b1, w2, b2, t, dos, tms, method=method, perturb=perturb).detach()
    gh = p["cot"].to(dev).contiguous()
    gy0 = torch.empty_like(y0)
    d = _desc(y0, t, dos, tms, w1, b1, w2, b2, h, L.METHODS[method], perturb)
    d.grad_h, d.grad_y0 = gh.data_ptr(), gy0.data_ptr()
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    ws = torch.empty(max(n, 4), device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    L.check(lib.hode_rk_bwd(d, torch.cuda.current_stream().cuda_stream), "hode_rk_bwd[neural, tape]")
    T, B, D = h.shape
    gw1, gb1, gw2, gb2 = contract_tape(ws, d, T, B, D, L.METHODS[method])
    torch.cuda.synchronize()
    return dict(h=h, gy0=gy0, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2)


NEURAL_GRADS = ("gy0", "gw1", "gb1", "gw2", "gb2")


@pytest.mark.parametrize("case", _family("neural"), ids=kv.case_id)
def test_neural_fixed_grid(case, record_property):
    """neural_mf_* (on-chip and tape-writing backward) and the lane layout against oracle.rhs.NeuralRHS in fp64 with
    oracle.solvers.odeint, perturb included: trajectory 2e-5 (1 + max|h|), every gradient rel-L2 1e-4.  The tape backward is
    also compared with the on-chip backward on the same inputs (_tape_same_as_onchip)."""
    dev = _dev()
    method, perturb = case["method"], case["perturb"]
    p = _neural_problem(case)
    ref = _neural_ref(p, method, perturb)
    if case["dose"] == "third":  # the 1/3-stage impulse is part of the problem: one ulp later it does not fire
        q = dict(p, times=p["times"].clone())
        q["times"][:, 0] = torch.nextafter(q["times"][:, 0], torch.tensor(1e9))
        assert (_neural_ref(q, method, perturb)["h"] - ref["h"]).abs().max() > 1e-3
    got = _neural_gpu_tape_backward(p, method, perturb, dev) if not case["onchip"] and case["layout"] == "mf" \
        else _neural_gpu(p, method, perturb, dev, kv.neural_lanes(case))
    assert torch.equal(got["h"][0].cpu(), p["y0"])
    _traj_ok(got["h"], ref["h"])
    record_property("err_h", (got["h"].double().cpu() - ref["h"]).abs().max().item() / (1 + ref["h"].abs().max().item()))
    for k in NEURAL_GRADS:
        err = _rel(got[k], ref[k]) if float(ref[k].abs().max()) > 0 else float(got[k].abs().max())
        record_property("err_" + k, err)
        assert err <= 1e-4, (k, err)
    if not case["onchip"] and case["layout"] == "mf":
        _tape_same_as_onchip(got, _neural_gpu(p, method, perturb, dev), method, record_property)


def _tape_same_as_onchip(tape, onchip, method, record_property):
    """neural_mf_bwd_kernel<D, M, false> against <D, M, true> on the same inputs; h comes from the same forward.  grad_y0
    is bit-identical for euler and midpoint.  For rk4 the on-chip variant keeps one stage's activations and recomputes the
    others, and the compiler contracts the four-stage adjoint into different fmas than in the tape variant: grad_y0 moves by
    an ulp or two (rel-L2 <= 7.5e-8 measured over the table).  The weight gradients are the same sums in a different order
    -- BLAS GEMMs over (instance, patient) against per-wave MFMA outer products folded in wave order -- (<= 4.0e-7
    measured).  Both are held to rel-L2 <= 1e-6 (_same_as_with_theta's bound): far below the 1e-4 fp64 tolerance, far above
    the reordering noise."""
    assert torch.equal(tape["h"], onchip["h"])
    e = _rel(tape["gy0"], onchip["gy0"])
    record_property("tape_vs_onchip_gy0", e)
    _same_as_with_theta(tape["gy0"], onchip["gy0"], method != "rk4", "gy0")
    for k in NEURAL_GRADS[1:]:
        e = _rel(tape[k], onchip[k]) if float(onchip[k].abs().max()) > 0 else float(tape[k].abs().max())
        record_property("tape_vs_onchip_" + k, e)
        assert e <= 1e-6, (k, e)


# ------------------------------------------------------------------------------------------------- NeuralODE dopri5
@pytest.mark.parametrize("case", _family("neural_dopri5"), ids=kv.case_id)
def test_neural_dopri5(case, record_property):
    """ndp_fwd_kernel (all three phases), ndp_bwd_kernel and, with the first step size attached, ndp_initbwd_kernel against
    the oracle's dopri5 step algebra replayed in fp64 along the run's own tape (oracle.solvers.odeint_dopri5_replay):
    trajectory 5e-6 (1 + max|h|), every gradient rel-L2 1e-4 (test_hip_neural's replay check)."""
    from hode import adaptive
    from oracle.solvers import odeint_dopri5_replay
    from test_hip_neural import _neural_case, _neural_hip_dopri5
    dev = _dev()
    D, B, T = case["D"], case["B"], case["T"]
    rtol, atol = 1e-6, 1e-8
    inp, f = _neural_case(B, max(T, 2), D, seed=D + B)
    if T == 1:  # one output time: no step, the attached backward is not launched
        inp = {"z0": inp["z0"], "actions": inp["actions"][:1] * 0, "t": inp["t"][:1]}
        f.set_action(inp["actions"])
    cot = torch.randn(T, B, D, generator=torch.Generator().manual_seed(D))
    adaptive.keep_workspace = True
    try:
        got = _neural_hip_dopri5(inp, f, dev, cot, rtol, atol, detach=case["detach"])
        tape = adaptive.read_tape()
    finally:
        adaptive.keep_workspace = False
    assert (got["stats"]["n_accepted"] > 0) == (T > 1)
    first = (not case["detach"]) and T > 1 and bool(tape["init"]["first_accepted"])
    f64 = copy.deepcopy(f).double()
    f64.dosage, f64.times = f.dosage.double(), f.times.double()
    y64 = inp["z0"].double().requires_grad_(True)
    pairs = list(zip(tape["t"], tape["dt"])) if T > 1 else []
    hr = odeint_dopri5_replay(f64, y64, inp["t"].double(), rtol, atol, pairs, first)
    (hr * cot.double()).sum().backward()
    err = (got["h"].double() - hr.detach()).abs().max().item()
    record_property("err_h", err / (1 + hr.abs().max().item()))
    assert err <= NEURAL_DOPRI5_TRAJ_TOL * (1 + hr.abs().max().item()), err
    n = f64.ml_net
    for k, a, b in zip(NEURAL_GRADS, got["g"], [y64.grad, n[0].weight.grad, n[0].bias.grad, n[2].weight.grad, n[2].bias.grad]):
        if T == 1:
            assert (torch.equal(a, cot[0]) if k == "gy0" else float(a.abs().max()) == 0.0), k
            continue
        e = _rel(a, b)
        record_property("err_" + k, e)
        assert e <= 1e-4, (k, case["detach"], e)


# ------------------------------------------------------------------------------------------------------- LSTM encoder
def _lstm_problem(case):
    from oracle.encoder import EncoderLSTMOracle
    H, obs, B, T = case["H"], case["obs"], case["B"], case["T"]
    gen = torch.Generator().manual_seed(H * 100 + obs + B)
    torch.manual_seed(H + obs)
    enc = EncoderLSTMOracle(obs + 1, H, 12)
    with torch.no_grad():
        for prm in enc.lstm.parameters():
            prm.mul_(1.5)
    x = torch.randn(T, B, obs, generator=gen)
    a = torch.rand(T, B, 1, generator=gen) * (torch.rand(T, B, 1, generator=gen) < 0.3).float()
    m = (torch.rand(T, B, obs, generator=gen) < 0.5).float()
    cot = torch.randn(B, H, generator=gen)
    return enc, x, a, m, cot


def _lstm_fwd_tape(x, a, m, w, dev, nt):
    """hode_lstm_fwd with save_tape = 1 (the forward lstm_encode runs), for its final c."""
    import hode
    from hode import _lib as L
    from hode.lstm import _desc
    lib = hode.lib()
    B, H = x.shape[1], w[1].shape[1]
    h = torch.empty((B, H), device=dev)
    c = torch.empty((B, H), device=dev)
    d = _desc(x, a, m, *w, True, True)
    d.patient_tiles, d.h_out, d.c_out = nt, h.data_ptr(), c.data_ptr()
    n = lib.hode_lstm_workspace_bytes(d)
    assert n > 0
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    L.check(lib.hode_lstm_fwd(d, torch.cuda.current_stream().cuda_stream), "hode_lstm_fwd")
    torch.cuda.synchronize()
    return h, c


def _lstm_fill_operand_ok(x, a, m, w, dev):
    """hode_lstm_fill_operand writes h_prev[t][b][0:obs] = x * mask and nothing else: exact, the rest stays NaN."""
    import hode
    from hode import _lib as L
    from hode.lstm import _desc
    lib = hode.lib()
    T, B, obs = x.shape
    H = w[1].shape[1]
    W = (obs + 1 + H + 1 + 3) // 4 * 4
    hp = torch.full((T, B, W), float("nan"), device=dev)
    d = _desc(x, a, m, *w, True, True)
    dummy = torch.empty(1, device=dev)
    d.h_out, d.c_out, d.h_prev = dummy.data_ptr(), dummy.data_ptr(), hp.data_ptr()
    L.check(lib.hode_lstm_fill_operand(d, torch.cuda.current_stream().cuda_stream), "hode_lstm_fill_operand")
    torch.cuda.synchronize()
    assert torch.equal(hp[..., :obs], x * m)
    assert torch.isnan(hp[..., obs:]).all()


@pytest.mark.parametrize("case", _family("lstm"), ids=kv.case_id)
def test_lstm(case, record_property):
    """lstm_fwd_kernel / lstm_bwd_kernel / lstm_fill_operand_kernel against oracle.encoder.EncoderLSTMOracle in fp64: final h
    to 2e-5 and c to 5e-5 (absolute, test_hip_lstm's bounds), grad_w_ih / grad_w_hh / grad_b_ih / grad_b_hh of sum(h * cot)
    rel-L2 1e-4.  Tape cases go through hode.lstm.lstm_encode (and the ABI forward for c), the others through
    lstm_final_state; NT from patient_tiles where the case forces it, else from the batch size."""
    from hode.lstm import lstm_encode, lstm_final_state
    dev = _dev()
    nt = case["nt"] or 0
    enc, x, a, m, cot = _lstm_problem(case)
    e64 = copy.deepcopy(enc).double()
    h64, c64 = e64.final_hidden(x.double(), a.double(), m.double())
    (h64 * cot.double()).sum().backward()
    p = enc.lstm
    w = [q.detach().to(dev) for q in (p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0)]
    xd, ad, md = x.to(dev), a.to(dev), m.to(dev)
    if case["tape"]:
        h, c = _lstm_fwd_tape(xd, ad, md, w, dev, nt)
        wg = [q.clone().requires_grad_(True) for q in w]
        he = lstm_encode(xd, ad, md, *wg, reverse=True, patient_tiles=nt)
        assert torch.equal(he.detach(), h)
        (he * cot.to(dev)).sum().backward()
        q64 = e64.lstm
        for name, g, r in zip(("w_ih", "w_hh", "b_ih", "b_hh"), wg,
                              (q64.weight_ih_l0, q64.weight_hh_l0, q64.bias_ih_l0, q64.bias_hh_l0)):
            e = _rel(g.grad, r.grad)
            record_property("err_g" + name, e)
            assert e <= 1e-4, (name, e)
        _lstm_fill_operand_ok(xd, ad, md, w, dev)
    else:
        h, c = lstm_final_state(xd, ad, md, *w, reverse=True, patient_tiles=nt)
    eh = (h.double().cpu() - h64.detach()).abs().max().item()
    ec = (c.double().cpu() - c64.detach()).abs().max().item()
    record_property("err_h", eh)
    record_property("err_c", ec)
    assert eh <= LSTM_H_TOL and ec <= LSTM_C_TOL, (eh, ec)


# ------------------------------------------------------------------------------------------------------------ readouts
def _lik_same(lik, lik0, record_property):
    """The loss from the GRAD = false launch against the GRAD = true launch on the same inputs: bit-identical (the loss
    partials are formed by the same code in both instantiations and folded by the same kernel in the same order)."""
    record_property("lik_grad_vs_nograd", abs(lik0 - lik) / abs(lik))
    assert lik0 == lik, (lik0, lik)


@pytest.mark.parametrize("case", _family("readout"), ids=kv.case_id)
def test_readout(case, record_property):
    """readout_sse_kernel / readout_mf_kernel (GRAD true and false) + readout_fold_kernel against the fp64 torch expression
    (test_hip_readout's bounds: loss rel 2e-5, gradients rel-L2 2e-5)."""
    from hode.readout import masked_sse_readout
    dev = _dev()
    variant = kv.READOUT_VARIANT_VALU if case["valu"] else 0
    D, obs, T, B = case["D"], case["obs"], case["T"], case["B"]
    gen = torch.Generator().manual_seed(D * 1000 + obs + B)
    torch.manual_seed(obs + T)
    h = torch.randn(T, B, D, generator=gen)
    x = torch.randn(T, B, obs, generator=gen)
    m = torch.rand(T, B, obs, generator=gen) * (torch.rand(T, B, obs, generator=gen) < 0.6).float()
    lin = torch.nn.Linear(D, obs)
    hr = h.clone().double().requires_grad_(True)
    w64, b64 = lin.weight.detach().double().requires_grad_(True), lin.bias.detach().double().requires_grad_(True)
    ref = torch.sum((x.double() - (hr @ w64.t() + b64)) ** 2 * m.double()) / B
    ref.backward()
    hg = h.to(dev).requires_grad_(True)
    wg, bg = lin.weight.detach().to(dev).requires_grad_(True), lin.bias.detach().to(dev).requires_grad_(True)
    lik = masked_sse_readout(hg, x.to(dev), m.to(dev), wg, bg, variant=variant)
    lik.backward()
    with torch.no_grad():
        lik0 = masked_sse_readout(hg.detach(), x.to(dev), m.to(dev), wg.detach(), bg.detach(), variant=variant)
    e = abs(lik.item() - ref.item()) / abs(ref.item())
    record_property("err_lik", e)
    assert e <= READOUT_TOL, e
    for k, g, want in (("gh", hg.grad, hr.grad), ("gw", wg.grad, w64.grad), ("gb", bg.grad, b64.grad)):
        e = _rel(g, want)
        record_property("err_" + k, e)
        assert e <= READOUT_TOL, (k, e)
    _lik_same(lik.item(), lik0.item(), record_property)


@pytest.mark.parametrize("case", _family("readout_mlp"), ids=kv.case_id)
def test_readout_mlp(case, record_property):
    """readout_mlp_kernel<DL, 24, GRAD true / false> + readout_mlp_fold_kernel against the fp64 torch expression
    (test_hip_readout's bounds: loss rel 2e-5, gradients rel-L2 3e-5)."""
    from hode.readout import masked_sse_readout_mlp
    dev = _dev()
    D, obs, T, B = case["D"], case["obs"], case["T"], case["B"]
    gen = torch.Generator().manual_seed(D * 1000 + B + T)
    torch.manual_seed(D + 3 * T)
    h = torch.randn(T, B, D, generator=gen)
    x = torch.randn(T, B, obs, generator=gen)
    m = (torch.rand(T, B, obs, generator=gen) < 0.5).float()
    net = torch.nn.Sequential(torch.nn.Linear(D, D + 1), torch.nn.ELU(), torch.nn.Linear(D + 1, obs))
    net64 = copy.deepcopy(net).double()
    hr = h.clone().double().requires_grad_(True)
    ref = torch.sum((x.double() - net64(hr)) ** 2 * m.double()) / B
    ref.backward()
    hg = h.to(dev).requires_grad_(True)
    prm = [q.detach().clone().to(dev).requires_grad_(True) for q in (net[0].weight, net[0].bias, net[2].weight, net[2].bias)]
    lik = masked_sse_readout_mlp(hg, x.to(dev), m.to(dev), *prm)
    lik.backward()
    with torch.no_grad():
        lik0 = masked_sse_readout_mlp(h.to(dev), x.to(dev), m.to(dev), *[q.detach() for q in prm])
    e = abs(lik.item() - ref.item()) / abs(ref.item())
    record_property("err_lik", e)
    assert e <= 2e-5, e
    wants = (hr.grad, net64[0].weight.grad, net64[0].bias.grad, net64[2].weight.grad, net64[2].bias.grad)
    for k, g, want in zip(("gh", "gw1", "gb1", "gw2", "gb2"), [hg.grad] + [q.grad for q in prm], wants):
        e = _rel(g, want)
        record_property("err_" + k, e)
        assert e <= READOUT_MLP_GRAD_TOL, (k, e)
    _lik_same(lik.item(), lik0.item(), record_property)
