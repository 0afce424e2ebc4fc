"""The one-step-ahead solve of the real-data hybrid rhs (libhode_real_step.so: N independent intervals per patient, a start
state each, one launch per direction) against the float64 oracle run per interval, against the chained kernels run per
interval, with sentinels around every buffer, through the presentations autograd hands the binding, and at the model level
(DecoderReal with a 3-D init).  GPU only.  Cases: tests/real_step_cases.py.

Bounds are the family's own for this rhs (tests/test_hip_real_dims.py::_assert_close): trajectory 2e-5 * (1 + max|h|),
gradients rel-L2 1e-4 -- set for a chain of six steps, held here by chains of one to three.  Model level: h under the same
trajectory bound; x_hat, which is h through the two-layer readout, under 1e-4 (1 + max|x_hat|), the relative bound
test_model_loss_matches_cpu_oracle_pipeline there holds the loss to; parameter and init gradients rel-L2 2e-3 as there,
gradients below 1e-10 skipped."""
import copy
import functools

import pytest
import torch

import binding_cases as bc
import real_step_cases as cases

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _flat(f):
    return [f.dx1_net[0].weight, f.dx1_net[0].bias, f.dx1_net[2].weight, f.dx1_net[2].bias,
            f.dx2_net[0].weight, f.dx2_net[0].bias, f.dx2_net[2].weight, f.dx2_net[2].bias,
            f.lin_hh.weight, f.lin_hz.weight, f.lin_hr.weight]


def _inputs(D, H, B, N):
    """fp32 inputs of one problem: the rhs module, doses on 20 % of the (hour, patient) cells -- before the window and
    inside it --, the grid of N + 1 points, a start state per interval and the cotangent of h."""
    from oracle.rhs import RocheRealRHS
    gen = torch.Generator().manual_seed(1000 * D + 10 * H + B + 7 * N)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    a = (torch.rand(cases.TA, B, 1, generator=gen) < 0.2).float() * torch.rand(cases.TA, B, 1, generator=gen)
    a[1, 0, 0], a[cases.T_START, 0, 0] = 0.7, 0.4   # patient 0: one dose before the window, one inside it, whatever the draw
    t = torch.arange(cases.T_START, cases.T_START + N + 1, 1, dtype=torch.float32)
    init = torch.randn(N, B, D, generator=gen) * 0.3
    cot = torch.randn(N + 1, B, D, generator=gen)
    wflat = torch.cat([p.detach().reshape(-1) for p in _flat(f)])
    assert wflat.numel() == cases.wflat_len(D, H)
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return f, dict(init=init, a=a, t=t, cot=cot, wflat=wflat, theta=theta)


@functools.lru_cache(maxsize=None)
def _problem(D, H, B, N, S, method, perturb):
    """The inputs and the float64 oracle of sum(h * cot), one oracle solve per interval over t[i : i + 2] with step_size
    1 / S; computed once per problem and left unchanged."""
    from oracle.solvers import odeint as oracle_odeint
    f, p = _inputs(D, H, B, N)
    f64 = copy.deepcopy(f).double()
    f64.set_action_static(p["a"].double())
    i64 = p["init"].double().requires_grad_(True)
    t64 = p["t"].double()
    ends = [oracle_odeint(f64, i64[i], t64[i:i + 2], method=method, options={"perturb": perturb, "step_size": 1.0 / S})[-1]
            for i in range(N)]
    ho = torch.stack([torch.zeros_like(ends[0])] + ends)
    (ho * p["cot"].double()).sum().backward()
    ref = dict(h=ho.detach(), ginit=i64.grad, gw=torch.cat([q.grad.reshape(-1) for q in _flat(f64)]),
               gth=torch.stack([f64.k_immunity.grad, f64.kel.grad, f64.kel2.grad]))
    return p, ref


def _case_problem(c):
    return _problem(c["D"], c["H"], c["B"], c["N"], c["S"], c["method"], c["perturb"])


def _gpu(p, c, dev, C=None, leaf=None, cot=None):
    """`leaf`: the start states as the tensor the binding is handed (default: the plain fp32 tensor); `cot`: a map of the
    cotangent."""
    from hode.real_step import real_step_solve
    wflat = p["wflat"].to(dev).requires_grad_(True)
    theta = p["theta"].to(dev).requires_grad_(True)
    leaf = (p["init"].to(dev) if leaf is None else leaf).requires_grad_(True)
    h = real_step_solve(leaf, theta, wflat, p["t"].to(dev), p["a"][..., 0].to(dev), c["H"],
                        method=c["method"], perturb=c["perturb"], step_size=1.0 / c["S"], intervals_per_wave=c["C"] if C is None else C)
    (h * (p["cot"].to(dev) if cot is None else cot(p["cot"].to(dev)))).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), ginit=leaf.grad, gw=wflat.grad, gth=theta.grad)


def _assert_close(got, ref, what, keys=("ginit", "gw", "gth")):
    err = (got["h"].double().cpu() - ref["h"].double().cpu()).abs().max().item()
    bound = 2e-5 * (1 + ref["h"].abs().max().item())
    rels = {k: _rel(got[k], ref[k]) for k in keys}
    print("%s: max|h - ref| = %.3e (bound %.3e); rel-L2 %s" % (what, err, bound, ", ".join("%s %.3e" % kv for kv in rels.items())))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert err <= bound, (what, err, bound)
    for k, v in rels.items():
        assert v <= 1e-4, (what, k, v)


# ---------------------------------------------------------------------------------------- 1. per case, against the oracle
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_forward_backward_vs_float64_oracle(case):
    dev = _dev()
    p, ref = _case_problem(case)
    got = _gpu(p, case, dev)
    assert got["h"].shape == (case["N"] + 1, case["B"], case["D"]) and got["ginit"].shape == p["init"].shape
    assert bool((got["h"][0] == 0).all())
    _assert_close(got, ref, cases.case_id(case))


# --------------------------------------------------------------------------- 2. S = 1 against the chained kernels, per interval
@pytest.mark.parametrize("case", cases.COMPARE_CASES, ids=cases.case_id)
def test_one_step_matches_the_chained_kernels_interval_by_interval(case):
    """h[i + 1] and grad_init[i] against real_solve(init[i], t[i : i + 2]) -- libhode_real_dims.so at D <= 19, libhode.so at
    20 -- bit for bit: the same device templates in the same stage order.  The summed weight and scalar gradients are held
    to the float64 bound only (another summation order)."""
    dev = _dev()
    import hode
    from hode import _real_dims_lib as RD
    from hode.real import real_solve
    p, ref = _case_problem(case)
    got = _gpu(p, case, dev)
    _assert_close(got, ref, cases.case_id(case))
    t, act, cot = p["t"].to(dev), p["a"][..., 0].to(dev), p["cot"].to(dev)
    assert RD.real_solver_library(case["D"]) is (hode.lib() if case["D"] == 20 else RD.side_library())
    gw = torch.zeros_like(got["gw"])
    for i in range(case["N"]):
        y0 = p["init"][i].to(dev).requires_grad_(True)
        wflat = p["wflat"].to(dev).requires_grad_(True)
        hc = real_solve(y0, p["theta"].to(dev), wflat, t[i:i + 2], act, case["H"], method=case["method"], perturb=case["perturb"])
        (hc[1] * cot[i + 1]).sum().backward()
        same_h, same_g = torch.equal(hc[1].detach(), got["h"][i + 1]), torch.equal(y0.grad, got["ginit"][i])
        print("interval %d: max|dh| %.3e max|dg| %.3e" % (i, float((hc[1].detach() - got["h"][i + 1]).abs().max()),
                                                           float((y0.grad - got["ginit"][i]).abs().max())))
        assert same_h and same_g, (i, same_h, same_g)
        gw += wflat.grad
    assert _rel(got["gw"], gw) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 3. padding
SENTINEL = -7.75e8


def _guarded(n, dev, pad=64):
    """A buffer of n floats inside a larger one filled with SENTINEL: (whole, inner view)."""
    whole = torch.full((n + 2 * pad,), SENTINEL, device=dev, dtype=torch.float32)
    return whole, whole[pad:pad + n]


@pytest.mark.parametrize("case", cases.PADDING_CASES, ids=cases.case_id)
def test_nothing_is_written_outside_the_buffers(case):
    """h, grad_init, the flat weight gradient and both workspaces placed inside sentinel-filled buffers, through the C ABI
    (the bindings allocate exact-size tensors): every sentinel survives forward and backward, every output entry is
    finite, and the values are those of the bindings' call."""
    dev = _dev()
    from hode import _lib as L, _real_step_lib as RS
    from hode.real import _desc
    from hode.real_step import interval_grids
    D, H, B, N, S, method, perturb = (case[k] for k in ("D", "H", "B", "N", "S", "method", "perturb"))
    p, _ = _case_problem(case)
    want = _gpu(p, case, dev)
    lib = RS.step_library(N, S, case["C"])
    init, theta, wflat = (p[k].to(dev).contiguous() for k in ("init", "theta", "wflat"))
    grids = interval_grids(p["t"], 1.0 / S).to(dev).contiguous()
    act, gh = p["a"][..., 0].contiguous().to(dev), p["cot"].to(dev).contiguous()
    pad = 64
    h_all, h = _guarded((N + 1) * B * D, dev)
    gi_all, gi = _guarded(N * B * D, dev)
    gw_all, gw = _guarded(wflat.numel(), dev)
    gw.zero_()   # the backward accumulates into it
    gth = torch.zeros(L.N_THETA, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    d = _desc(init, grids, act, theta, wflat, h, L.METHODS[method], perturb, H)
    n = lib.hode_workspace_bytes(d, L.WS_RK_FWD)
    assert n % 4 == 0
    wf_all, wf = _guarded(n // 4, dev)
    d.workspace, d.workspace_bytes = wf.data_ptr(), n
    lib.hode_rk_fwd(d, stream)
    d.grad_h, d.grad_y0, d.grad_theta, d.grad_w1 = gh.data_ptr(), gi.data_ptr(), gth.data_ptr(), gw.data_ptr()
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    wb_all, wb = _guarded(n // 4, dev)
    d.workspace, d.workspace_bytes = wb.data_ptr(), n
    lib.hode_rk_bwd(d, stream)
    torch.cuda.synchronize()
    for name, whole in (("h", h_all), ("grad_init", gi_all), ("grad_w", gw_all), ("fwd workspace", wf_all), ("bwd workspace", wb_all)):
        assert bool((whole[:pad] == SENTINEL).all()) and bool((whole[-pad:] == SENTINEL).all()), name
    for name, inner in (("h", h), ("grad_init", gi), ("grad_w", gw)):
        assert bool(torch.isfinite(inner).all()) and float(inner.abs().max()) < 1e6, name
    assert torch.equal(h.view(N + 1, B, D), want["h"]) and torch.equal(gi.view(N, B, D), want["ginit"])
    assert torch.equal(gw, want["gw"]) and torch.equal(gth[:3], want["gth"])


# ------------------------------------------------------------------------------------------- 4. determinism, the run length
def test_two_backwards_are_bit_identical():
    dev = _dev()
    case = cases.CASES[1]   # 37 patients, 7 intervals, S = 2, runs of 2: several waves per fold
    p, _ = _case_problem(case)
    first, second = _gpu(p, case, dev), _gpu(p, case, dev)
    for k in first:
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("case", [cases.CASES[1], cases.CASES[6], cases.CASES[14]], ids=cases.case_id)
def test_a_forced_run_length_changes_no_state(case):
    """h and grad_init do not depend on how the intervals are cut into runs; the folded gradients only in their summation
    order."""
    dev = _dev()
    from hode import _lib as L, _real_step_lib as RS
    p, ref = _case_problem(case)
    default = _gpu(p, case, dev, C=0)
    d = L.new_solve_desc()
    d.rhs_kind, d.batch, d.latent_dim, d.hidden_dim, d.n_action_times = L.RHS_ROCHE_REAL, case["B"], case["D"], case["H"], cases.TA
    assert RS.step_library(case["N"], case["S"], 0).chosen_intervals_per_wave(d) == 1   # small problems: one interval per wave
    for C in (1, 2, 3, case["N"], case["N"] + 5):
        forced = _gpu(p, case, dev, C=C)
        assert torch.equal(forced["h"], default["h"]) and torch.equal(forced["ginit"], default["ginit"]), C
        _assert_close(forced, ref, "C = %d" % C)
    assert torch.equal(_gpu(p, case, dev, C=1)["gw"], default["gw"])


# ----------------------------------------------------------------------------------- 5. what autograd hands the binding
def test_presentations_of_init_and_the_cotangent_match_the_plain_call():
    """Offset, strided and expanded views of init, an fp64 init, rows beyond N, and a non-contiguous / fp64 cotangent
    against the plain call, bit for bit (helpers of tests/binding_cases.py)."""
    dev = _dev()
    case = cases.CASES[1]
    p, _ = _case_problem(case)
    plain = _gpu(p, case, dev)
    N = case["N"]

    views = {"offset4": bc.offset_view(p["init"], dev, 1), "offset8": bc.offset_view(p["init"], dev, 2),
             "strided": bc.strided_view(p["init"], dev), "fp64": p["init"].double().to(dev)}
    assert not views["strided"].is_contiguous() and views["offset4"].data_ptr() % 16 == 4
    for name, view in views.items():
        assert torch.equal(view.float(), p["init"].to(dev)), name
        got = _gpu(p, case, dev, leaf=view)
        for k in plain:
            assert got[k].shape == plain[k].shape and torch.equal(got[k].float(), plain[k]), (name, k)
    # constant along time: a stride-0 expand against the same values as a dense tensor
    q = dict(p, init=p["init"][:1].expand(p["init"].shape).contiguous())
    dense = _gpu(q, case, dev)
    got = _gpu(q, case, dev, leaf=bc.expanded_view(q["init"], dev))
    for k in dense:
        assert torch.equal(got[k], dense[k]), ("expanded", k)
    # cotangents as autograd produces them: a transposed (non-contiguous) one, an fp64 one
    for name, cot in (("transposed", lambda c: c.transpose(0, 1).contiguous().transpose(0, 1)), ("fp64", lambda c: c.double())):
        got = _gpu(p, case, dev, cot=cot)
        for k in plain:
            assert torch.equal(got[k].float(), plain[k]), (name, k)
    # a leaf with more rows than intervals: the rows beyond N get exactly zero
    from hode.real_step import real_step_solve
    leaf = torch.cat([p["init"], torch.full((2,) + tuple(p["init"].shape[1:]), float("nan"))]).to(dev).requires_grad_(True)
    h = real_step_solve(leaf, p["theta"].to(dev), p["wflat"].to(dev), p["t"].to(dev), p["a"][..., 0].to(dev), case["H"],
                        method=case["method"], perturb=case["perturb"], step_size=1.0 / case["S"])
    (h * p["cot"].to(dev)).sum().backward()
    assert leaf.grad.shape == leaf.shape and bool((leaf.grad[N:] == 0).all()) and torch.equal(leaf.grad[:N], plain["ginit"])


# -------------------------------------------------------------------------------------------------------- 6. model level
def _decoders(D, ode_step_div, dev, T=12, B=33):
    import model
    from oracle.solvers import odeint as oracle_odeint
    obs, act, stat, hidden = 24, 1, 11, 43
    torch.manual_seed(3 + D)
    cpu = torch.device("cpu")
    dec_c = model.DecoderReal(obs, D, act, stat, hidden, T, 1, method="midpoint", ode_step_size=1.0 / ode_step_div, ode_type="hybrid", t0=1, device=cpu)
    dec_c._odeint = oracle_odeint
    dec_g = copy.deepcopy(dec_c).to(dev)
    dec_g.device = dec_g.ode.device = dev
    dec_g.t = dec_g.t.to(dev)
    dec_g.options["step_t"] = dec_g.t
    dec_g._odeint = model.hode.odeint
    gen = torch.Generator().manual_seed(4)
    data = dict(a=(torch.rand(T, B, 1, generator=gen) < 0.2).float() * torch.rand(T, B, 1, generator=gen),
                s=torch.rand(T, B, stat, generator=gen), init=torch.randn(T, B, D, generator=gen) * 0.3,
                c1=torch.randn(T - 1, B, obs, generator=gen), c2=torch.randn(T, B, D, generator=gen))
    return dec_c, dec_g, data


@pytest.mark.parametrize("ode_step_div", cases.MODEL_STEP_DIVS)
@pytest.mark.parametrize("D", cases.MODEL_DIMS)
def test_decoder_matches_the_cpu_oracle_loop(D, ode_step_div):
    """DDW-shaped small inputs (obs 24, statics 11, hidden 43, T 12, B 33): DecoderReal with a 3-D init on the GPU (one
    launch per direction) against the same decoder on the CPU with the oracle solver called once per interval."""
    dev = _dev()
    dec_c, dec_g, data = _decoders(D, ode_step_div, dev)
    outs = []
    for dec, where in ((dec_c, torch.device("cpu")), (dec_g, dev)):
        q = {k: v.to(where) for k, v in data.items()}
        init = q["init"].detach().clone().requires_grad_(True)
        x_hat, h = dec(init, q["a"], q["s"])
        ((x_hat * q["c1"]).sum() + (h * q["c2"]).sum()).backward()
        outs.append((x_hat.detach(), h.detach(), init.grad))
    (xc, hc, gc), (xg, hg, gg) = outs
    T = data["init"].shape[0]
    assert hg.shape == (T, 33, D) and xg.shape == (T - 1, 33, 24)
    assert bool((hg[0] == 0).all()) and bool((xg[0] == 0).all()) and bool((gg[T - 1:] == 0).all())
    for name, got, want, tol in (("x_hat", xg, xc, 1e-4), ("h", hg, hc, 2e-5)):
        err = float((got.cpu() - want).abs().max())
        print("%s: max err %.3e (max|.| %.3e)" % (name, err, float(want.abs().max())))
        assert err <= tol * (1 + float(want.abs().max())), (name, err)
    print("grad_init rel-L2 %.3e" % _rel(gg, gc))
    assert _rel(gg, gc) <= 2e-3
    checked = 0
    for (n, pg), (_, pc) in zip(dec_g.named_parameters(), dec_c.named_parameters()):
        if pc.grad is None or float(pc.grad.abs().max()) < 1e-10:
            continue
        print("%s rel-L2 %.3e" % (n, _rel(pg.grad, pc.grad)))
        assert _rel(pg.grad, pc.grad) <= 2e-3, (n, _rel(pg.grad, pc.grad))
        checked += 1
    assert checked > 10


def test_a_teacher_forced_training_step_reaches_every_parameter():
    """EncoderLSTMReal(output_all=True) over the window -> the 3-D decoder -> masked SSE on x[1:], composed here: every
    parameter of the encoder and the decoder receives a finite, non-zero gradient."""
    import model
    dev = _dev()
    obs, act, stat, T, B, D = 24, 1, 11, 12, 33, 20
    input_dim = obs + act + stat + 1
    torch.manual_seed(11)
    enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=True, reverse=False, device=dev)
    dec = model.DecoderReal(obs, D, act, stat, 43, T, 1, method="midpoint", ode_step_size=1.0, ode_type="hybrid", t0=1, device=dev)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(T, B, obs, generator=gen).to(dev)
    a = ((torch.rand(T, B, 1, generator=gen) < 0.2).float() * torch.rand(T, B, 1, generator=gen)).to(dev)
    mask = (torch.rand(T, B, obs, generator=gen) < 0.5).float().to(dev)
    s = torch.rand(T, B, stat, generator=gen).to(dev)
    mu, log_var = enc(x, torch.cat([a, s], dim=-1), mask)
    assert mu.shape == (T, B, D)
    z = mu + torch.exp(0.5 * log_var) * torch.randn(mu.shape, generator=gen).to(dev)   # a filtered state per step
    x_hat, h = dec(z, a, s)
    assert x_hat.shape == (T - 1, B, obs) and h.shape == (T, B, D)
    loss = (((x[1:] - x_hat) ** 2) * mask[1:]).sum() / B
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for n, q in list(enc.named_parameters()) + list(dec.named_parameters()):
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and bool((q.grad != 0).any()), n
