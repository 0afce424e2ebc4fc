"""The real-data hybrid decoder at the latent sizes 5 .. 19 (libhode_real_dims.so: the matrix-core kernels with the GRU
block as a ragged 16-row tile) against the float64 oracle, against libhode.so at size 20, with sentinels around every
output, through its refusals and at the model level.  GPU only.  Cases: tests/real_dims_cases.py.

Bounds are the family's own (tests/test_hip_real.py): trajectory 2e-5 * (1 + max|h|), gradients rel-L2 1e-4 -- the
arithmetic per row is the one D = 20 runs; model level (test_config5_mirror_loss_matches_cpu_oracle_pipeline): loss 1e-4
relative, parameter gradients rel-L2 2e-3, gradients below 1e-10 skipped."""
import copy
import functools

import pytest
import torch

import real_dims_cases as cases

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _flat(f):
    ps = [f.dx1_net[0].weight, f.dx1_net[0].bias, f.dx1_net[2].weight, f.dx1_net[2].bias,
          f.dx2_net[0].weight, f.dx2_net[0].bias, f.dx2_net[2].weight, f.dx2_net[2].bias]
    if f.ml_dim > 0:
        ps += [f.lin_hh.weight, f.lin_hz.weight, f.lin_hr.weight]
    return ps


def _inputs(D, H, B):
    """fp32 inputs of one problem: the rhs module, doses on 20 % of the (hour, patient) cells -- before the window (hours
    1 .. T0 - 1) and inside it -- the grid, y0 and the cotangent of h."""
    from oracle.rhs import RocheRealRHS
    gen = torch.Generator().manual_seed(1000 * D + 10 * H + B)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    a = (torch.rand(cases.TA, B, 1, generator=gen) < 0.2).float() * torch.rand(cases.TA, B, 1, generator=gen)
    a[1, 0, 0], a[cases.T0 + 1, 0, 0] = 0.7, 0.4   # patient 0: one dose before the window, one inside it, whatever the draw
    t = torch.arange(cases.T0 - 1, cases.TA, 1, dtype=torch.float32)
    y0 = torch.randn(B, D, generator=gen) * 0.3
    cot = torch.randn(t.numel(), B, D, generator=gen)
    wflat = torch.cat([p.detach().reshape(-1) for p in _flat(f)])
    assert wflat.numel() == cases.wflat_len(D, H) and t.numel() >= 3
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return f, dict(y0=y0, a=a, t=t, cot=cot, wflat=wflat, theta=theta)


@functools.lru_cache(maxsize=None)
def _problem(D, H, B, method, perturb):
    """The inputs and the float64 oracle (h, grad_y0, flat weight gradient, theta gradient) of sum(h * cot); computed once
    per case and left unchanged."""
    from oracle.solvers import odeint as oracle_odeint
    f, p = _inputs(D, H, B)
    f64 = copy.deepcopy(f).double()
    f64.set_action_static(p["a"].double())
    y64 = p["y0"].double().requires_grad_(True)
    ho = oracle_odeint(f64, y64, p["t"].double(), method=method, options={"perturb": perturb, "step_size": 1.0})
    (ho * p["cot"].double()).sum().backward()
    ref = dict(h=ho.detach(), gy0=y64.grad, gw=torch.cat([q.grad.reshape(-1) for q in _flat(f64)]),
               gth=torch.stack([f64.k_immunity.grad, f64.kel.grad, f64.kel2.grad]))
    return p, ref


def _gpu(p, H, method, perturb, dev, library=None):
    from hode.real import real_solve
    wflat = p["wflat"].to(dev).requires_grad_(True)
    theta = p["theta"].to(dev).requires_grad_(True)
    y0 = p["y0"].to(dev).requires_grad_(True)
    h = real_solve(y0, theta, wflat, p["t"].to(dev), p["a"][..., 0].to(dev), H, method=method, perturb=perturb, library=library)
    (h * p["cot"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(h=h.detach(), gy0=y0.grad, gw=wflat.grad, gth=theta.grad)


def _assert_close(got, ref, what):
    err = (got["h"].double().cpu() - ref["h"].double().cpu()).abs().max().item()
    bound = 2e-5 * (1 + ref["h"].abs().max().item())
    rels = {k: _rel(got[k], ref[k]) for k in ("gy0", "gw", "gth")}
    print("%s: max|h - ref| = %.3e (bound %.3e); rel-L2 %s" % (what, err, bound, ", ".join("%s %.3e" % kv for kv in rels.items())))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert err <= bound, (what, err, bound)
    for k, v in rels.items():
        assert v <= 1e-4, (what, k, v)


# ---------------------------------------------------------------------------------------- 1. per case, against the oracle
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_forward_backward_vs_float64_oracle(case):
    dev = _dev()
    D, H, B, method, perturb = (case[k] for k in ("D", "H", "B", "method", "perturb"))
    p, ref = _problem(D, H, B, method, perturb)
    got = _gpu(p, H, method, perturb, dev)
    assert got["h"].shape == (p["t"].numel(), B, D)
    _assert_close(got, ref, cases.case_id(case))


def test_the_default_library_at_these_sizes_is_the_side_library():
    """What the cases above ran: `library=None` chose libhode_real_dims.so; libhode.so alone still refuses the size."""
    dev = _dev()
    import hode
    from hode import _real_dims_lib as RD
    from hode.real import real_solve
    _, p = _inputs(7, 16, 3)
    args = [p[k].to(dev) for k in ("y0", "theta", "wflat", "t")] + [p["a"][..., 0].to(dev), 16]
    assert RD.real_solver_library(7) is RD.side_library() and RD.real_solver_library(20) is hode.lib()
    with pytest.raises(hode.HodeConfigError, match=r"latent_dim 7 has no compiled kernel \(have 4, 20\)"):
        real_solve(*args, library=hode.lib())
    assert torch.equal(real_solve(*args), real_solve(*args, library=RD.side_library()))


# ------------------------------------------------------------------------------------- 2. size 20 through the new library
@pytest.mark.parametrize("case", cases.COMPARE_CASES, ids=cases.case_id)
def test_size_20_through_the_side_library_matches_libhode(case):
    """The ragged kernels at M = 16 against libhode.so's full-tile kernels on the same inputs: both inside the family's
    bounds of the oracle and of each other.  (Whether they are bit-identical is printed, not asserted.)"""
    dev = _dev()
    import hode
    from hode import _real_dims_lib as RD
    D, H, B, method, perturb = (case[k] for k in ("D", "H", "B", "method", "perturb"))
    p, ref = _problem(D, H, B, method, perturb)
    main = _gpu(p, H, method, perturb, dev, library=hode.lib())
    side = _gpu(p, H, method, perturb, dev, library=RD.side_library())
    print("bit-identical to libhode.so: %s" % {k: bool(torch.equal(main[k], side[k])) for k in main})
    _assert_close(main, ref, "libhode.so")
    _assert_close(side, ref, "libhode_real_dims.so")
    _assert_close(side, main, "libhode_real_dims.so vs libhode.so")


# ------------------------------------------------------------------------------------------------------------ 3. padding
SENTINEL = -7.75e8


def _guarded(n, dev, pad=64):
    """A buffer of n floats inside a larger one filled with SENTINEL: (whole, inner view)."""
    whole = torch.full((n + 2 * pad,), SENTINEL, device=dev, dtype=torch.float32)
    return whole, whole[pad:pad + n]


@pytest.mark.parametrize("case", cases.PADDING_CASES, ids=cases.case_id)
def test_nothing_is_written_outside_the_outputs(case):
    """h, grad_y0 and the flat weight gradient placed inside sentinel-filled buffers, through the C ABI (the bindings
    allocate exact-size tensors): every sentinel survives forward and backward, every entry inside is finite, and the
    values are those of the bindings' call."""
    dev = _dev()
    from hode import _lib as L, _real_dims_lib as RD
    from hode.real import _desc
    D, H, B, method, perturb = (case[k] for k in ("D", "H", "B", "method", "perturb"))
    p, _ = _problem(D, H, B, method, perturb)
    want = _gpu(p, H, method, perturb, dev)
    lib = RD.side_library()
    y0, theta, wflat, t = (p[k].to(dev).contiguous() for k in ("y0", "theta", "wflat", "t"))
    act, gh = p["a"][..., 0].contiguous().to(dev), p["cot"].to(dev).contiguous()
    T, pad = t.numel(), 64
    h_all, h = _guarded(T * B * D, dev)
    gy_all, gy0 = _guarded(B * D, dev)
    gw_all, gw = _guarded(wflat.numel(), dev)
    gw.zero_()   # the backward accumulates into it
    gth = torch.zeros(L.N_THETA, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    d = _desc(y0, t, act, theta, wflat, h, L.METHODS[method], perturb, H)
    n = lib.hode_workspace_bytes(d, L.WS_RK_FWD)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    lib.hode_rk_fwd(d, stream)
    d.grad_h, d.grad_y0, d.grad_theta, d.grad_w1 = gh.data_ptr(), gy0.data_ptr(), gth.data_ptr(), gw.data_ptr()
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    lib.hode_rk_bwd(d, stream)
    torch.cuda.synchronize()
    for name, whole, inner in (("h", h_all, h), ("grad_y0", gy_all, gy0), ("grad_w", gw_all, gw)):
        assert bool((whole[:pad] == SENTINEL).all()) and bool((whole[-pad:] == SENTINEL).all()), name
        assert bool(torch.isfinite(inner).all()) and float(inner.abs().max()) < 1e6, name
    assert torch.equal(h.view(T, B, D), want["h"]) and torch.equal(gy0.view(B, D), want["gy0"])
    assert torch.equal(gw, want["gw"]) and torch.equal(gth[:3], want["gth"])


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_name_the_sizes_and_launch_nothing():
    """Every configuration outside the domain raises HodeConfigError with the sizes in its text; the output buffers are
    untouched afterwards (nothing ran)."""
    dev = _dev()
    import hode
    from hode import _lib as L, _real_dims_lib as RD
    from hode.real import _desc, real_solve
    side = RD.side_library()
    sizes = "latent_dim 5 .. 20 with hidden_dim 1 .. 64"

    def problem(D, H, B=3):
        T = 3
        return dict(y0=torch.zeros(B, D, device=dev), theta=torch.ones(3, device=dev),
                    wflat=torch.zeros(cases.wflat_len(D, H), device=dev), t=torch.arange(1.0, 1.0 + T, device=dev),
                    act=torch.zeros(4, B, device=dev))

    def solve(D, H, **kw):
        q = problem(D, H)
        return real_solve(q["y0"], q["theta"], q["wflat"], q["t"], q["act"], H, **kw)

    # the bindings: before any library call, with the sizes of both libraries
    for D, H, kw in ((7, 65, {}), (19, 80, {}), (7, 16, dict(lanes_per_patient=1)), (12, 43, dict(lanes_per_patient=1))):
        with pytest.raises(hode.HodeConfigError) as e:
            solve(D, H, **kw)
        text = str(e.value)
        assert "latent_dim %d with hidden_dim %d" % (D, H) in text and "4, 20" in text and "5 .. 19" in text and "1 .. 64" in text
        assert "libhode.so" in text and "libhode_real_dims.so" in text
    # the library itself, handed what real_solver_library would never give it
    for D, H, kw, pat in ((4, 9, {}, "latent_dim 4 has no compiled kernel"), (21, 9, {}, "latent_dim 21 has no compiled kernel"),
                          (24, 9, {}, "latent_dim 24 has no compiled kernel"), (7, 65, {}, "hidden_dim 65 has no compiled kernel"),
                          (7, 16, dict(lanes_per_patient=1), "lanes_per_patient 1 "), (7, 16, dict(lanes_per_patient=4), "lanes_per_patient 4 ")):
        with pytest.raises(hode.HodeConfigError) as e:
            solve(D, H, library=side, **kw)
        assert pat in str(e.value) and sizes in str(e.value) and "hode_real_dims_rk_fwd failed (code -3)" in str(e.value)
    # C ABI: another rhs kind, a backward without grad_w1, a short workspace -- the outputs keep their sentinel
    q = problem(9, 17)
    h = torch.full((3, 3, 9), SENTINEL, device=dev)
    gy0 = torch.full((3, 9), SENTINEL, device=dev)
    gth = torch.full((L.N_THETA,), SENTINEL, device=dev)
    gw = torch.full_like(q["wflat"], SENTINEL)
    ws = torch.empty(1 << 20, device=dev, dtype=torch.uint8)

    def desc(**over):
        d = _desc(q["y0"], q["t"], q["act"], q["theta"], q["wflat"], h, L.METHODS["rk4"], True, 17)
        d.grad_h, d.grad_y0, d.grad_theta, d.grad_w1 = h.data_ptr(), gy0.data_ptr(), gth.data_ptr(), gw.data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        for k, v in over.items():
            setattr(d, k, v)
        return d

    for over, pat in ((dict(rhs_kind=L.RHS_ROCHE), r"rhs_kind %d is not served here .*" % L.RHS_ROCHE + sizes),
                      (dict(rhs_kind=L.RHS_NEURAL), r"rhs_kind %d is not served here .*" % L.RHS_NEURAL + sizes),
                      (dict(grad_w1=None), "grad_w1 is NULL .*libhode.so has it at latent_dim 4 and 20"), (dict(workspace_bytes=64), "workspace 64 B < required"),
                      (dict(method=7), "unknown fixed-grid method 7"), (dict(batch=0), "batch=0"), (dict(theta=None), "must be non-NULL")):
        for fn in (side.hode_rk_fwd, side.hode_rk_bwd):
            if fn is side.hode_rk_fwd and "grad_w1" in over:
                continue   # the forward does not read it
            with pytest.raises(hode.HodeConfigError, match=pat):
                fn(desc(**over), None)
    torch.cuda.synchronize()
    for buf in (h, gy0, gth, gw):
        assert bool((buf == SENTINEL).all())


# -------------------------------------------------------------------------------------------------------- 5. model level
@pytest.mark.parametrize("ode_step_div", cases.MODEL_STEP_DIVS)
@pytest.mark.parametrize("D", cases.MODEL_DIMS)
def test_model_loss_matches_cpu_oracle_pipeline(D, ode_step_div):
    """DDW-shaped tensors (obs 24, statics 11, enc 37->44, dec hidden 43, t0 24, T 40, B 33): VariationalInferenceReal.loss
    and its gradients on the GPU against the same modules on the CPU with the oracle solver injected, as
    tests/test_hip_real.py::test_config5_mirror_loss_matches_cpu_oracle_pipeline does at D = 20.  The readout of DecoderReal
    runs through torch at these sizes (hode.readout.mlp_supported says no): that is the intended path."""
    import model
    from hode import readout
    from oracle.solvers import odeint as oracle_odeint
    dev = _dev()
    obs, act, stat, T, t0, B = 24, 1, 11, 40, 24, 33
    input_dim = obs + act + stat + 1
    hidden = int((obs + act + stat) * 1.2)
    assert hidden == 43 and not readout.mlp_supported(D, D + 1, obs)
    torch.manual_seed(3)
    cpu = torch.device("cpu")
    enc_c = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=cpu)
    dec_c = model.DecoderReal(obs, D, act, stat, hidden, T, 1, method="midpoint", ode_step_size=1.0 / ode_step_div, ode_type="hybrid", t0=t0, device=cpu)
    dec_c._odeint = oracle_odeint
    enc_g, dec_g = copy.deepcopy(enc_c).to(dev), copy.deepcopy(dec_c).to(dev)
    enc_g.device = dec_g.device = dec_g.ode.device = dev
    dec_g.t = dec_g.t.to(dev)
    dec_g.options["step_t"] = dec_g.t
    dec_g._odeint = model.hode.odeint
    gen = torch.Generator().manual_seed(4)
    data = {"measurements": torch.randn(T, B, obs, generator=gen),
            "actions": (torch.rand(T, B, 1, generator=gen) < 0.1).float() * torch.rand(T, B, 1, generator=gen),
            "masks": (torch.rand(T, B, obs, generator=gen) < 0.5).float(),
            "statics": torch.rand(T, B, stat, generator=gen)}
    vi_c = model.VariationalInferenceReal(enc_c, dec_c, elbo=False, t0=t0)
    vi_g = model.VariationalInferenceReal(enc_g, dec_g, elbo=False, t0=t0)
    lc = vi_c.loss(data)
    lc.backward()
    lg = vi_g.loss({k: v.to(dev) for k, v in data.items()})
    lg.backward()
    assert vi_g.x_hat.shape == (T - t0, B, obs)
    print("loss gpu %.8e cpu %.8e" % (lg.item(), lc.item()))
    assert abs(lg.item() - lc.item()) <= 1e-4 * abs(lc.item())
    checked = 0
    for (n, pg), (_, pc) in zip(list(enc_g.named_parameters()) + list(dec_g.named_parameters()),
                                list(enc_c.named_parameters()) + list(dec_c.named_parameters())):
        if pc.grad is None or float(pc.grad.abs().max()) < 1e-10:
            continue
        print("%s rel-L2 %.3e" % (n, _rel(pg.grad, pc.grad)))
        assert _rel(pg.grad, pc.grad) <= 2e-3, (n, _rel(pg.grad, pc.grad))
        checked += 1
    assert checked > 10


@pytest.mark.parametrize("D", [4, 5, 8, 12, 16, 19, 20])
def test_decoder_real_trains_one_step(D):
    """run_real.py-style construction of the hybrid decoder at latent sizes across 4 .. 20: one optimiser step on the GPU
    changes the GRU block's (at D = 4: the expert MLP's) weights and leaves everything finite."""
    import model
    dev = _dev()
    obs, act, stat, T, t0, B = 24, 1, 11, 30, 24, 5
    torch.manual_seed(D)
    dec = model.DecoderReal(obs, D, act, stat, 43, T, 1, method="midpoint", ode_step_size=1.0, ode_type="hybrid", t0=t0, device=dev)
    opt = torch.optim.SGD(dec.parameters(), lr=1e-2)
    gen = torch.Generator().manual_seed(D)
    a = ((torch.rand(T, B, 1, generator=gen) < 0.3).float() * torch.rand(T, B, 1, generator=gen)).to(dev)
    s = torch.rand(T, B, stat, generator=gen).to(dev)
    init = (torch.randn(B, D, generator=gen) * 0.3).to(dev)
    watched = dec.ode.lin_hh.weight if D > 4 else dec.ode.dx1_net[0].weight
    before = watched.detach().clone()
    x = dec(init, a, s)
    x = x[0] if isinstance(x, tuple) else x
    x.square().mean().backward()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and all(bool(torch.isfinite(q).all()) for q in dec.parameters())
    assert not torch.equal(before, watched.detach())
