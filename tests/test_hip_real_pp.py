"""dopri5 with per-patient step control for the real-data hybrid rhs (libhode_real_pp.so, hode.real_pp,
model._RocheRealPatientDopri5, RocheODEReal.step_control = "patient").  GPU only.  Cases, inputs and the eager runs:
tests/real_pp_cases.py, tests/real_pp_eager.py.

Bounds.  Against the float64 replay of the device's own per-patient tapes: trajectory reference_checks.TRAJ_TOL (1 + max|h|),
gradients rel-L2 reference_checks.GRAD_TOL -- the bounds of the fixed-grid kernels of this rhs; the float32 eager replay
stays 30 times inside them on these cases (tests/test_real_pp_host.py measures it: h 1.9e-7, gy0 6.0e-7, gw 3.1e-6, gth
1.9e-6), so nothing is widened.  Controller against the float64 eager controller at batch one: per patient, the accepted
count within the float32 eager controller's own distance from the float64 one on that case, plus one step (the rejected
counts are printed: one flipped decision changes every step size after it, and float32 eager itself is up to 10 away).
Against a much finer fixed-grid rk4 solve: ACCURACY_FACTOR * rtol (1 + max|h|) -- a solve of n accepted steps, each with a
local error below rtol |y| + atol, is within n times that of the exact one up to the amplification of the flow, and n <= 60
here; the fine solve's own fp32 rounding (448 steps) is allowed for by a floor of 1e-4."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import real_pp_cases as cases
import real_pp_eager as eager
import reference_checks as rc

pytestmark = pytest.mark.gpu
SENTINEL = -7.75e8
ACCURACY_FACTOR, ACCURACY_FLOOR = 100.0, 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _on(c, dev, patients=None):
    _, p = cases.inputs(c)
    sl = slice(None) if patients is None else patients
    return dict(y0=p["y0"][sl].contiguous().to(dev), theta=p["theta"].to(dev), wflat=p["wflat"].to(dev), t=p["t"].to(dev),
                act=p["a"][:, sl, 0].contiguous().to(dev), cot=p["cot"][:, sl].contiguous().to(dev))


def _forward(c, q, **kw):
    from hode import real_pp
    h, ws, stats = real_pp.real_patient_dopri5_forward(q["y0"], q["theta"], q["wflat"], q["t"], q["act"], c["H"], rtol=c["rtol"],
                                                       atol=c["atol"], **kw)
    return h, ws, dict(stats)


def _run(c, q, **kw):
    """Forward, the tapes read back, backward of sum(h * cot)."""
    from hode import real_pp
    h, ws, st = _forward(c, q, **kw)
    B, D = q["y0"].shape
    tapes = real_pp.read_tape(ws, B, D, c["H"], q["act"].shape[0], st["max_steps"], st["n_accepted"])
    gy0, gth, gw = real_pp.real_patient_dopri5_backward(q["y0"], q["theta"], q["wflat"], q["t"], q["act"], c["H"], h, ws,
                                                        st["n_accepted"], st["max_steps"], q["cot"], rtol=c["rtol"], atol=c["atol"])
    torch.cuda.synchronize()
    return dict(h=h, gy0=gy0, gth=gth, gw=gw, tapes=tapes, n_acc=st["n_accepted"].cpu(), n_rej=st["n_rejected"].cpu(),
                status=st["status"].cpu(), ws=ws, stats=st)


@pytest.fixture(scope="module")
def runs():
    """One device run per case, shared by the tests that only read it."""
    done = {}

    def get(c):
        k = cases.case_id(c)
        if k not in done:
            done[k] = _run(c, _on(c, _dev()))
        return done[k]
    return get


# ------------------------------------------------------------------------ 1. per case, against the replay of its own tapes
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_h_and_gradients_vs_the_float64_replay_of_the_devices_own_tapes(c, runs):
    got = runs(c)
    _, p = cases.inputs(c)
    T, B = c["T"], c["B"]
    assert not got["status"].any() and bool((got["n_acc"] >= T - 1).all())
    h = got["h"].cpu()
    assert torch.equal(h[0], p["y0"])
    for b, tape in enumerate(got["tapes"]):
        rows = list(zip(tape["t"], tape["dt"], tape["j"]))
        # the tape's times never cross an output time, and the outputs are reached in order
        assert eager.tape_is_clipped(rows, p["t"]), (b, rows)
        assert torch.equal(torch.from_numpy(tape["y"][0]), p["y0"][b])
        # h[j] is the endpoint of the step that reached t[j]: the start state of the step after it, bit for bit
        for n, j in enumerate(tape["j"][:-1]):
            if j >= 0:
                assert torch.equal(h[j, b], torch.from_numpy(tape["y"][n + 1])), (b, n, j)
        assert tape["j"][-1] == T - 1
    ref = cases.replay(c, [list(zip(tp["t"], tp["dt"], tp["j"])) for tp in got["tapes"]])
    herr = float((h.double() - ref["h"]).abs().max())
    rels = {k: cases.rel_l2(got[k], ref[k]) for k in ("gy0", "gw", "gth")}
    print("%s: steps %d .. %d, rejected %d .. %d; h err %.3e (scale %.2f); rel-L2 %s" % (
        cases.case_id(c), int(got["n_acc"].min()), int(got["n_acc"].max()), int(got["n_rej"].min()), int(got["n_rej"].max()), herr,
        1 + float(ref["h"].abs().max()), ", ".join("%s %.3e" % kv for kv in rels.items())))
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("h", "gy0", "gw", "gth"))
    assert herr <= rc.TRAJ_TOL * (1 + float(ref["h"].abs().max()))
    for k, v in rels.items():
        assert v <= rc.GRAD_TOL, (k, v)


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_the_controller_vs_the_float64_eager_controller_at_batch_one(c, runs):
    got = runs(c)
    r64, r32 = cases.controller(c), cases.controller(c, torch.float32)
    allow_acc = max(abs(a["n_accepted"] - b["n_accepted"]) for a, b in zip(r64, r32)) + 1
    eager_rej = max(abs(a["n_rejected"] - b["n_rejected"]) for a, b in zip(r64, r32))
    d_acc = [abs(int(got["n_acc"][b]) - r64[b]["n_accepted"]) for b in range(c["B"])]
    d_rej = [abs(int(got["n_rej"][b]) - r64[b]["n_rejected"]) for b in range(c["B"])]
    h64 = torch.cat([r["h"] for r in r64], dim=1)
    err = float((got["h"].cpu().double() - h64).abs().max())
    print("%s: |accepted - eager| max %d (allowed %d), |rejected - eager| max %d (float32 eager: %d), h err %.3e" % (
        cases.case_id(c), max(d_acc), allow_acc, max(d_rej), eager_rej, err))
    assert max(d_acc) <= allow_acc
    # two free-running controllers at this tolerance
    assert err <= ACCURACY_FACTOR * c["rtol"] * (1 + float(h64.abs().max()))
    if c["stiff"]:  # the step counts really differ inside the tile of the scaled-up patient
        tile = got["n_acc"][:16]
        assert int(tile.max()) > int(tile.min()) and int(got["n_rej"][cases.STIFF]) > 0


@pytest.mark.parametrize("c", [cases.CASES[2], cases.CASES[10], cases.CASES[-1]], ids=cases.case_id)
def test_accuracy_vs_a_much_finer_fixed_grid_rk4_solve(c, runs):
    from hode import real
    dev = _dev()
    got, q = runs(c), _on(c, dev)
    fine = 64
    t64 = q["t"].double().cpu()
    grid = torch.cat([torch.linspace(float(t64[i]), float(t64[i + 1]), fine + 1, dtype=torch.float64)[:-1] for i in range(c["T"] - 1)]
                     + [t64[-1:]]).float().to(dev)
    ref = real.real_solve(q["y0"], q["theta"], q["wflat"], grid, q["act"], c["H"], method="rk4", perturb=True)[::fine]
    err = float((got["h"] - ref).abs().max())
    bound = max(ACCURACY_FACTOR * c["rtol"], ACCURACY_FLOOR) * (1 + float(ref.abs().max()))
    print("%s: against rk4 on %d steps per interval: %.3e (bound %.3e)" % (cases.case_id(c), fine, err, bound))
    assert err <= bound


# ------------------------------------------------------------------------------------------ 2. isolation, tape-less, repeats
ISOLATION_CASE = cases.CASES[10]  # B = 17, the scaled-up patient in column 3


@pytest.mark.parametrize("col", [0, 15, 16])
def test_a_patient_alone_and_in_a_column_of_a_batch_of_17_bit_for_bit(col, runs):
    c = ISOLATION_CASE
    assert c["B"] == 17
    dev = _dev()
    whole = runs(c)
    for src in sorted({col, cases.STIFF}):
        # patient `src` of the case moved into column `col` of the batch (the other patients keep their places)
        order = list(range(17))
        order[col], order[src] = order[src], order[col]
        moved = _run(c, _on(c, dev, order)) if src != col else whole
        alone = _run(dict(c, B=1), _on(c, dev, [src]))
        assert torch.equal(alone["h"][:, 0], moved["h"][:, col]) and torch.equal(alone["gy0"][0], moved["gy0"][col])
        ta, tb = alone["tapes"][0], moved["tapes"][col]
        assert ta["t"] == tb["t"] and ta["dt"] == tb["dt"] and ta["j"] == tb["j"] and np.array_equal(ta["y"], tb["y"])
        assert int(alone["n_rej"][0]) == int(moved["n_rej"][col])


@pytest.mark.parametrize("c", [cases.CASES[5], cases.CASES[13]], ids=cases.case_id)
def test_the_tapeless_forward_and_repeats_are_bit_identical(c, runs):
    dev = _dev()
    q, first = _on(c, dev), runs(c)
    h, ws, st = _forward(c, q, no_tape=True)
    assert torch.equal(h, first["h"]) and torch.equal(st["n_accepted"].cpu(), first["n_acc"])
    assert torch.equal(st["n_rejected"].cpu(), first["n_rej"])
    assert st["no_tape"] is True and st["workspace_bytes"] < first["stats"]["workspace_bytes"]
    again = _run(c, q)
    for k in ("h", "gy0", "gth", "gw", "n_acc", "n_rej"):
        assert torch.equal(again[k], first[k]), k


# --------------------------------------------------------------------------------------------------------- 3. sentinels
@pytest.mark.parametrize("c", [cases.CASES[1], cases.CASES[12]], ids=cases.case_id)
def test_sentinels_around_every_output_gradient_and_workspace_buffer(c, runs):
    from hode import _lib as L
    from hode import _real_pp_lib as PL
    from hode.solver import _stream
    dev = _dev()
    q, want = _on(c, dev), runs(c)
    B, D, T = c["B"], c["D"], c["T"]
    PAD = 64

    def padded(n, dtype=torch.float32, fill=SENTINEL):
        buf = torch.full((n + 2 * PAD,), fill, device=dev, dtype=dtype)
        return buf, buf[PAD:PAD + n]

    lib = PL.lib()
    d = PL.new_desc()
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times = B, D, c["H"], T, q["act"].shape[0]
    d.max_steps, d.rtol, d.atol = want["stats"]["max_steps"], c["rtol"], c["atol"]
    for k in ("t", "y0", "act", "theta", "wflat"):
        setattr(d, k, q[k].data_ptr())
    nbytes = lib.hode_real_pp_workspace_bytes(d)
    assert nbytes == want["stats"]["workspace_bytes"] and nbytes % 16 == 0
    bufs = {"h": padded(T * B * D), "gy0": padded(B * D), "gw": padded(q["wflat"].numel()), "gth": padded(3),
            "ws": padded(nbytes // 4, torch.int32, -77), "status": padded(1, torch.int32, -77), "nacc": padded(B, torch.int32, -77),
            "nrej": padded(B, torch.int32, -77), "pst": padded(B, torch.int32, -77)}
    for k in ("gw", "gth", "status"):
        bufs[k][1].zero_()
    d.h, d.status = bufs["h"][1].data_ptr(), bufs["status"][1].data_ptr()
    d.n_accepted, d.n_rejected, d.patient_status = (bufs[k][1].data_ptr() for k in ("nacc", "nrej", "pst"))
    d.workspace, d.workspace_bytes = bufs["ws"][1].data_ptr(), nbytes
    assert bufs["ws"][1].data_ptr() % 16 == 0
    PL.check(lib.hode_real_pp_fwd(d, _stream()), "fwd")
    d.grad_h, d.grad_y0 = q["cot"].data_ptr(), bufs["gy0"][1].data_ptr()
    d.grad_wflat, d.grad_theta = bufs["gw"][1].data_ptr(), bufs["gth"][1].data_ptr()
    PL.check(lib.hode_real_pp_bwd(d, _stream()), "bwd")
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        fill = SENTINEL if buf.dtype == torch.float32 else -77
        assert bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all()), k
    assert torch.equal(bufs["h"][1].view(T, B, D), want["h"]) and torch.equal(bufs["gy0"][1].view(B, D), want["gy0"])
    assert torch.equal(bufs["gw"][1], want["gw"]) and torch.equal(bufs["gth"][1], want["gth"])
    assert torch.equal(bufs["nacc"][1].cpu(), want["n_acc"]) and int(bufs["status"][1]) == 0
    assert L.STATUS_MAX_STEPS == eager.MAX_STEPS and L.STATUS_NONFINITE == eager.NONFINITE and L.STATUS_DT_UNDERFLOW == eager.DT_UNDERFLOW


# ------------------------------------------------------------------------------------------------- 4. failure reporting
def test_a_nan_patient_is_named_while_its_tile_mates_finish(runs):
    """The NaN is a data input (as in tests/failure_cases.py): one patient's start state."""
    import hode
    from hode import real_pp
    c = ISOLATION_CASE
    q, clean = _on(c, _dev()), runs(c)
    bad = 5
    q["y0"][bad, 2] = float("nan")
    with pytest.raises(hode.HodeError, match=r"non-finite values in state `y` \(first failing patient: %d\)" % bad):
        _forward(c, q)
    st = real_pp.last_stats
    status, nacc = st["status"].cpu(), st["n_accepted"].cpu()
    others = [b for b in range(c["B"]) if b != bad]
    assert int(status[bad]) == eager.NONFINITE and int(nacc[bad]) == 0 and not status[others].any()
    assert torch.equal(nacc[others], clean["n_acc"][others]) and torch.equal(st["n_rejected"].cpu()[others], clean["n_rej"][others])


def test_the_attempt_bound_ends_a_patient():
    import hode
    from hode import real_pp
    c = ISOLATION_CASE
    q = _on(c, _dev())
    with pytest.raises(hode.HodeError, match=r"max_num_steps exceeded \(first failing patient: 0\)"):
        _forward(c, q, max_attempts=2)
    st = real_pp.last_stats
    assert bool((st["status"].cpu() == eager.MAX_STEPS).all())
    assert bool(((st["n_accepted"] + st["n_rejected"]).cpu() == 2).all())


# ------------------------------------------------------------------------------- 5. autograd, the model, the evaluation
def _ode_for(c, dev):
    import model
    f, p = cases.inputs(c)
    ode = model.RocheODEReal(c["D"], 1, 3, c["H"], 12, 1, device=dev)
    with torch.no_grad():
        for dst, src in zip(cases.flat(ode), cases.flat(f)):
            dst.copy_(src.to(dev))
        ode.k_immunity.copy_(f.k_immunity)
        ode.kel.copy_(f.kel)
        ode.kel2.copy_(f.kel2)
    ode.set_action_static(p["a"].to(dev), None)
    return ode


def test_the_tensors_autograd_really_hands_the_binding(runs):
    """hode.odeint with options["step_control"] = "patient": the launch functions' gradients through autograd, for a
    contiguous cotangent, an expanded one (stride 0) and one that is a slice of a larger buffer."""
    import hode
    c = cases.CASES[3]
    dev = _dev()
    want, q = runs(c), _on(c, dev)
    ode = _ode_for(c, dev)
    assert ode.step_control == "batch"
    y0 = q["y0"].clone().requires_grad_(True)
    opts = {"step_control": "patient", "step_t": q["t"], "step_size": 0.5, "perturb": True}
    h = hode.odeint(ode, y0, q["t"], rtol=c["rtol"], atol=c["atol"], method="dopri5", options=dict(opts))
    assert torch.equal(h.detach(), want["h"])
    (h * q["cot"]).sum().backward()
    assert torch.equal(y0.grad, want["gy0"]) and torch.equal(ode.kel.grad, want["gth"][1])
    assert torch.equal(torch.cat([w.grad.reshape(-1) for w in cases.flat(ode)]), want["gw"])
    assert ode.dosage.grad is None
    # an expanded cotangent and a slice of a larger one
    big = torch.randn(c["T"] + 1, c["B"], c["D"] + 4, device=dev)
    for make in (lambda hh: hh.sum(), lambda hh: (hh * big[1:, :, 2:2 + c["D"]]).sum()):
        ya, yb = (q["y0"].clone().requires_grad_(True) for _ in range(2))
        make(hode.odeint(ode, ya, q["t"], rtol=c["rtol"], atol=c["atol"], method="dopri5", options=dict(opts))).backward()
        hb = hode.odeint(ode, yb, q["t"], rtol=c["rtol"], atol=c["atol"], method="dopri5", options=dict(opts))
        (g,) = torch.autograd.grad(make(hb), hb)
        hb.backward(g.contiguous().clone())
        assert torch.equal(ya.grad, yb.grad)
    with torch.no_grad():
        hn = hode.odeint(ode, q["y0"], q["t"], rtol=c["rtol"], atol=c["atol"], method="dopri5", options=dict(opts))
    from hode import real_pp
    assert torch.equal(hn, want["h"]) and real_pp.last_stats["no_tape"] is True


def test_the_default_decoder_trains_and_evaluates_with_patient_step_control():
    """A default-constructed DecoderReal(ode_type="hybrid") -- method dopri5, step_t = its grid, rtol 1e-7, atol 1e-8 -- with
    ode.step_control = "patient": VariationalInferenceReal.loss(...).backward() fills every gradient, and evaluate_real runs
    under no_grad without tapes."""
    import hode
    import model
    import training_utils
    from hode import real_pp
    dev = _dev()
    obs, act, stat, T, t0, B, D = 24, 1, 11, 30, 24, 17, 12   # DDW-shaped: encoder 37 -> 44, decoder hidden 43
    input_dim = obs + act + stat + 1
    torch.manual_seed(5)
    enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=dev)
    dec = model.DecoderReal(obs, D, act, stat, 43, T, 1, t0=t0, ode_type="hybrid", device=dev)
    assert dec.method == "dopri5" and dec.options["step_t"] is dec.t and (dec.rtol, dec.atol) == (1e-7, 1e-8)
    gen = torch.Generator().manual_seed(6)
    data = {"measurements": torch.randn(T, B, obs, generator=gen),
            "actions": (torch.rand(T, B, 1, generator=gen) < 0.3).float() * torch.rand(T, B, 1, generator=gen),
            "masks": (torch.rand(T, B, obs, generator=gen) < 0.5).float(), "statics": torch.rand(T, B, stat, generator=gen)}
    data = {k: v.to(dev) for k, v in data.items()}
    vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0)
    with pytest.raises(hode.HodeConfigError, match="RocheODEReal is built for the fixed-grid methods"):
        vi.loss(data)   # the default control: refused as before
    dec.ode.step_control = "patient"
    loss = vi.loss(data)
    loss.backward()
    torch.cuda.synchronize()
    assert real_pp.last_stats["no_tape"] is False and bool(torch.isfinite(loss))
    for name, q in list(enc.named_parameters()) + list(dec.named_parameters()):
        if name.startswith("log_var"):   # elbo=False: the variance head takes no part in the loss
            continue
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    assert float(dec.ode.lin_hh.weight.grad.abs().max()) > 0 and float(dec.ode.kel.grad.abs()) > 0
    out = training_utils.evaluate_real(vi, data, t0, horizons=(1, 3))
    assert real_pp.last_stats["no_tape"] is True and bool(torch.isfinite(out["x_hat"]).all())
    assert out["x_hat"].shape == (T - t0, B, obs)
