"""The NeuralODE kernels at the odd latent sizes 5 .. 15 (libhode_neural_odd.so) against float64 / the CPU oracle.  GPU only.
Bounds are those of the even sizes (tests/test_hip_neural.py, tests/reference_checks.py): fixed grid 2e-5 (1 + max|h|) and
rel-L2 1e-4; dopri5 against the free-running oracle 1e-5 (1 + max|h|) / 2e-4, along the run's own tape 5e-6 / 1e-4.
The cases are tests/neural_odd_cases.py's tables, which tests/test_neural_odd_host.py checks against the compiled kernels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import neural_odd_cases as cases
from neural_odd_cases import rel
from oracle.rhs import dose_schedule
from oracle.solvers import odeint as oracle_odeint
from reference_checks import GRAD_TOL, NEURAL_DOPRI5_TRAJ_TOL, TRAJ_TOL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _solve_fixed(p, method, perturb, dev, present=None):
    """hode.neural.neural_solve + backward; `present` maps (name, plain tensor) to the tensor actually handed over."""
    from hode.neural import neural_solve
    present = present or (lambda name, x: x)
    prm = [present("w", x.detach()).requires_grad_(True) for x in cases.params(p["f"], dev)]
    y0 = present("y0", p["y0"].to(dev)).requires_grad_(True)
    h = neural_solve(y0, *prm, p["t"].to(dev), p["dosage"].to(dev), p["times"].to(dev), method=method, perturb=perturb)
    h.backward(present("cot", p["cot"].to(dev)))
    torch.cuda.synchronize()
    return dict(h=h.detach(), gy0=y0.grad, gw1=prm[0].grad, gb1=prm[1].grad, gw2=prm[2].grad, gb2=prm[3].grad)


def _check_fixed(got, ref, y0):
    assert torch.equal(got["h"][0].cpu(), y0)
    err = (got["h"].double().cpu() - ref["h"]).abs().max().item()
    print("  h err %.3e (bound %.3e)" % (err, TRAJ_TOL * (1 + ref["h"].abs().max().item())))
    for k in cases.GRADS:
        print("  %s rel-L2 %.3e" % (k, rel(got[k], ref[k])))
    assert err <= TRAJ_TOL * (1 + ref["h"].abs().max().item())
    for k in cases.GRADS:
        assert rel(got[k], ref[k]) <= GRAD_TOL, (k, rel(got[k], ref[k]))
    gb1 = got["gb1"]
    assert float(gb1.abs().max()) > 0 and rel(gb1, ref["gb1"]) <= GRAD_TOL  # by name: at D = 15 it has a path of its own


# ------------------------------------------------------------------------------------------------------ fixed grid
@pytest.mark.parametrize("case", cases.FIXED_CASES, ids=cases.fixed_id)
def test_fixed_grid_vs_float64_oracle(case):
    dev = _dev()
    D, method, perturb, dose = case["D"], case["method"], case["perturb"], case["dose"]
    p = cases.fixed_problem(D, dose)
    ref = cases.fixed_reference(D, method, perturb, dose)
    if dose == "stage":  # the impulse at the midpoint stage is part of the problem: it moves the trajectory
        assert (ref["h"] - cases.fixed_reference(D, method, perturb, "grid")["h"]).abs().max() > 1e-4
    _check_fixed(_solve_fixed(p, method, perturb, dev), ref, p["y0"])


def test_fixed_grid_two_output_times_at_15():
    dev = _dev()
    p = cases.fixed_problem(15, "grid", cases.N, 2)
    for method in ("euler", "rk4"):
        _check_fixed(_solve_fixed(p, method, False, dev), cases.fixed_reference(15, method, False, "grid", cases.N, 2), p["y0"])


# ----------------------------------------------------------------------------------------------------------- dopri5
def _dopri5_case(D, n):
    from test_hip_neural import _neural_case
    return _neural_case(n, cases.T_DOPRI5, D, seed=D + n)


def _cot(D, n, T=cases.T_DOPRI5):
    return torch.randn(T, n, D, generator=torch.Generator().manual_seed(1))


def _free_running(inp, f, cot):
    from test_hip_neural import _neural_ref_grads
    y0 = inp["z0"].clone().requires_grad_(True)
    f.zero_grad()
    st = {}
    ho = oracle_odeint(f, y0, inp["t"], method="dopri5", rtol=cases.RTOL, atol=cases.ATOL, stats=st)
    (ho * cot).sum().backward()
    return ho.detach(), [g.clone() for g in _neural_ref_grads(f, y0)], st


def _check_free_running(hip, inp, f, cot):
    ho, grads, st = _free_running(inp, f, cot)
    print("  accepted %d (oracle %d), rejected %d (oracle %d)" % (hip["stats"]["n_accepted"], st["n_accepted"],
                                                               hip["stats"]["n_rejected"], st["n_rejected"]))
    err = (hip["h"] - ho).abs().max().item()
    rels = [rel(a, b) for a, b in zip(hip["g"], grads)]
    print("  free-running: h err %.3e, gradients rel-L2 %s" % (err, ["%.2e" % r for r in rels]))
    assert abs(hip["stats"]["n_accepted"] - st["n_accepted"]) <= 1
    assert torch.equal(hip["h"][0], ho[0])
    assert err <= 1e-5 * (1 + ho.abs().max().item())
    assert max(rels) <= 2e-4, rels
    assert float(hip["g"][2].abs().max()) > 0 and rels[2] <= 2e-4  # b1


@pytest.mark.parametrize("case", cases.DOPRI5_FULL, ids=cases.dopri5_id)
def test_dopri5_vs_oracle_and_tape_replay(case):
    from hode import adaptive
    from oracle.solvers import odeint_dopri5_replay
    from test_hip_neural import _neural_hip_dopri5, _neural_ref_grads
    dev = _dev()
    D, n = case["D"], case["N"]
    inp, f = _dopri5_case(D, n)
    cot = _cot(D, n)
    adaptive.keep_workspace = True
    try:
        hip = _neural_hip_dopri5(inp, f, dev, cot, cases.RTOL, cases.ATOL)
        tape = adaptive.read_tape()
    finally:
        adaptive.keep_workspace = False
    hip_det = _neural_hip_dopri5(inp, f, dev, cot, cases.RTOL, cases.ATOL, detach=True)
    _check_free_running(hip, inp, f, cot)
    assert len(tape["t"]) == hip["stats"]["n_accepted"] > 0
    pairs = list(zip(tape["t"], tape["dt"]))
    first = bool(tape["init"]["first_accepted"])
    for run, with_first in ((hip_det, False), (hip, first)):
        y0 = inp["z0"].clone().requires_grad_(True)
        f.zero_grad()
        hr = odeint_dopri5_replay(f, y0, inp["t"], cases.RTOL, cases.ATOL, pairs, with_first)
        (hr * cot).sum().backward()
        err = (run["h"] - hr.detach()).abs().max().item()
        rels = [rel(a, b) for a, b in zip(run["g"], _neural_ref_grads(f, y0))]
        print("  replay (first step %s): h err %.3e, gradients rel-L2 %s" % (with_first, err, ["%.2e" % r for r in rels]))
        assert err <= NEURAL_DOPRI5_TRAJ_TOL * (1 + hr.abs().max().item())
        assert max(rels) <= 1e-4, (with_first, rels)


@pytest.mark.parametrize("case", cases.DOPRI5_ONCE, ids=cases.dopri5_id)
def test_dopri5_vs_free_running_oracle(case):
    from test_hip_neural import _neural_hip_dopri5
    dev = _dev()
    inp, f = _dopri5_case(case["D"], case["N"])
    cot = _cot(case["D"], case["N"])
    _check_free_running(_neural_hip_dopri5(inp, f, dev, cot, cases.RTOL, cases.ATOL), inp, f, cot)


def test_dopri5_one_output_time_at_15():
    """No step: 0 accepted, grad_y0 is the cotangent of h[0], the weight gradients are zero (db1's own slots included)."""
    from test_hip_neural import _neural_case, _neural_hip_dopri5
    dev = _dev()
    inp, f = _neural_case(5, 2, 15, seed=9)
    one = {"z0": inp["z0"], "actions": inp["actions"][:1] * 0, "t": inp["t"][:1]}
    f.set_action(one["actions"])
    cot = torch.randn(1, 5, 15, generator=torch.Generator().manual_seed(3))
    hip = _neural_hip_dopri5(one, f, dev, cot, cases.RTOL, cases.ATOL)
    assert hip["stats"]["n_accepted"] == 0 and torch.equal(hip["h"][0], one["z0"]) and torch.equal(hip["g"][0], cot[0])
    assert all(float(g.abs().max()) == 0.0 for g in hip["g"][1:])


# ------------------------------------------------------------------------------------------------ through the mirror
@pytest.mark.parametrize("method,tol_h", [("dopri5", 5e-6), ("rk4", 2e-5)])
def test_decoder_at_15_through_the_mirror(method, tol_h):
    """RocheExpertDecoder(roche=False) at latent 15, what run_simulation --method=neural --encoder_output_dim=15 builds:
    a configuration error before libhode_neural_odd.so existed."""
    import model
    from hode import adaptive, synth
    from oracle import vi as ovi
    dev = _dev()
    obs, D, T, B = 40, 15, 12, 20
    torch.manual_seed(0)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * synth.STEP, synth.STEP, roche=False, method=method, device=dev)
    dec_o = ovi.DecoderOracle(obs, D, (T - 1) * synth.STEP, synth.STEP, roche=False, method=method)
    dec_o.load_state_dict({k: v.cpu() for k, v in dec.state_dict().items()})
    inp = synth.solver_inputs(B, T, D, seed=2)
    z = inp["z0"].to(dev).requires_grad_(True)
    zo = inp["z0"].clone().requires_grad_(True)
    cot = torch.randn(T, B, obs, generator=torch.Generator().manual_seed(4))
    adaptive.last_stats.update(n_accepted=-1)
    x_hat, h = dec(z, inp["actions"].to(dev))
    assert method != "dopri5" or adaptive.last_stats["n_accepted"] > 0
    x_o, h_o = dec_o(zo, inp["actions"])
    err = (h.detach().cpu() - h_o.detach()).abs().max().item()
    print("  %s: h err %.3e" % (method, err))
    assert err <= tol_h
    (x_hat * cot.to(dev)).sum().backward()
    (x_o * cot).sum().backward()
    assert rel(z.grad, zo.grad) <= 2e-4
    seen = set()
    for (n, p), (_, po) in zip(dec.named_parameters(), dec_o.named_parameters()):
        if po.grad is None or float(po.grad.abs().max()) == 0.0:
            continue
        print("  %s rel-L2 %.3e" % (n, rel(p.grad, po.grad)))
        assert rel(p.grad, po.grad) <= 2e-4, n
        seen.add(n)
    assert "ode.ml_net.0.bias" in seen


def test_g15_vi_loss_and_grads_through_the_kernels(golden_dir):
    """The fixture's VariationalInference.loss (reference numbers, oracle solver in the loop) through the kernels, at the
    bounds tests/test_hip_golden.py holds G5's dopri5 cases to."""
    import model
    from test_hip_golden import _HostDraws, _load_sd
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g15_neural_odd.npz"), allow_pickle=False)
    obs, D, T, B, seed = [int(v) for v in g["vi_meta"]]
    step = float(g["vi_step"])
    enc = model.EncoderLSTM(obs + 1, obs * 2, D, normalize=False, device=dev)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * step, step, roche=False, method="dopri5", device=dev)
    _load_sd(enc, g, "vi_enc_")
    _load_sd(dec, g, "vi_dec_")
    vi = model.VariationalInference(enc, dec, elbo=True, prior_log_pdf=None)
    data = {k2: torch.from_numpy(g["vi_" + k]).to(dev) for k, k2 in (("x", "measurements"), ("a", "actions"), ("mask", "masks"))}
    torch.manual_seed(seed)
    with _HostDraws():
        loss = vi.loss(data)
    loss.backward()
    want = float(g["vi_loss"])
    assert abs(loss.item() - want) <= 5e-5 * abs(want), (loss.item(), want)
    np.testing.assert_allclose(vi.z.detach().cpu().numpy(), g["vi_z"], rtol=2e-5, atol=1e-7)
    for k in ("h_hat", "x_hat"):
        ref = g["vi_" + k]
        assert np.abs(getattr(vi, k).detach().cpu().numpy() - ref).max() <= 2e-4 * (1 + np.abs(ref).max()), k
    for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
        for n, p in mod.named_parameters():
            w = g["vi_" + tag + n.replace(".", "__")]
            got = p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros_like(w)
            np.testing.assert_allclose(got, w, rtol=5e-3, atol=2e-3 * (1 + np.abs(w).max()), err_msg=n)


# ------------------------------------------------------------------------------------ the tensors autograd hands over
def _presentations(dev):
    def strided(name, x):
        if name != "y0":
            return x
        big = torch.zeros(x.shape[0], 2 * x.shape[1], device=x.device, dtype=x.dtype)
        big[:, ::2] = x
        return big[:, ::2].detach()

    def expanded(name, x):
        return x[:, :1].expand_as(x) if name == "cot" else x

    def fp64(name, x):
        return x if name == "cot" else x.double()   # y0 and the four weights

    return {"strided_y0": strided, "expanded_cot": expanded, "fp64": fp64}


def _equal(a, b, keys):
    for k in keys:  # a float64 leaf gets its float32 gradient widened by autograd: compare the values
        assert torch.equal(a[k].float(), b[k].float()), k


def test_bindings_with_real_tensors_at_15_fixed_grid():
    """_NeuralFixedGrid at D = 15 with a strided y0, an expanded cotangent, float64 inputs and on a side stream: within the
    bounds, and bit for bit what the plain call gives (the fold runs in a fixed order)."""
    dev = _dev()
    p = cases.fixed_problem(15)
    keys = ("h",) + cases.GRADS
    pres = _presentations(dev)
    for name in ("strided_y0", "fp64"):
        plain = _solve_fixed(p, "rk4", False, dev)
        _check_fixed(plain, cases.fixed_reference(15, "rk4", False), p["y0"])
        got = _solve_fixed(p, "rk4", False, dev, pres[name])
        assert not name == "strided_y0" or got["gy0"].shape == p["y0"].shape
        _equal(got, plain, keys)
    # an expanded cotangent is a different problem: the plain call gets the same values, materialised
    q = dict(p, cot=p["cot"][:, :1].expand_as(p["cot"]).contiguous())
    plain = _solve_fixed(q, "rk4", False, dev)
    _equal(_solve_fixed(q, "rk4", False, dev, pres["expanded_cot"]), plain, keys)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = _solve_fixed(q, "rk4", False, dev)
    side.synchronize()
    _equal(got, plain, keys)


def test_bindings_with_real_tensors_at_15_dopri5():
    """_NeuralDopri5 at D = 15, the same presentations."""
    from hode import adaptive
    dev = _dev()
    D, n = 15, 17
    inp, f = _dopri5_case(D, n)
    dosage, times = dose_schedule(inp["actions"], 0.125)
    cot = _cot(D, n)

    def run(present=lambda name, x: x, cotangent=cot):
        prm = [present("w", x.detach()).requires_grad_(True) for x in cases.params(f, dev)]
        y0 = present("y0", inp["z0"].to(dev)).requires_grad_(True)
        h = adaptive.neural_dopri5(y0, *prm, inp["t"].to(dev), dosage.to(dev), times.to(dev), rtol=cases.RTOL, atol=cases.ATOL)
        h.backward(present("cot", cotangent.to(dev)))
        torch.cuda.synchronize()
        return dict(h=h.detach(), gy0=y0.grad, gw1=prm[0].grad, gb1=prm[1].grad, gw2=prm[2].grad, gb2=prm[3].grad)

    keys = ("h",) + cases.GRADS
    pres = _presentations(dev)
    plain = run()
    ho, grads, _ = _free_running(inp, f, cot)
    assert (plain["h"].cpu() - ho).abs().max().item() <= 1e-5 * (1 + ho.abs().max().item())
    for k, b in zip(cases.GRADS, grads):
        assert rel(plain[k], b) <= 2e-4, k
    _equal(run(pres["strided_y0"]), plain, keys)
    _equal(run(pres["fp64"]), plain, keys)
    cot_e = cot[:, :1].expand_as(cot).contiguous()
    plain_e = run(cotangent=cot_e)
    _equal(run(pres["expanded_cot"], cot_e), plain_e, keys)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = run(cotangent=cot_e)
    side.synchronize()
    _equal(got, plain_e, keys)


# ------------------------------------------------------------------------------------------------------ still refused
def test_16_is_still_refused():
    import hode
    import model
    from hode import synth
    from hode.neural import neural_solve
    dev = _dev()
    obs, T, B = 40, 12, 20
    dec = model.RocheExpertDecoder(obs, 16, 1, (T - 1) * synth.STEP, synth.STEP, roche=False, method="dopri5", device=dev)
    inp = synth.solver_inputs(B, T, 16, seed=2)
    with pytest.raises(hode.HodeConfigError, match="4, 6, 8, 10, 12, 14"):
        dec(inp["z0"].to(dev), inp["actions"].to(dev))
    dec = model.RocheExpertDecoder(obs, 16, 1, (T - 1) * synth.STEP, synth.STEP, roche=False, method="rk4", device=dev)
    with pytest.raises(hode.HodeConfigError, match="4, 6, 8, 10, 12, 14"):
        dec(inp["z0"].to(dev), inp["actions"].to(dev))
    p = cases.fixed_problem(15)   # the lane-per-patient layout does not exist at the odd sizes
    with pytest.raises(hode.HodeConfigError, match="lanes_per_patient 1"):
        neural_solve(p["y0"].to(dev), *cases.params(p["f"], dev), p["t"].to(dev), p["dosage"].to(dev), p["times"].to(dev),
                     method="rk4", lanes_per_patient=1)
