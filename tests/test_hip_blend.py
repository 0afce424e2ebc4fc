"""The blend kernels on the device (libhode_blend.so through hode.blend) against their float64 eager forms
(tests/blend_eager.py) over the case tables of tests/blend_cases.py, the tensors a caller may hand them bit for bit
against the plain call, the multi-column dose of the expert decoder against the float64 oracle rhs, and the four
training_utils functions of the real-data two-model scripts end to end on the reference's recorded run (G13)."""
import os

import numpy as np
import pytest
import torch

import binding_cases as bc
import blend_cases as bcases
import blend_eager as eager
import model
import training_utils
from reference_checks import TRAJ_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP2 = 2.4e-7            # 2 ulp of fp32
HORIZONS = (6, 12, 24, 72)


def _dev(x):
    return x.to(DEV) if torch.is_tensor(x) else x


# ------------------------------------------------------------------------------------------------------ the fit
def _nnls(x_e, x_m, truth, present=_dev):
    from hode.blend import nnls2_weights
    w_e, w_m = nnls2_weights(present(x_e), present(x_m), present(truth))
    torch.cuda.synchronize()
    return w_e.cpu(), w_m.cpu()


@pytest.fixture(scope="module")
def nnls_reference():
    """Inputs and float64 eager weights of every fit case, computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            inputs = bcases.nnls_inputs(c, seed=c.Tn * 100003 + c.B * 131 + c.obs)
            cache[c] = (inputs, eager.nnls2(*inputs))
        return cache[c]
    return get


@pytest.mark.parametrize("case", bcases.NNLS_CASES, ids=bcases.case_id)
def test_nnls2_against_fp64(case, nnls_reference):
    (x_e, x_m, truth), (r_e, r_m) = nnls_reference(case)
    w_e, w_m = _nnls(x_e, x_m, truth)
    assert w_e.shape == w_m.shape == (case.Tn,) and w_e.dtype == torch.float32
    assert torch.isfinite(w_e).all() and torch.isfinite(w_m).all() and (w_e >= 0).all() and (w_m >= 0).all()
    if bcases.rank_deficient(case):
        got, want = eager.objective(w_e, w_m, x_e, x_m, truth), eager.objective(r_e, r_m, x_e, x_m, truth)
        sb2 = (truth.double() ** 2).sum(dim=(1, 2))
        print("%s: max (objective - eager objective) / sum b^2 = %.3e" % (bcases.case_id(case), ((got - want) / sb2.clamp_min(1e-300)).max()))
        assert torch.all(got <= want + 1e-6 * sb2)
    else:
        assert torch.equal(eager.active_set(w_e, w_m), eager.active_set(r_e, r_m))
        rel = max(((w.double() - r).abs() / r.abs().clamp_min(1e-300))[r != 0].max().item() if (r != 0).any() else 0.0
                  for w, r in ((w_e, r_e), (w_m, r_m)))
        print("%s: max relative weight error %.3e (bound %.1e)" % (bcases.case_id(case), rel, ULP2))
        assert rel <= ULP2
        assert torch.all(w_e[r_e == 0] == 0) and torch.all(w_m[r_m == 0] == 0)
    again = _nnls(x_e, x_m, truth)
    assert torch.equal(w_e, again[0]) and torch.equal(w_m, again[1])


def test_all_four_active_sets_occur_on_the_device(nnls_reference):
    c = bcases.NnlsCase(6, 40, 3, "mixed")
    (x_e, x_m, truth), _ = nnls_reference(c)
    assert eager.active_set(*_nnls(x_e, x_m, truth)).tolist() == [3, 1, 2, 0, 3, 2]


@pytest.mark.parametrize("pres", ["offset4", "strided", "fp64"])
@pytest.mark.parametrize("shape", [(5, 13), (7, 37)], ids=["wave", "block"])
def test_nnls2_presentations_are_bit_identical(shape, pres, nnls_reference):
    (x_e, x_m, truth), _ = nnls_reference(bcases.NnlsCase(5, *shape, "both"))
    plain = _nnls(x_e, x_m, truth)
    other = _nnls(x_e, x_m, truth, lambda x: bc.present(None, pres, None, x, DEV))
    assert torch.equal(plain[0], other[0]) and torch.equal(plain[1], other[1])


# ---------------------------------------------------------------------------------------------- the horizon tail
def _hz(i, horizons, present=_dev):
    from hode.blend import horizon_sse
    p = {k: (present(v) if torch.is_tensor(v) else v) for k, v in i.items()}
    sse, cnt = horizon_sse(p["x_e"], p["truth"], p["mask"], horizons, x_m=p["x_m"], weight_e=p["weight_e"], weight_m=p["weight_m"])
    torch.cuda.synchronize()
    return sse.cpu(), cnt.cpu()


@pytest.mark.parametrize("case", bcases.HORIZON_CASES, ids=bcases.case_id)
def test_horizon_sse_against_fp64(case):
    c = case
    i = bcases.horizon_inputs(c, seed=c.Tn * 7919 + c.B * 31 + c.obs)
    sse, cnt = _hz(i, c.horizons)
    args = (i["x_e"], i["truth"], i["mask"], c.horizons)
    kw = dict(x_m=i["x_m"], weight_e=i["weight_e"], weight_m=i["weight_m"])
    sse64, cnt64 = eager.horizon_sse(*args, **kw)
    S = eager.horizon_scale(*args, **kw)
    assert sse.shape == cnt.shape == (len(c.horizons), c.B) and sse.dtype == cnt.dtype == torch.float32
    assert torch.equal(cnt.double(), cnt64)
    err = (sse.double() - sse64).abs()
    print("%s: max |sse - sse64| / S = %.3e (bound %.3e)" % (bcases.case_id(c), (err / S.clamp_min(1e-300)).max(), 8 * 2.0 ** -24))
    assert torch.all(err <= 8 * 2.0 ** -24 * S)
    if c.B > 1:
        assert cnt[:, 1].eq(0).all() and sse[:, 1].eq(0).all()       # the unobserved patient
    again = _hz(i, c.horizons)
    assert torch.equal(sse, again[0]) and torch.equal(cnt, again[1])


@pytest.mark.parametrize("pres", ["offset4", "strided", "fp64"])
@pytest.mark.parametrize("weights", bcases.WEIGHT_FORMS)
def test_horizon_sse_presentations_are_bit_identical(weights, pres):
    c = bcases.HorizonCase(73, 65, 24, HORIZONS, weights)
    i = bcases.horizon_inputs(c, seed=5)
    plain = _hz(i, c.horizons)
    other = _hz(i, c.horizons, lambda x: bc.present(None, pres, None, x, DEV))
    assert torch.equal(plain[0], other[0]) and torch.equal(plain[1], other[1])


def test_weight_forms_agree():
    """A number, a (T',) table, a (T', obs) table and a (T', 1, obs) tensor with the same values: the same bits."""
    c = bcases.HorizonCase(73, 3, 24, HORIZONS, "numbers")
    i = bcases.horizon_inputs(c, seed=9)
    want = _hz(i, c.horizons)
    for form in (lambda v: torch.full((c.Tn,), v), lambda v: torch.full((c.Tn, c.obs), v), lambda v: torch.full((c.Tn, 1, c.obs), v)):
        j = dict(i, weight_e=form(0.1), weight_m=form(1.0))
        got = _hz(j, c.horizons)
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


# --------------------------------------------------------------------------------------------- multi-column dose
def test_multi_column_dose_on_the_device():
    """The expert decoder driven by cat([a, s], -1), as run_real_ensemble.py / run_real_residual.py drive it: the same bits
    as the one summed column, and the float64 oracle rhs with the all-column dose (reference model.py:653-657) to the
    real-data solver's trajectory bound."""
    from oracle.rhs import RocheRealRHS
    from oracle.solvers import odeint as oracle_odeint
    T, t0, B, S, H = 37, 24, 33, 3, 16
    torch.manual_seed(11)
    dec = model.DecoderReal(10, 4, 1, S, H, T, 1.0, t0=t0, method="midpoint", ode_step_size=1.0, ode_type="expert", device=DEV)
    g = torch.Generator().manual_seed(12)
    a = (torch.rand(T, B, 1, generator=g) < 0.15).float() * torch.rand(T, B, 1, generator=g)
    s = (0.1 + 0.4 * torch.rand(1, B, S, generator=g)).repeat(T, 1, 1)
    a_in = torch.cat([a, s], dim=-1)
    z0 = 0.3 * torch.randn(B, 4, generator=g)
    with torch.no_grad():
        h = dec.latent(z0.to(DEV), a_in.to(DEV), s.to(DEV)).cpu()
        # the column sum is formed where the decoder forms it: a host sum may add the four columns in another order
        h_sum = dec.latent(z0.to(DEV), a_in.to(DEV).sum(-1, keepdim=True), s.to(DEV)).cpu()
        h_first = dec.latent(z0.to(DEV), a.to(DEV), s.to(DEV)).cpu()
    assert torch.equal(h, h_sum)
    f = RocheRealRHS(4, H)
    f.load_state_dict({k: v.detach().cpu() for k, v in dec.ode.state_dict().items()})
    f = f.double()
    f.set_action_static(a_in.double())
    with torch.no_grad():
        ho = oracle_odeint(f, z0.double(), dec.t.cpu().double(), method="midpoint", options={"perturb": True, "step_size": 1.0})
    err, bound = (h.double() - ho).abs().max().item(), TRAJ_TOL * (1 + ho.abs().max().item())
    print("max |h - oracle| = %.3e (bound %.3e); column 0 alone is off by %.3e" % (err, bound, (h_first.double() - ho).abs().max()))
    assert err <= bound
    assert (h_first.double() - ho).abs().max().item() > 100 * bound   # the statics are in the dose


# ------------------------------------------------------------------------------------------------ end to end, G13
@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_real_two_model.npz"))


def _sd(g, pre):
    return {k[len(pre):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def _fold(g, pre):
    d = {k: torch.from_numpy(g[pre + k]) for k in ("measurements", "actions", "masks")}
    d["statics"] = torch.from_numpy(g[pre + "statics"])[None].repeat(d["measurements"].shape[0], 1, 1)
    return {k: v.to(DEV) for k, v in d.items()}


def _models(g, ml_prefix):
    """The two models of the scripts' init_and_load (encoder_latent_ratio 1.2, ode_step_div 1) with the recorded weights."""
    T, t0, obs, S = (int(v) for v in g["meta"][:4])
    input_dim, hidden = obs + 1 + S + 1, int((obs + 1 + S) * 1.2)
    out = []
    for D, kind, pre in ((4, "expert", "e_"), (20, "gruode", ml_prefix)):
        enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=DEV)
        if kind == "expert":
            dec = model.DecoderReal(obs, D, 1, S, hidden, T, 1.0, method="midpoint", ode_step_size=1.0, ode_type=kind, t0=t0, device=DEV)
        else:
            dec = model.DecoderRealBenchmark(obs, D, 1, S, hidden, T, 1.0, ode_type=kind, t0=t0, device=DEV)
        enc.load_state_dict(_sd(g, pre + "enc_"))
        dec.load_state_dict(_sd(g, pre + "dec_"))
        out.append(model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0))
    return out


def _rmse_fields(lines):
    return [float(str(l).split(",")[2]) for l in lines]


def test_fit_ensemble_weights_on_the_recorded_run(g13):
    """Per step the recorded active set, and weights within the first-order perturbation bound of the device's forecast
    differences: with G, b the recorded Gram matrix and right-hand side restricted to the active columns and dG, db their
    change when the device's forecasts replace the fixture's (float64), |dw| <= 2 |G^-1| (|db| + |dG| |w|) + 2 ulp.
    Measured on MI355X: max |x_hat - recorded| 1.9e-6 (expert) and 1.8e-7 (gruode); the weights then differ
    from the recorded ones by at most 4.4e-7 relative."""
    T, t0, obs, S, n_val, n_test = (int(v) for v in g13["meta"][:6])
    expert, ml = _models(g13, "ens_m_")
    val = _fold(g13, "val_")
    w_e, w_m = training_utils.fit_ensemble_weights(expert, ml, val, t0)
    assert w_e.shape == w_m.shape == (T - t0, 1, obs) and w_e.is_cuda
    assert torch.equal(w_e, w_e[:, :, :1].expand_as(w_e)) and torch.equal(w_m, w_m[:, :, :1].expand_as(w_m))
    got = torch.stack([w_e[:, 0, 0], w_m[:, 0, 0]], dim=1).cpu().double()
    ref = torch.from_numpy(g13["ens_weights"])
    # the device's component forecasts against the fixture's
    x, a, mask, s = (val[k] for k in ("measurements", "actions", "masks", "statics"))
    a_in = torch.cat([a, s], dim=-1)
    with torch.no_grad():
        xe_dev = expert.decoder(expert.encoder(x, a_in, mask)[0], a_in, s)[0].cpu()
        xm_dev = ml.decoder(ml.encoder(x, a_in, mask)[0], a, s)[0].cpu()
    xe_rec, xm_rec = torch.from_numpy(g13["ens_val_x_hat_e"]), torch.from_numpy(g13["ens_val_x_hat_m"])
    print("max |x_hat_e - recorded| = %.3e, max |x_hat_m - recorded| = %.3e" % ((xe_dev - xe_rec).abs().max(), (xm_dev - xm_rec).abs().max()))
    truth = x[t0:].cpu()
    rec, dev = eager.gram(xe_rec, xm_rec, truth), eager.gram(xe_dev, xm_dev, truth)
    assert torch.equal(eager.active_set(got[:, 0], got[:, 1]), eager.active_set(ref[:, 0], ref[:, 1]))
    worst = 0.0
    for i in range(T - t0):
        G = torch.tensor([[rec[0][i], rec[2][i]], [rec[2][i], rec[1][i]]])
        dG = torch.tensor([[dev[0][i], dev[2][i]], [dev[2][i], dev[1][i]]]) - G
        db = torch.tensor([dev[3][i] - rec[3][i], dev[4][i] - rec[4][i]])
        act = (ref[i] > 0).nonzero().flatten()
        if not len(act):
            continue
        Ginv = torch.linalg.inv(G[act][:, act])
        tol = 2 * torch.linalg.matrix_norm(Ginv, 2) * (db[act].norm() + torch.linalg.matrix_norm(dG[act][:, act], 2) * ref[i][act].norm())
        tol = tol + ULP2 * ref[i][act].abs().max()
        dw = (got[i][act] - ref[i][act]).abs().max()
        worst = max(worst, (dw / ref[i][act].abs().max()).item())
        assert dw <= tol, (i, dw.item(), tol.item())
    print("max relative weight difference to the recorded weights: %.3e" % worst)


@pytest.mark.parametrize("run", ["ens", "res"])
def test_evaluate_real_two_model_on_the_recorded_run(g13, run, capsys):
    T, t0, obs, S, n_val, n_test = (int(v) for v in g13["meta"][:6])
    expert, ml = _models(g13, run + "_m_")
    test = _fold(g13, "test_")
    if run == "ens":
        ref = g13["ens_weights"].astype(np.float32)
        weights = tuple(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(ref[:, c, None, None], (T - t0, 1, obs)))).to(DEV) for c in (0, 1))
    else:
        weights = (0.1, 1)
    capsys.readouterr()
    res = training_utils.evaluate_real_two_model(expert, ml, test, t0, *weights)
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if l.startswith("rmse_x,")]
    want = _rmse_fields(g13[run + "_lines"])
    print(run, "device", lines, "recorded", [str(l) for l in g13[run + "_lines"]])
    print("max |x_hat - recorded| = %.3e" % (res["x_hat"].cpu() - torch.from_numpy(g13[run + "_x_hat"])).abs().max())
    assert len(lines) == 4 and [l.split(",")[1] for l in lines] == ["%.4f" % (t0 + n) for n in HORIZONS]
    for h in range(4):
        assert abs(round(float(res["rmse"][h]), 4) - want[h]) <= 1.0001e-4     # the 4 printed decimals, or 1 in the last place
        assert len(res["mse"][h]) == n_test - 1 and np.isfinite(res["rmse_sd"][h])


def test_evaluate_real_on_the_expert_model(g13, capsys):
    T, t0, obs, S, n_val, n_test = (int(v) for v in g13["meta"][:6])
    expert, _ = _models(g13, "ens_m_")
    test = _fold(g13, "test_")
    res = training_utils.evaluate_real(expert, test, t0)
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if l.startswith("rmse_x,")]
    assert len(lines) == 4 and res["x_hat"].shape == (T - t0, n_test, obs)
    # the scripts' formula in float64 on the function's own forecast; both sides are within 8 * 2^-24 S / sse of exact
    per = eager.script_rmse(res["x_hat"].cpu().double(), test["measurements"].cpu().double(), test["masks"].cpu().double(), t0, HORIZONS)
    for h in range(4):
        np.testing.assert_allclose(res["rmse"][h], per[h][1], rtol=1e-5)
        np.testing.assert_allclose(res["mse"][h].double().numpy(), per[h][0].numpy(), rtol=1e-5)
        assert lines[h].startswith("rmse_x,{:.4f},".format(t0 + HORIZONS[h]))
