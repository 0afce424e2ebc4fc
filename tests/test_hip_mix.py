"""The two-model mixture CRPS on the device (libhode_mix.so: hode_mix_crps through hode.mix.mixture_crps) against the
float64 reference (tests/mix_cases.py) over the case table, the tensors a caller may hand it (offset, strided, fp64, a
side stream) bit for bit against the plain call, its reduction to hode.crps.ensemble_crps, the domain refusals, and
training_utils.evaluate_ensemble / evaluate_ensemble_horizon on the device against the same call with the fp64 stand-in."""
import numpy as np
import pytest
import torch

import binding_cases as bc
import mix_cases as mc
import model
import training_utils
from reference_checks import CRPS_TOL, crps_oracle, within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(x):
    return None if x is None else x.to(DEV)


def _call(i, M, per_component, present=_dev):
    from hode.mix import mixture_crps
    p = {k: present(v) for k, v in i.items()}
    out = mixture_crps(p["h_e"], p["h_m"], p["truth"], M, (p["w_e"], p["b_e"]), (p["w_m"], p["b_m"]), weight_e=p["g_e"],
                       weight_m=p["g_m"], per_component=per_component)
    torch.cuda.synchronize()
    return out.cpu()


def _subset(c):
    """Large batches: the fp64 yardstick on a subset of patients (each row's sums are its own), both ends included."""
    if c.B < 10000:
        return None
    g = torch.Generator().manual_seed(c.B)
    return torch.cat([torch.arange(64), torch.randint(0, c.B, (64,), generator=g), torch.arange(c.B - 64, c.B)])


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_kernel_against_fp64(case):
    c = case
    i = mc.inputs(c, seed=c.obs * 1000 + c.M * 10 + c.De + c.Dm + c.B)
    got = _call(i, c.M, c.per_component)
    assert got.shape == ((c.Tn, c.B, c.obs) if c.per_component else (c.Tn, c.B)) and torch.isfinite(got).all()
    idx = _subset(c)
    h_e, h_m, truth = i["h_e"], i["h_m"], i["truth"]
    if idx is not None:
        pick = lambda h: h.reshape(c.Tn, c.M, c.B, -1)[:, :, idx].reshape(c.Tn, c.M * len(idx), -1)
        h_e, h_m, truth, got = pick(h_e), pick(h_m), truth[:, idx], got[:, idx]
    ref, scale = mc.mix_oracle(h_e, h_m, truth, c.M, i["w_e"], i["b_e"], i["w_m"], i["b_m"], i["g_e"], i["g_m"])
    if not c.per_component:
        ref, scale = ref.sum(-1), scale.sum(-1)
    err = ((got.double() - ref).abs() / scale).max().item()
    print("%s: max |err| / scale = %.3e (bound %.1e)" % (mc.case_id(c), err, CRPS_TOL))
    within(got.reshape(-1), ref.reshape(-1), scale.reshape(-1), CRPS_TOL, mc.case_id(c))


def test_one_member_is_the_absolute_error():
    c = mc.Case(20, 4, 6, 1, 9, 7, True, True, True)
    i = mc.inputs(c, seed=3)
    got = _call(i, 1, True)
    vals, _ = mc.mixture_values(i["h_e"], i["h_m"], 1, i["w_e"], i["b_e"], i["w_m"], i["b_m"], i["g_e"], i["g_m"])
    np.testing.assert_allclose(got.numpy(), (vals[:, 0] - i["truth"].double()).abs().numpy(), rtol=1e-5, atol=1e-5)


def test_number_weights_are_broadcast():
    c = mc.Case(20, 4, 6, 10, 9, 7, True, True, True)
    i = mc.inputs(c, seed=4)
    i["g_e"], i["g_m"] = torch.full((c.Tn, c.obs), 0.25), torch.full((c.Tn, c.obs), 1.5)
    table = _call(i, c.M, True)
    i["g_e"], i["g_m"] = None, None
    from hode.mix import mixture_crps
    p = {k: _dev(v) for k, v in i.items()}
    number = mixture_crps(p["h_e"], p["h_m"], p["truth"], c.M, (p["w_e"], p["b_e"]), (p["w_m"], p["b_m"]), weight_e=0.25,
                          weight_m=1.5, per_component=True).cpu()
    assert torch.equal(table, number)
    lin_e, lin_m = torch.nn.Linear(c.De, c.obs).to(DEV), torch.nn.Linear(c.Dm, c.obs).to(DEV)
    a = mixture_crps(p["h_e"], p["h_m"], p["truth"], c.M, lin_e, lin_m)
    b = mixture_crps(p["h_e"], p["h_m"], p["truth"], c.M, (lin_e.weight, lin_e.bias), (lin_m.weight, lin_m.bias))
    assert torch.equal(a, b)


@pytest.mark.parametrize("pres", ["offset4", "offset8", "strided", "fp64", "side_stream", "twice"])
@pytest.mark.parametrize("shape", mc.SIM_SHAPES, ids=lambda s: "obs%d" % s[0])
def test_presentations_are_bit_identical_to_the_plain_call(shape, pres):
    c = mc.Case(*shape, 10, 5, 7, True, True, False)
    i = mc.inputs(c, seed=11)
    plain = [_call(i, c.M, pc) for pc in (False, True)]
    if pres == "side_stream":
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            other = [_call(i, c.M, pc) for pc in (False, True)]
        torch.cuda.current_stream().wait_stream(s)
    elif pres == "twice":
        other = [_call(i, c.M, pc) for pc in (False, True)]
    else:
        present = lambda x: bc.present(None, pres, None, x, DEV)
        other = [_call(i, c.M, pc, present) for pc in (False, True)]
    for a, b in zip(plain, other):
        assert torch.equal(a, b)
    assert torch.allclose(plain[0], plain[1].sum(-1), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", mc.SIM_SHAPES, ids=lambda s: "obs%d" % s[0])
def test_reduces_to_the_single_model_kernel(shape):
    """weight_m = 0, weight_e = 1: hode.crps.ensemble_crps with the expert's affine readout, to CRPS_TOL of its scale."""
    from hode.crps import ensemble_crps
    c = mc.Case(*shape, 50, 9, 7, True, True, True)
    i = mc.inputs(c, seed=13)
    i["g_e"], i["g_m"] = torch.ones(c.Tn, c.obs), torch.zeros(c.Tn, c.obs)
    got = _call(i, c.M, True)
    single = ensemble_crps(i["h_e"].to(DEV), i["truth"].to(DEV), c.M, weight=i["w_e"].to(DEV), bias=i["b_e"].to(DEV),
                           per_component=True).cpu()
    ref, scale = crps_oracle(i["h_e"].reshape(c.Tn, c.M, c.B, c.De), i["truth"], i["w_e"], i["b_e"])
    within(single.reshape(-1), ref.reshape(-1), scale.reshape(-1), CRPS_TOL, "ensemble_crps")
    within(got.reshape(-1), ref.reshape(-1), scale.reshape(-1), CRPS_TOL, "mixture_crps")
    within(got.reshape(-1), single.double().reshape(-1), scale.reshape(-1), CRPS_TOL, "mixture_crps vs ensemble_crps")


def test_domain_refused_on_device():
    from hode import HodeConfigError
    from hode.mix import mixture_crps
    obs, De, Dm, M = mc.FIRST_REFUSED
    c = mc.Case(obs, De, Dm, M, 2, 3, False, False, False)
    p = {k: _dev(v) for k, v in mc.inputs(c, seed=1).items()}
    with pytest.raises(HodeConfigError, match="LDS"):
        mixture_crps(p["h_e"], p["h_m"], p["truth"], M, (p["w_e"], None), (p["w_m"], None))
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(HodeConfigError):
        mixture_crps(z(2, 6, 4), z(2, 6, 6), z(2, 3, 129), 2, (z(129, 4), None), (z(129, 6), None))
    with pytest.raises(HodeConfigError):
        mixture_crps(z(2, 6, 129), z(2, 6, 6), z(2, 3, 20), 2, (z(20, 129), None), (z(20, 6), None))
    with pytest.raises(ValueError):
        mixture_crps(z(2, 7, 4), z(2, 7, 6), z(2, 3, 20), 2, (z(20, 4), None), (z(20, 6), None))
    with pytest.raises(ValueError):
        mixture_crps(z(2, 6, 4), z(2, 6, 6), z(2, 3, 20), 2, (z(20, 4), None), (z(20, 6), None), weight_e=z(3, 20))
    with pytest.raises(HodeConfigError):
        mixture_crps(z(2, 6, 4), z(2, 6, 6), z(2, 3, 20), 2, (z(20, 4), None), (torch.zeros(20, 6), None))


# ------------------------------------------------------------------------------------------------ end to end
OBS, ACT, STEP, T, T0 = 20, 1, 0.125, 15, 5


def _models(seed):
    torch.manual_seed(seed)
    out = []
    for D, roche in ((4, True), (6, False)):
        enc = model.EncoderLSTM(OBS + ACT, 2 * OBS, D, device=DEV, normalize=roche)
        dec = model.RocheExpertDecoder(OBS, D, ACT, (T - 1) * STEP, STEP, roche=roche, method="rk4", device=DEV)
        out.append(model.VariationalInference(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density if roche else None))
    return out


@pytest.mark.parametrize("tensor_weights", [False, True])
def test_evaluate_ensemble_on_device_against_the_fp64_stand_in(tensor_weights, capsys, monkeypatch):
    from hode.batches import DeviceFolds
    expert, ml = _models(7)
    folds = DeviceFolds.synthetic(60, T, OBS, 6, 10, 20, DEV, seed=4, step=STEP)
    if tensor_weights:
        g = torch.Generator().manual_seed(2)
        w_e, w_m = torch.zeros(T, 1, OBS), torch.zeros(T, 1, OBS)
        w_e[T0:], w_m[T0:] = torch.rand(T - T0, 1, OBS, generator=g), torch.rand(T - T0, 1, OBS, generator=g)
        w = dict(weight_expert=w_e.to(DEV), weight_ml=w_m.to(DEV))
    else:
        w = {}
    results = []
    for hooked in (False, True):
        if hooked:
            monkeypatch.setattr(training_utils, "_mixture_crps", mc.oracle_mixture_crps)
            monkeypatch.setattr(training_utils, "_ensemble_crps", mc.oracle_ensemble_crps)
        torch.manual_seed(21)
        torch.cuda.manual_seed(21)
        tup = training_utils.evaluate_ensemble(expert, ml, folds, 10, T0, mc_itr=8, **w)
        lines = capsys.readouterr().out.splitlines()[-4:]
        assert [l.split(",")[0] for l in lines] == ["rmse_z0", "rmse_x", "cprs_z0", "cprs_x"]
        torch.manual_seed(21)
        torch.cuda.manual_seed(21)
        hz = training_utils.evaluate_ensemble_horizon(expert, ml, folds, 10, T0, mc_itr=8, **w)
        results.append((tup, hz))
    (tup, hz), (tup_ref, hz_ref) = results
    print("device", tup, "stand-in", tup_ref)
    assert all(np.isfinite(v) for v in tup)
    # the same draws and the same decoders on both sides: only the scoring kernel differs
    np.testing.assert_allclose([tup[0], tup[3]], [tup_ref[0], tup_ref[3]], rtol=1e-6)
    # every element is within CRPS_TOL of its scale (test_kernel_against_fp64); that scale -- the members' distance to the
    # truth plus the readout magnitudes -- is a few times the CRPS itself: 5 x CRPS_TOL relative to the mean CRPS
    np.testing.assert_allclose([tup[2], tup[5]], [tup_ref[2], tup_ref[5]], rtol=5 * CRPS_TOL)
    np.testing.assert_allclose(hz["rmse_x"], hz_ref["rmse_x"], rtol=1e-6)
    np.testing.assert_allclose(hz["cprs_x"], hz_ref["cprs_x"], rtol=5 * CRPS_TOL)
    np.testing.assert_allclose(hz["cprs_x_sd"], hz_ref["cprs_x_sd"], rtol=1e-3)  # a spread of values that each moved 1e-4
    assert hz["cprs_x"].shape == (T - T0,) and np.all(hz["cprs_x"] > 0)
