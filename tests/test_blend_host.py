"""CPU checks of the real-data two-model scoring (no GPU): the float64 eager forms (tests/blend_eager.py) against
scipy.optimize.nnls over the GPU case table and against the reference's own run (G13,
tests/golden/make_golden_real_two_model.py); training_utils.evaluate_real / fit_ensemble_weights / residual_targets /
evaluate_real_two_model with the eager forms behind their swap points and the recorded component forecasts injected;
libhode_blend.so's C ABI, digest and refusals; the guard that every compiled blend kernel is reached by a case of the GPU
table; and the multi-column dose of model.RocheODEReal's eager rhs."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_checks
import blend_cases as bcases
import blend_eager as eager
import model
import training_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLEND_SRC = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "blend", "hode_blend.hip")
BLEND_BUILD = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "blend", "build")
HORIZONS = (6, 12, 24, 72)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------- eager forms vs scipy
def test_eager_nnls2_is_scipy_nnls_over_the_case_table():
    nnls = pytest.importorskip("scipy.optimize").nnls
    seen = set()
    for c in bcases.NNLS_CASES:
        if c.B * c.obs > 1000 and c.Tn > 5:
            continue  # the same shape is in the table at T' = 5
        x_e, x_m, truth = bcases.nnls_inputs(c, seed=7)
        w_e, w_m = eager.nnls2(x_e, x_m, truth)
        assert torch.isfinite(w_e).all() and torch.isfinite(w_m).all() and (w_e >= 0).all() and (w_m >= 0).all()
        ref = np.array([nnls(np.stack([x_e[i].numpy().flatten(), x_m[i].numpy().flatten()], axis=1).astype(np.float64),
                             truth[i].numpy().flatten().astype(np.float64))[0] for i in range(c.Tn)])
        if bcases.rank_deficient(c) or c.problem == "zero_col":
            # no unique minimiser (or a free second weight): the same objective, no weight-for-weight claim
            got = eager.objective(w_e, w_m, x_e, x_m, truth)
            want = eager.objective(torch.from_numpy(ref[:, 0]), torch.from_numpy(ref[:, 1]), x_e, x_m, truth)
            assert torch.all((got - want).abs() <= 1e-9 * (truth.double() ** 2).sum(dim=(1, 2)) + 1e-300), bcases.case_id(c)
            continue
        seen |= set(eager.active_set(w_e, w_m).tolist())
        assert torch.equal(eager.active_set(w_e, w_m), eager.active_set(ref[:, 0], ref[:, 1])), bcases.case_id(c)
        assert np.array_equal(_f32(w_e), _f32(ref[:, 0])) and np.array_equal(_f32(w_m), _f32(ref[:, 1])), bcases.case_id(c)
    assert seen == {0, 1, 2, 3}


def test_eager_horizon_sse_is_the_scripts_formula():
    c = bcases.HorizonCase(10, 3, 24, HORIZONS, "t1o")
    i = bcases.horizon_inputs(c, seed=3)
    sse, cnt = eager.horizon_sse(i["x_e"], i["truth"], i["mask"], c.horizons, x_m=i["x_m"], weight_e=i["weight_e"],
                                 weight_m=i["weight_m"])
    assert sse.shape == cnt.shape == (4, 3) and cnt[:, 1].eq(0).all() and sse[:, 1].eq(0).all()
    x_hat = i["x_e"].double() * i["weight_e"].double() + i["x_m"].double() * i["weight_m"].double()
    t0 = 4
    pad = lambda v: torch.cat([torch.zeros(t0, *v.shape[1:], dtype=v.dtype), v])
    per = eager.script_rmse(x_hat, pad(i["truth"].double()), pad(i["mask"].double()), t0, c.horizons)
    for h, (vec, rmse) in enumerate(per):
        mine = sse[h] / cnt[h]
        np.testing.assert_allclose(mine[~torch.isnan(mine)].numpy(), vec.numpy(), rtol=1e-12)
    assert torch.equal(sse[1], sse[2]) and torch.equal(sse[2], sse[3])  # clipped to T' = 10


# ------------------------------------------------------------------------------------------------------ G13
@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_real_two_model.npz"))


def _fold(g, pre):
    d = {k: torch.from_numpy(g[pre + k]) for k in ("measurements", "actions", "masks")}
    d["statics"] = torch.from_numpy(g[pre + "statics"])[None].repeat(d["measurements"].shape[0], 1, 1)
    return d


def _meta(g):
    T, t0, obs, n_static, n_val, n_test = (int(v) for v in g["meta"][:6])
    return T, t0, obs, n_static, n_val, n_test


def test_eager_forms_against_the_recorded_run(g13):
    T, t0, obs, n_static, n_val, n_test = _meta(g13)
    val, test = _fold(g13, "val_"), _fold(g13, "test_")
    x_e, x_m = torch.from_numpy(g13["ens_val_x_hat_e"]), torch.from_numpy(g13["ens_val_x_hat_m"])
    assert x_e.shape == x_m.shape == (T - t0, n_val, obs)
    a11, a22, a12, _, _ = eager.gram(x_e, x_m, val["measurements"][t0:])
    assert torch.all(a11 * a22 - a12 ** 2 > 1e-6 * a11 * a22)
    w_e, w_m = eager.nnls2(x_e, x_m, val["measurements"][t0:])
    ref = g13["ens_weights"]
    assert len(set(eager.active_set(ref[:, 0], ref[:, 1]).tolist())) >= 3
    assert torch.equal(eager.active_set(w_e, w_m), eager.active_set(ref[:, 0], ref[:, 1]))
    assert np.array_equal(_f32(w_e), _f32(ref[:, 0])) and np.array_equal(_f32(w_m), _f32(ref[:, 1]))
    # the recorded blend and the recorded lines from the recorded component forecasts
    assert not test["masks"][t0:, -1].any() and test["masks"][t0:, :-1].sum(dim=(0, 2)).gt(0).all()
    for run, weights in (("ens", (torch.from_numpy(_f32(ref[:, 0])), torch.from_numpy(_f32(ref[:, 1])))), ("res", (0.1, 1))):
        xe, xm = torch.from_numpy(g13[run + "_test_x_hat_e"]), torch.from_numpy(g13[run + "_test_x_hat_m"])
        x_hat = torch.from_numpy(g13[run + "_x_hat"])
        sse, cnt = eager.horizon_sse(xe, test["measurements"][t0:], test["masks"][t0:], HORIZONS, x_m=xm, weight_e=weights[0],
                                     weight_m=weights[1])
        assert torch.isnan((sse / cnt)[:, -1]).all() and cnt[:, -1].eq(0).all()
        per = eager.script_rmse(x_hat, test["measurements"], test["masks"], t0, HORIZONS)
        for h, line in enumerate(g13[run + "_lines"]):
            _, t1, rmse, _ = str(line).split(",")
            mse = (sse[h] / cnt[h])[:-1]
            assert float(t1) == t0 + HORIZONS[h] and len(per[h][0]) == n_test - 1
            assert "%.4f" % per[h][1] == rmse
            np.testing.assert_allclose(mse.numpy(), per[h][0].double().numpy(), rtol=1e-5)
            assert "%.4f" % float(torch.sqrt(mse.mean())) == rmse


# ----------------------------------------------------------------- training_utils with the recorded forecasts injected
class _Recorded:
    """A stand-in model: the encoder notes what it was shown, the decoder hands back the recorded forecast of the fold."""

    def __init__(self, forecasts, log, name):
        self.forecasts, self.log, self.name = forecasts, log, name

    def encoder(self, x, a, m):
        assert x.shape[:2] == a.shape[:2] == m.shape[:2]
        self.log.append((self.name, "enc", x.shape[0], a.shape[-1]))
        return (torch.zeros(x.shape[1], 1),)

    def decoder(self, z0, a, s):
        self.log.append((self.name, "dec", a.shape[0], a.shape[-1]))
        return self.forecasts[a.shape[1]], None


@pytest.fixture
def eager_hooks(monkeypatch):
    monkeypatch.setattr(training_utils, "_nnls2_weights", lambda *a: tuple(w.float() for w in eager.nnls2(*a)))
    monkeypatch.setattr(training_utils, "_horizon_sse", lambda *a, **k: tuple(v.float() for v in eager.horizon_sse(*a, **k)))


def _reseeded_bootstrap(monkeypatch, seeds):
    """The generator's wrapper: torch is reseeded with the next recorded seed before every bootstrap."""
    orig, used = training_utils.bootstrap_RMSE, []

    def bootstrap_RMSE(err_sq):
        torch.manual_seed(int(seeds[len(used)]))
        used.append(int(seeds[len(used)]))
        return orig(err_sq)
    monkeypatch.setattr(training_utils, "bootstrap_RMSE", bootstrap_RMSE)
    return orig, used


def _check_lines(out, res, g, run, t0, x_hat, test, orig_bootstrap):
    lines = [l for l in out.strip().split("\n") if l.startswith("rmse_x,")]
    want = [str(l) for l in g[run + "_lines"]]
    assert [l.rsplit(",", 1)[0] for l in lines] == [l.rsplit(",", 1)[0] for l in want]      # horizon and rmse, 4 decimals
    per = eager.script_rmse(x_hat, test["measurements"], test["masks"], t0, HORIZONS)
    for h, seed in enumerate(g[run + "_seeds"]):
        torch.manual_seed(int(seed))
        sd = orig_bootstrap(per[h][0])                                                     # the reference's own arithmetic
        assert "%.4f" % sd == want[h].rsplit(",", 1)[1]
        np.testing.assert_allclose(res["rmse_sd"][h], sd, rtol=1e-4)
        assert "%.4f" % res["rmse"][h] == want[h].split(",")[2]
        assert len(res["mse"][h]) == len(per[h][0])


def test_ensemble_flow_reproduces_the_reference_run(g13, eager_hooks, monkeypatch, capsys):
    T, t0, obs, n_static, n_val, n_test = _meta(g13)
    val, test = _fold(g13, "val_"), _fold(g13, "test_")
    log = []
    expert = _Recorded({n_val: torch.from_numpy(g13["ens_val_x_hat_e"]), n_test: torch.from_numpy(g13["ens_test_x_hat_e"])}, log, "e")
    ml = _Recorded({n_val: torch.from_numpy(g13["ens_val_x_hat_m"]), n_test: torch.from_numpy(g13["ens_test_x_hat_m"])}, log, "m")
    w_e, w_m = training_utils.fit_ensemble_weights(expert, ml, val, t0)
    # both encoders see the whole fold and cat([a, s]); the expert decoder is driven by cat([a, s]), the ml decoder by a
    assert log == [("e", "enc", T, 1 + n_static), ("e", "dec", T, 1 + n_static), ("m", "enc", T, 1 + n_static), ("m", "dec", T, 1)]
    assert w_e.shape == w_m.shape == (T - t0, 1, obs) and w_e.dtype == torch.float32
    ref = g13["ens_weights"]
    for w, col in ((w_e, 0), (w_m, 1)):
        assert np.array_equal(w.numpy(), np.broadcast_to(_f32(ref[:, col])[:, None, None], w.shape))
    del log[:]
    orig, used = _reseeded_bootstrap(monkeypatch, g13["ens_seeds"])
    capsys.readouterr()
    res = training_utils.evaluate_real_two_model(expert, ml, test, t0, w_e, w_m)
    assert log == [("e", "enc", t0, 1 + n_static), ("e", "dec", T, 1 + n_static), ("m", "enc", t0, 1 + n_static), ("m", "dec", T, 1)]
    assert used == [int(s) for s in g13["ens_seeds"]]
    assert set(res) == {"x_hat", "rmse", "rmse_sd", "mse"}
    np.testing.assert_allclose(res["x_hat"].numpy(), g13["ens_x_hat"], rtol=1e-6, atol=1e-7)
    _check_lines(capsys.readouterr().out, res, g13, "ens", t0, torch.from_numpy(g13["ens_x_hat"]), test, orig)


def test_residual_flow_reproduces_the_reference_run(g13, eager_hooks, monkeypatch, capsys):
    T, t0, obs, n_static, n_val, n_test = _meta(g13)
    val, test = _fold(g13, "val_"), _fold(g13, "test_")
    log = []
    expert = _Recorded({n_val: torch.from_numpy(g13["ens_val_x_hat_e"]), n_test: torch.from_numpy(g13["res_test_x_hat_e"])}, log, "e")
    ml = _Recorded({n_test: torch.from_numpy(g13["res_test_x_hat_m"])}, log, "m")
    before = val["measurements"].clone()
    target = training_utils.residual_targets(expert, val, t0)
    assert log == [("e", "enc", T, 1 + n_static), ("e", "dec", T, 1 + n_static)]
    assert torch.equal(val["measurements"], before) and target.data_ptr() != val["measurements"].data_ptr()
    assert torch.equal(target[:t0], before[:t0])
    assert torch.equal(target[t0:], before[t0:] - torch.from_numpy(g13["ens_val_x_hat_e"]) * 0.1)
    del log[:]
    orig, used = _reseeded_bootstrap(monkeypatch, g13["res_seeds"])
    capsys.readouterr()
    res = training_utils.evaluate_real_two_model(expert, ml, test, t0, 0.1, 1)
    np.testing.assert_allclose(res["x_hat"].numpy(), g13["res_x_hat"], rtol=1e-6, atol=1e-7)
    _check_lines(capsys.readouterr().out, res, g13, "res", t0, torch.from_numpy(g13["res_x_hat"]), test, orig)


def test_evaluate_real_is_the_scripts_tail(g13, eager_hooks, monkeypatch, capsys):
    T, t0, obs, n_static, n_val, n_test = _meta(g13)
    test = _fold(g13, "test_")
    log = []
    x_hat = torch.from_numpy(g13["ens_test_x_hat_m"])
    vi = _Recorded({n_test: x_hat}, log, "m")
    orig, used = _reseeded_bootstrap(monkeypatch, [5, 6, 7, 8])
    capsys.readouterr()
    res = training_utils.evaluate_real(vi, test, t0)
    lines = capsys.readouterr().out.strip().split("\n")
    assert log == [("m", "enc", t0, 1 + n_static), ("m", "dec", T, 1)] and res["x_hat"] is x_hat
    per = eager.script_rmse(x_hat, test["measurements"], test["masks"], t0, HORIZONS)
    for h, line in enumerate(lines):
        torch.manual_seed(5 + h)
        sd = orig(per[h][0])
        assert line.rsplit(",", 1)[0] == "rmse_x,{:.4f},{:.4f}".format(t0 + HORIZONS[h], per[h][1])
        np.testing.assert_allclose(res["rmse_sd"][h], sd, rtol=1e-4)
        np.testing.assert_allclose(res["rmse"][h], per[h][1], rtol=1e-6)


# -------------------------------------------------------------------------------------------- libhode_blend.so ABI
@pytest.fixture(scope="module")
def blend_lib():
    from hode import _blend_lib as BL
    return abi_checks.built(BL.LIBRARY)


def test_header_functions_are_exported_and_bound(blend_lib):
    from hode import _blend_lib as BL
    src = abi_checks.header_text("hode_blend.h")
    declared = abi_checks.declared_functions("hode_blend.h", "hode_blend_")
    assert declared == {name for name, _, _ in BL.EXPORTS} == {"hode_blend_version", "hode_blend_last_error_string",
                                                               "hode_blend_nnls2", "hode_blend_horizon_sse"}
    for name in declared:
        assert getattr(blend_lib, name) is not None
    assert blend_lib.hode_blend_version() == BL.HODE_BLEND_ABI_VERSION == int(re.search(r"#define HODE_BLEND_ABI_VERSION (\d+)", src).group(1))
    assert int(re.search(r"#define HODE_BLEND_MAX_OBS (\d+)", src).group(1)) == BL.MAX_OBS
    assert int(re.search(r"#define HODE_BLEND_MAX_HORIZONS (\d+)", src).group(1)) == BL.MAX_HORIZONS
    codes = dict(re.findall(r"#define (HODE_BLEND_E_[A-Z]+) (-\d+)", src))
    assert (int(codes["HODE_BLEND_E_NULL"]), int(codes["HODE_BLEND_E_SIZE"])) == (BL.E_NULL, BL.E_SIZE)
    assert int(re.search(r"constexpr int kWaveRows = (\d+);", open(BLEND_SRC).read()).group(1)) == bcases.WAVE_ROWS


@pytest.mark.parametrize("cls,ctype", [("Nnls2Desc", "hode_blend_nnls2_desc"), ("HorizonDesc", "hode_blend_horizon_desc")])
def test_struct_size_matches_the_c_header(tmp_path, cls, ctype):
    from hode import _blend_lib as BL
    abi_checks.assert_c_layout("hode_blend.h", ctype, getattr(BL, cls), tmp_path)


def _horizon_desc(obs=24, H=4, ends=HORIZONS):
    from hode import _blend_lib as BL
    d = BL.new_desc(BL.HorizonDesc)
    d.n_times, d.batch, d.obs_dim, d.n_horizons = 73, 7, obs, H
    for h, n in enumerate(ends):
        d.horizons[h] = n
    d.time_stride, d.patient_stride = 7 * obs, obs
    return d


def _nnls_desc():
    from hode import _blend_lib as BL
    d = BL.new_desc(BL.Nnls2Desc)
    d.n_steps, d.rows = 5, 15
    d.step_stride_e = d.step_stride_m = d.step_stride_b = 15
    return d


def test_argument_errors_do_not_launch(blend_lib):
    from hode import _blend_lib as BL
    for fn, make in ((blend_lib.hode_blend_nnls2, _nnls_desc), (blend_lib.hode_blend_horizon_sse, _horizon_desc)):
        assert fn(None, None) == BL.E_NULL and b"NULL" in blend_lib.hode_blend_last_error_string()
        d = make()
        d.struct_size = 8
        assert fn(d, None) == BL.E_SIZE and b"struct_size" in blend_lib.hode_blend_last_error_string()
        assert fn(make(), None) == BL.E_NULL      # a shape of the domain, pointers missing: nothing is launched
    for field, bad in (("n_steps", 0), ("rows", 0), ("rows", 2 ** 31), ("step_stride_e", -1), ("step_stride_b", -1)):
        d = _nnls_desc()
        setattr(d, field, bad)
        assert blend_lib.hode_blend_nnls2(d, None) == BL.E_SIZE, field
    for field, bad in (("n_times", 0), ("batch", 0), ("obs_dim", 0), ("obs_dim", 129), ("n_horizons", 0), ("n_horizons", 9),
                       ("time_stride", -1), ("patient_stride", -1)):
        d = _horizon_desc()
        setattr(d, field, bad)
        assert blend_lib.hode_blend_horizon_sse(d, None) == BL.E_SIZE, field
    assert blend_lib.hode_blend_horizon_sse(_horizon_desc(obs=128, H=8, ends=(1, 2, 3, 4, 5, 6, 7, 8)), None) == BL.E_NULL
    for ends in ((6, 12, 11, 72), (0, 12, 24, 72)):
        assert blend_lib.hode_blend_horizon_sse(_horizon_desc(ends=ends), None) == BL.E_SIZE
        assert b"non-decreasing" in blend_lib.hode_blend_last_error_string()
    d = _horizon_desc()
    d.n_times, d.batch = 65536, 32768
    assert blend_lib.hode_blend_horizon_sse(d, None) == BL.E_SIZE and b"2^31" in blend_lib.hode_blend_last_error_string()
    d = _horizon_desc()
    for f in ("x_e", "truth", "mask", "sse", "cnt", "w_m"):
        setattr(d, f, 16)
    assert blend_lib.hode_blend_horizon_sse(d, None) == BL.E_NULL and b"w_m without x_m" in blend_lib.hode_blend_last_error_string()


def test_the_binding_refuses_what_is_outside_the_domain():
    from hode import HodeConfigError, blend
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(HodeConfigError, match="HIP device"):
        blend.nnls2_weights(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4))
    with pytest.raises(HodeConfigError, match="HIP device"):
        blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4), HORIZONS)
    with pytest.raises(HodeConfigError, match="obs 129"):
        blend.horizon_sse(z(5, 3, 129), z(5, 3, 129), z(5, 3, 129), HORIZONS)
    with pytest.raises(HodeConfigError, match="9 horizons"):
        blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4), range(1, 10))
    with pytest.raises(HodeConfigError, match="0 horizons"):
        blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4), ())
    for ends in ((6, 12, 11, 72), (0, 1)):
        with pytest.raises(HodeConfigError, match="non-decreasing"):
            blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4), ends)
    for bad in (dict(x_m=z(5, 3, 5)), dict(weight_e=z(4, 4)), dict(weight_e=z(5, 2, 4)), dict(weight_m=0.5)):
        with pytest.raises(HodeConfigError, match="shape|weight_m without x_m"):
            blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 3, 4), HORIZONS, **bad)
    with pytest.raises(HodeConfigError, match="shape"):
        blend.horizon_sse(z(5, 3, 4), z(5, 3, 4), z(5, 4, 4), HORIZONS)
    with pytest.raises(HodeConfigError, match="shape"):
        blend.nnls2_weights(z(5, 3, 4), z(5, 3, 5), z(5, 3, 4))
    with pytest.raises(HodeConfigError, match="every dimension"):
        blend.nnls2_weights(z(0, 3, 4), z(0, 3, 4), z(0, 3, 4))
    with pytest.raises(HodeConfigError, match="every dimension"):
        blend.horizon_sse(z(5, 0, 4), z(5, 0, 4), z(5, 0, 4), HORIZONS)


def test_every_blend_kernel_is_reached_by_a_gpu_case():
    objs = sorted(glob.glob(os.path.join(BLEND_BUILD, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_variants as kv
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    covered = set().union(*(bcases.kernels(c) for c in bcases.CASES))
    assert compiled, "no kernels found in %s" % BLEND_BUILD
    assert compiled <= covered, sorted(compiled - covered)
    assert covered <= compiled, sorted(covered - compiled)
    assert all(n.startswith("hode_blend::") for n in compiled)  # none is another library's


# --------------------------------------------------------------------------------------------- multi-column dose
def test_multi_column_dose_is_the_summed_single_column():
    """The reference's dose_at_time sums over dims (0, 2): with cat([a, s], -1) as the action every static column is added
    into the dose.  The mirror's eager rhs does the same, and it equals the rhs driven by the one summed column."""
    cpu = torch.device("cpu")
    torch.manual_seed(2)
    T, B, S, D = 12, 5, 3, 4
    ode = model.RocheODEReal(D, 1, S, 9, T, 1.0, device=cpu)
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(T, B, 1, generator=g) < 0.3).float() * torch.rand(T, B, 1, generator=g)
    s = (0.1 + 0.4 * torch.rand(1, B, S, generator=g)).repeat(T, 1, 1)
    a_in = torch.cat([a, s], dim=-1)
    y = torch.randn(B, D, generator=g)
    for t in (0.5, 3.0, 7.5, 11.0):
        tt = torch.tensor(t)
        ode.set_action_static(a_in, s)
        dose_all, rhs_all = ode.dose_at_time(tt), ode(tt, y)
        ode.set_action_static(a_in.sum(-1, keepdim=True), s)
        dose_one, rhs_one = ode.dose_at_time(tt), ode(tt, y)
        ode.set_action_static(a, s)
        dose_first = ode.dose_at_time(tt)
        torch.testing.assert_close(dose_all, dose_one, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(rhs_all, rhs_one, rtol=1e-6, atol=1e-7)
        if t >= 1.0:
            assert (dose_all > dose_first + 0.05).all()   # the statics are in the dose
