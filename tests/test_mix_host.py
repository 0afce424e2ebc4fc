"""CPU checks of the two-model evaluation (no GPU): training_utils.evaluate_ensemble / evaluate_ensemble_horizon against
the reference's own numbers (G12, tests/golden/make_golden_ensemble.py) with the solver and the mixture-CRPS kernel
replaced by their oracles (test-only hooks), the residual and the ensemble flow of the two experiment scripts end to end
on hode.batches folds, libhode_mix.so's C ABI, and the guards that every compiled mix kernel is reached by a case of the
GPU test table and that no accepted shape asks for more LDS than a workgroup has."""
import glob
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

import abi_checks
import mix_cases as mc
import model
import training_utils
from oracle.solvers import odeint as oracle_odeint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_SRC = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "mix", "hode_mix.hip")
MIX_BUILD = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "mix", "build")
CPU = torch.device("cpu")
OBS, ACT, D_EXPERT, D_ML, T, T0, STEP = 20, 1, 4, 6, 10, 5, 0.125


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_ensemble_eval.npz"))


@pytest.fixture
def oracle_hooks(monkeypatch):
    monkeypatch.setattr(training_utils, "_ensemble_crps", mc.oracle_ensemble_crps)
    monkeypatch.setattr(training_utils, "_mixture_crps", mc.oracle_mixture_crps)


def _sd(g, pre):
    return {k[len(pre):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def _pair(t_max=(T - 1) * STEP, step=STEP):
    """The two models of experiments/run_simulation_ensemble.py: expert-only (D 4) and NeuralODE (D 6), on the oracle solver."""
    out = []
    for D, roche in ((D_EXPERT, True), (D_ML, False)):
        enc = model.EncoderLSTM(OBS + ACT, 2 * OBS, D, device=CPU, normalize=roche)
        dec = model.RocheExpertDecoder(OBS, D, ACT, t_max, step, roche=roche, method="rk4", device=CPU)
        dec._odeint = oracle_odeint
        out.append(model.VariationalInference(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density if roche else None,
                                              elbo=True))
    return out


class _Folds:
    expert_dim = D_EXPERT

    def __init__(self, g, pre, n_chunks=None):
        n, bs = int(g[pre + "meta"][0]), int(g[pre + "meta"][1])
        self.test_size = n if n_chunks is None else n_chunks * bs
        self.data = {k: torch.from_numpy(g[pre + "data_" + k]) for k in ("measurements", "masks", "latents", "actions")}

    def get_split(self, fold, bs, chunk=0):
        assert fold == "test"
        return {k: v[:, chunk * bs:(chunk + 1) * bs] for k, v in self.data.items()}


def _run(g, pre):
    expert, ml = _pair()
    for tag, vi in (("e", expert), ("m", ml)):
        vi.encoder.load_state_dict(_sd(g, "%s%s_enc_" % (pre, tag)))
        vi.decoder.load_state_dict(_sd(g, "%s%s_dec_" % (pre, tag)))
    w = [torch.from_numpy(g[pre + k]) if g[pre + k].ndim else float(g[pre + k]) for k in ("w_e", "w_m")]
    return expert, ml, w


@pytest.mark.parametrize("pre", ["s_", "w_"])
def test_evaluate_ensemble_against_the_reference(g12, oracle_hooks, capsys, pre):
    """The reference's numbers on the reference's draws: both sides consume the seeded generator in the same order (per
    iteration the expert's draw, then the ml model's; then the z0 bootstrap, then the x bootstrap), so the bootstrap
    spreads are compared too."""
    n, bs, mc_itr, mc_h, seed, tensor_w, blind = (int(v) for v in g12[pre + "meta"])
    assert n // bs == 2 and not blind and bool(tensor_w) == (pre == "w_")
    expert, ml, (w_e, w_m) = _run(g12, pre)
    capsys.readouterr()
    torch.manual_seed(seed)
    got = training_utils.evaluate_ensemble(expert, ml, _Folds(g12, pre), bs, T0, mc_itr=mc_itr, weight_expert=w_e, weight_ml=w_m)
    lines = capsys.readouterr().out.strip().split("\n")
    ref = g12[pre + "tuple"]
    print(pre, "got", got, "ref", ref)
    assert len(got) == 6
    rmse_z0, rmse_z0_sd, cprs_z0, rmse_x, rmse_x_sd, cprs_x = got
    np.testing.assert_allclose([rmse_z0, cprs_z0, rmse_x], ref[[0, 2, 3]], rtol=1e-5)
    np.testing.assert_allclose(cprs_x, ref[5], rtol=2e-5)
    np.testing.assert_allclose([rmse_z0_sd, rmse_x_sd], ref[[1, 4]], rtol=1e-4)
    assert lines == [str(l) for l in g12[pre + "lines"]]


@pytest.mark.parametrize("pre", ["s_", "w_"])
def test_horizon_against_the_reference_is_the_first_chunk(g12, oracle_hooks, pre):
    n, bs, mc_itr, mc_h, seed, tensor_w, blind = (int(v) for v in g12[pre + "meta"])
    expert, ml, (w_e, w_m) = _run(g12, pre)
    results = []
    for n_chunks in (None, 1):  # the whole test fold, and a fold cut down to its first chunk: the same result
        torch.manual_seed(seed)
        results.append(training_utils.evaluate_ensemble_horizon(expert, ml, _Folds(g12, pre, n_chunks), bs, T0, mc_itr=mc_h,
                                                                weight_expert=w_e, weight_ml=w_m))
    hz, first = results
    assert set(hz) == {"rmse_x", "rmse_x_sd", "cprs_x", "cprs_x_sd"}
    for k in hz:
        print(pre, k, hz[k], g12[pre + "hz_" + k])
        assert hz[k].shape == (T - T0,) and np.array_equal(hz[k], first[k])
    np.testing.assert_allclose(hz["rmse_x"], g12[pre + "hz_rmse_x"], rtol=1e-5)
    np.testing.assert_allclose(hz["cprs_x"], g12[pre + "hz_cprs_x"], rtol=2e-5)
    np.testing.assert_allclose(hz["cprs_x_sd"], g12[pre + "hz_cprs_x_sd"], rtol=1e-4)
    np.testing.assert_allclose(hz["rmse_x_sd"], g12[pre + "hz_rmse_x_sd"], rtol=1e-4)
    assert hz["rmse_x"].dtype == g12[pre + "hz_rmse_x"].dtype
    assert training_utils.evaluate_ensemble_horizon(expert, ml, _Folds(g12, pre, 0), bs, T0, mc_itr=mc_h) is None


def test_unobserved_patient_gives_the_reference_nan(g12, oracle_hooks, capsys):
    """evaluate_ensemble does not drop NaN entries (reference :473-475): rmse_x and its spread are NaN; the horizon's
    nanmean survives, its raw-row bootstrap does not."""
    pre = "n_"
    n, bs, mc_itr, mc_h, seed, tensor_w, blind = (int(v) for v in g12[pre + "meta"])
    assert blind
    expert, ml, (w_e, w_m) = _run(g12, pre)
    capsys.readouterr()
    torch.manual_seed(seed)
    got = training_utils.evaluate_ensemble(expert, ml, _Folds(g12, pre), bs, T0, mc_itr=mc_itr, weight_expert=w_e, weight_ml=w_m)
    lines = capsys.readouterr().out.strip().split("\n")
    ref = g12[pre + "tuple"]
    assert np.isnan(ref[3]) and np.isnan(ref[4]) and np.isnan(got[3]) and np.isnan(got[4])
    np.testing.assert_allclose([got[0], got[2]], ref[[0, 2]], rtol=1e-5)
    np.testing.assert_allclose(got[5], ref[5], rtol=2e-5)
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-4)
    assert lines == [str(l) for l in g12[pre + "lines"]] and lines[1] == "rmse_x,nan,nan"
    torch.manual_seed(seed)
    hz = training_utils.evaluate_ensemble_horizon(expert, ml, _Folds(g12, pre), bs, T0, mc_itr=mc_h, weight_expert=w_e, weight_ml=w_m)
    np.testing.assert_allclose(hz["rmse_x"], g12[pre + "hz_rmse_x"], rtol=1e-5)
    assert np.isfinite(hz["rmse_x"]).all() and np.isnan(g12[pre + "hz_rmse_x_sd"]).all() and np.isnan(hz["rmse_x_sd"]).all()
    np.testing.assert_allclose(hz["cprs_x"], g12[pre + "hz_cprs_x"], rtol=2e-5)


def test_forecast_weights_are_sliced_on_the_host():
    w = torch.arange(T * OBS, dtype=torch.float32).reshape(T, 1, OBS)
    assert torch.equal(training_utils._forecast_weight(w, T0), w[T0:, 0, :])
    assert training_utils._forecast_weight(1, T0) is None and training_utils._forecast_weight(1.0, T0) is None
    assert training_utils._forecast_weight(0.25, T0) == 0.25 and training_utils._forecast_weight(torch.tensor(0.5), T0) == 0.5


def test_product_mixture_crps_refuses_cpu_tensors():
    import hode
    from hode import mix
    lin_e, lin_m = torch.nn.Linear(4, 3), torch.nn.Linear(6, 3)
    with pytest.raises(hode.HodeConfigError):
        mix.mixture_crps(torch.zeros(1, 4, 4), torch.zeros(1, 4, 6), torch.zeros(1, 2, 3), 2, lin_e, lin_m)


# ------------------------------------------------------------------------------- the two scripts' flows, end to end
def _folds():
    from hode.batches import DeviceFolds
    return DeviceFolds.synthetic(24, T, OBS, D_ML, 12, 6, CPU, seed=4, step=STEP)


def _four_finite_lines(out):
    lines = out.strip().split("\n")[-4:]
    assert [l.split(",")[0] for l in lines] == ["rmse_z0", "rmse_x", "cprs_z0", "cprs_x"], lines
    assert all(np.isfinite(float(v)) for l in lines for v in l.split(",")[1:]), lines


def test_residual_flow_end_to_end(oracle_hooks, capsys, tmp_path):
    """experiments/run_simulation_residual.py: the validation fold's measurements become the expert's residuals, the
    NeuralODE is trained on that fold, and the sum of the two forecasts (weights 1 / 1) is evaluated."""
    torch.manual_seed(3)
    dg = _folds()
    expert, vi = _pair()
    x, a, mask = (dg.data_val[k] for k in ("measurements", "actions", "masks"))
    with torch.no_grad():
        x_hat, _ = expert.decoder(expert.encoder(x, a, mask)[0], a)
        dg.data_val["measurements"] = (x - x_hat).detach()
    n_val = min(8, x.shape[1])
    dg.set_val_size(n_val)
    assert dg.data_val["measurements"].shape == (T, n_val, OBS) and dg.val_size == n_val
    params = (list(vi.encoder.parameters()) + list(vi.decoder.output_function.parameters())
              + list(vi.decoder.ode.ml_net.parameters()))
    before = [p.detach().clone() for p in params]
    vi, best, _ = training_utils.variational_training_loop(2, dg, vi, 4, torch.optim.Adam(params, lr=0.01), 1,
                                                           path=str(tmp_path) + "/", shuffle=False, train_fold="val")
    assert np.isfinite(best) and any(not torch.equal(p.detach(), q) for p, q in zip(params, before))
    capsys.readouterr()
    out = training_utils.evaluate_ensemble(expert, vi, dg, 3, T0, mc_itr=4)
    _four_finite_lines(capsys.readouterr().out)
    assert len(out) == 6 and all(np.isfinite(v) for v in out)
    hz = training_utils.evaluate_ensemble_horizon(expert, vi, dg, 3, T0, mc_itr=3)
    assert all(np.isfinite(hz[k]).all() and hz[k].shape == (T - T0,) for k in ("rmse_x", "cprs_x", "cprs_x_sd"))


def test_ensemble_flow_end_to_end(oracle_hooks, capsys):
    """experiments/run_simulation_ensemble.py: one non-negative stacking weight pair per forecast step from the
    validation fold (scipy's NNLS), handed over as (T, 1, obs) tensors."""
    nnls = pytest.importorskip("scipy.optimize").nnls
    torch.manual_seed(5)
    dg = _folds()
    expert, ml = _pair()
    x, a, mask = (dg.data_val[k][:, :10] for k in ("measurements", "actions", "masks"))
    with torch.no_grad():
        x_hat, _ = expert.decoder(expert.encoder(x, a, mask)[0], a)
        x_hat_ml, _ = ml.decoder(ml.encoder(x, a, mask)[0], a)
    w_e, w_m = torch.zeros(T, 1, OBS), torch.zeros(T, 1, OBS)
    for i in range(T0, T):
        A = np.stack([x_hat[i].numpy().flatten(), x_hat_ml[i].numpy().flatten()], axis=1)
        w, _ = nnls(A, x[i].numpy().flatten())
        w_e[i, 0, :], w_m[i, 0, :] = float(w[0]), float(w[1])
    assert (w_e >= 0).all() and (w_m >= 0).all()
    capsys.readouterr()
    out = training_utils.evaluate_ensemble(expert, ml, dg, 3, T0, mc_itr=4, weight_expert=w_e, weight_ml=w_m)
    _four_finite_lines(capsys.readouterr().out)
    assert len(out) == 6 and all(np.isfinite(v) for v in out)
    hz = training_utils.evaluate_ensemble_horizon(expert, ml, dg, 3, T0, weight_expert=w_e, weight_ml=w_m)
    assert all(np.isfinite(hz[k]).all() and hz[k].shape == (T - T0,) for k in ("rmse_x", "cprs_x", "cprs_x_sd"))


def test_oracle_stand_in_is_the_reference_loop():
    """The fp64 stand-in against the reference's own arithmetic: two torch readouts, the mix, crps_ensemble per element."""
    from oracle.evalmetrics import crps_ensemble
    c = mc.Case(5, 4, 6, 3, 2, 2, True, True, True)
    i = mc.inputs(c, 1)
    got = mc.oracle_mixture_crps(i["h_e"], i["h_m"], i["truth"], c.M, (i["w_e"], i["b_e"]), (i["w_m"], i["b_m"]),
                                 i["g_e"], i["g_m"], per_component=True)
    xe = (i["h_e"] @ i["w_e"].t() + i["b_e"]).reshape(c.Tn, c.M, c.B, c.obs) * i["g_e"][:, None, None, :]
    xm = (i["h_m"] @ i["w_m"].t() + i["b_m"]).reshape(c.Tn, c.M, c.B, c.obs) * i["g_m"][:, None, None, :]
    x = (xe + xm).numpy()
    for t in range(c.Tn):
        for b in range(c.B):
            for o in range(c.obs):
                assert got[t, b, o].item() == pytest.approx(crps_ensemble(i["truth"][t, b, o].item(), x[t, :, b, o]), rel=1e-5, abs=1e-7)
    ref, scale = mc.mix_oracle(i["h_e"], i["h_m"], i["truth"], c.M, i["w_e"], i["b_e"], i["w_m"], i["b_m"], i["g_e"], i["g_m"])
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-7)
    assert (scale > 0).all()


# ------------------------------------------------------------------------------------------------ libhode_mix.so ABI
@pytest.fixture(scope="module")
def mix_lib():
    from hode import _mix_lib as M
    return abi_checks.built(M.LIBRARY)


def test_header_functions_are_exported_and_bound(mix_lib):
    from hode import _mix_lib as M
    src = abi_checks.header_text("hode_mix.h")
    declared = abi_checks.declared_functions("hode_mix.h", "hode_mix_")
    assert declared == {name for name, _, _ in M.EXPORTS} == {"hode_mix_version", "hode_mix_last_error_string", "hode_mix_crps"}
    for name in declared:
        assert getattr(mix_lib, name) is not None
    assert mix_lib.hode_mix_version() == M.HODE_MIX_ABI_VERSION == int(re.search(r"#define HODE_MIX_ABI_VERSION (\d+)", src).group(1))
    assert int(re.search(r"#define HODE_MIX_MAX_DIM (\d+)", src).group(1)) == M.MAX_DIM
    codes = dict(re.findall(r"#define (HODE_MIX_E_[A-Z]+) (-\d+)", src))
    assert (int(codes["HODE_MIX_E_NULL"]), int(codes["HODE_MIX_E_SIZE"]), int(codes["HODE_MIX_E_UNSUPPORTED"])) == \
        (M.E_NULL, M.E_SIZE, M.E_UNSUPPORTED)


def test_struct_size_matches_the_c_header(tmp_path):
    from hode import _mix_lib as M
    abi_checks.assert_c_layout("hode_mix.h", "hode_mix_crps_desc", M.MixCrpsDesc, tmp_path)


def _shape_desc(obs=20, M_=50, De=4, Dm=6):
    from hode import _mix_lib as M
    d = M.new_desc()
    d.n_times, d.batch, d.n_members, d.obs_dim, d.latent_dim_e, d.latent_dim_m = 9, 7, M_, obs, De, Dm
    return d


def test_argument_errors_do_not_launch(mix_lib):
    from hode import _mix_lib as M
    assert mix_lib.hode_mix_crps(None, None) == M.E_NULL and b"NULL" in mix_lib.hode_mix_last_error_string()
    d = _shape_desc()
    d.struct_size = 8
    assert mix_lib.hode_mix_crps(d, None) == M.E_SIZE and b"struct_size" in mix_lib.hode_mix_last_error_string()
    assert mix_lib.hode_mix_crps(_shape_desc(), None) == M.E_NULL  # a shape of the domain, pointers missing
    for field, bad in (("n_times", 0), ("batch", 0), ("n_members", 0), ("n_members", 129), ("obs_dim", 0), ("obs_dim", 129),
                       ("latent_dim_e", 0), ("latent_dim_e", 129), ("latent_dim_m", 0), ("latent_dim_m", 129),
                       ("time_stride_e", -1), ("patient_stride_m", -1)):
        e = _shape_desc()
        setattr(e, field, bad)
        assert mix_lib.hode_mix_crps(e, None) == M.E_SIZE, field
    e = _shape_desc()
    e.n_times, e.batch = 65536, 32768
    assert mix_lib.hode_mix_crps(e, None) == M.E_SIZE and b"2^31" in mix_lib.hode_mix_last_error_string()
    assert mix_lib.hode_mix_crps(_shape_desc(*mc.FIRST_REFUSED[:1], mc.FIRST_REFUSED[3], *mc.FIRST_REFUSED[1:3]), None) == M.E_UNSUPPORTED
    assert b"LDS" in mix_lib.hode_mix_last_error_string()
    assert mix_lib.hode_mix_crps(_shape_desc(*mc.LARGEST[:1], mc.LARGEST[3], *mc.LARGEST[1:3]), None) == M.E_NULL
    # an output is required even when every input is there (the pointers are never read: nothing launches)
    e = _shape_desc()
    for f in ("h_e", "h_m", "w_e", "w_m", "truth"):
        setattr(e, f, 16)
    assert mix_lib.hode_mix_crps(e, None) == M.E_NULL and b"nothing to compute" in mix_lib.hode_mix_last_error_string()


# --------------------------------------------------------------------------------------------- kernel accounting
def _mix_objects():
    objs = sorted(glob.glob(os.path.join(MIX_BUILD, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    return objs


def test_every_mix_kernel_is_reached_by_a_gpu_case():
    objs = _mix_objects()
    import kernel_variants as kv
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    covered = set().union(*(mc.kernels(c) for c in mc.CASES))
    assert compiled, "no kernels found in %s" % MIX_BUILD
    assert compiled <= covered, sorted(compiled - covered)
    assert covered <= compiled, sorted(covered - compiled)
    assert not any(n.startswith("hode::") or n.startswith("hode_flow::") for n in compiled)  # none is another library's


def _source_rule():
    """The host's LDS rule, read from hode_mix.hip: its constants and the body of mix_lds_bytes as a Python expression."""
    src = open(MIX_SRC).read()
    consts = {}
    for name, expr in re.findall(r"constexpr (?:int|size_t) (kMix[A-Za-z]+) = ([^;]+);", src):
        consts[name] = eval(expr.replace("sizeof(float)", "4"), {}, dict(consts))
    body = re.search(r"static size_t mix_lds_bytes\(int rpw, int M, int De, int Dm, int obs\) \{\s*return ([^;]+);", src).group(1)
    body = body.replace("sizeof(float)", "4").replace("(size_t)", "")
    return consts, lambda rpw, M, De, Dm, obs: eval(body, {}, dict(consts, rpw=rpw, M=M, De=De, Dm=Dm, obs=obs))


def test_no_accepted_shape_exceeds_the_lds_of_a_workgroup(mix_lib):
    from hode import _mix_lib as M, mix
    from kernel_descriptor import kernel_descriptors
    objs = _mix_objects()
    consts, lds_bytes = _source_rule()
    # group_segment_fixed_size of every kernel descriptor (a symbol may be listed by both symbol tables)
    static = sorted({struct.unpack_from("<I", kd, 0)[0] for o in objs for _, kd in kernel_descriptors(o)})
    assert static == [consts["kMixStaticLds"]] and consts["kMixLdsLimit"] == 160 * 1024
    assert (consts["kMixThreads"], consts["kMixMaxRows"], consts["kMixPackLds"], consts["kMixLdsLimit"], consts["kMixStaticLds"]) == \
        (mix.THREADS, mix.MAX_ROWS, mix.PACK_LDS, mix.LDS_LIMIT, mix.STATIC_LDS)
    worst, accepted, refused = 0, 0, 0
    for obs in range(1, 129):
        for n in (1, 10, 21, 22, 50, 64, 127, 128):
            for De, Dm in ((1, 1), (4, 6), (4, 12), (32, 32), (47, 48), (48, 48), (64, 64), (1, 128), (128, 128)):
                rpw = mix.rows_per_workgroup(n, De, Dm, obs)
                assert 1 <= rpw <= consts["kMixMaxRows"] and rpw * obs <= consts["kMixThreads"]
                assert mix.lds_bytes(rpw, n, De, Dm, obs) == lds_bytes(rpw, n, De, Dm, obs)
                total = lds_bytes(rpw, n, De, Dm, obs) + static[0]
                code = mix_lib.hode_mix_crps(_shape_desc(obs, n, De, Dm), None)
                assert code in (M.E_NULL, M.E_UNSUPPORTED)
                assert (code == M.E_NULL) == mix.supported(n, De, Dm, obs) == (total <= 160 * 1024), (obs, n, De, Dm, total)
                if code == M.E_NULL:
                    worst, accepted = max(worst, total), accepted + 1
                else:
                    refused += 1
    assert accepted and refused and worst <= 160 * 1024
    obs, De, Dm, n = mc.LARGEST
    assert worst == lds_bytes(1, n, De, Dm, obs) + static[0] == 160 * 1024
    for c in mc.CASES:
        assert mix.supported(c.M, c.De, c.Dm, c.obs), c
    assert not mix.supported(mc.FIRST_REFUSED[3], *mc.FIRST_REFUSED[1:3], mc.FIRST_REFUSED[0])
    # what the table says about the packing it exercises
    assert [mix.rows_per_workgroup(50, De, Dm, obs) for obs, De, Dm in mc.SIM_SHAPES] == [6, 3, 1]
    assert [mix.rows_per_workgroup(10, 4, 6, obs) for obs in (1, 64, 65, 128)] == [8, 2, 1, 1]
    assert mix.rows_per_workgroup(128, 4, 6, 20) == 1
