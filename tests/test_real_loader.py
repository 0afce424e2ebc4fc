"""``dataloader.DataGeneratorReal`` on the CPU (no GPU): against G20, the fixture recorded from the REFERENCE's class
(tests/golden/make_golden_real_loader.py) -- attributes, coefficients, folds, minibatches, ``set_train_size`` and numpy's
stream position, bit for bit; its refusals; tensor-valued pickles; the pickle round trip; ``set_device``;
``device_folds()``; and ``experiments/run_real.py``'s flow from four pickles to the ``rmse_x`` lines, with the oracle solver
and the eager horizon score behind the tests' swap points (tests/test_golden_real.py, tests/test_blend_host.py)."""
import os
import pickle

import numpy as np
import pytest
import torch

import blend_eager as eager
import dataloader
import model
import sim_config
import training_utils
from oracle.solvers import odeint as oracle_odeint

CPU = torch.device("cpu")
FIELDS = ("measurements", "actions", "latents", "masks", "statics")
FILES = ("array_xt_mask5", "array_xt5", "array_at5", "array_x_constant")
VAL, TEST, SEED = 4, 6, 666


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_real_loader.npz"), allow_pickle=False)


def write_pickles(path, arrays, as_tensor=False):
    for name in FILES:
        with open(os.path.join(str(path), name + ".pkl"), "wb") as f:
            pickle.dump(torch.from_numpy(arrays[name].copy()) if as_tensor else arrays[name], f)
    return str(path) + "/"


def make_arrays(T, N, obs, n_static, seed):
    """Seeded DDW-shaped arrays (shared with tests/test_hip_real_loader.py): one dose per patient inside the window."""
    rng = np.random.RandomState(seed)
    act = np.zeros((T, N, 1), dtype=np.float32)
    act[rng.randint(0, T - 1, N), np.arange(N), 0] = rng.rand(N).astype(np.float32) + 0.1
    return {"array_xt_mask5": (rng.rand(T, N, obs) < 0.6).astype(np.float32),
            "array_xt5": (0.5 * rng.randn(T, N, obs)).astype(np.float32), "array_at5": act,
            "array_x_constant": (0.1 + 0.4 * rng.rand(N, n_static)).astype(np.float32)}


def generator(data_path, n_sample=23, latent_dim=4, device=CPU, **kw):
    return dataloader.DataGeneratorReal(n_sample, 1, 1, 1, sim_config.RochConfig(), 1, val_size=VAL, test_size=TEST,
                                        latent_dim=latent_dim, device=device, data_type="5", data_path=data_path, **kw)


@pytest.fixture
def g20_path(g20, tmp_path):
    return write_pickles(tmp_path, {k: g20["in_" + k] for k in FILES})


def _same(batch, g, prefix):
    assert tuple(batch) == FIELDS
    for k in FIELDS:
        got = batch[k].numpy()
        assert got.dtype == np.float32 and np.array_equal(got, g[prefix + k]), prefix + k


# ------------------------------------------------------------------------------------------------------------- G20
@pytest.mark.parametrize("n_sample", [23, 20])
def test_g20_attributes_folds_batches_and_stream_are_the_references(g20, g20_path, n_sample, capsys):
    pre = "n%d_" % n_sample
    np.random.seed(SEED)
    dg = generator(g20_path, n_sample)
    assert type(dg.t_max) is int and type(dg.step_size) is float
    got = np.array([float(getattr(dg, str(k))) for k in g20["scalar_names"]])
    assert np.array_equal(got, g20[pre + "scalars"]), dict(zip(g20["scalar_names"], got))
    assert (dg.time_dim, dg.n_sample, dg.obs_dim, dg.static_dim, dg.train_size) == (30, 23, 5, 3, n_sample - VAL - TEST)
    assert np.array_equal(dg.output_coef, g20[pre + "output_coef"]) and dg.ml_coef.shape == g20[pre + "ml_coef"].shape
    assert np.array_equal(dg.ml_coef, g20[pre + "ml_coef"])
    assert dg.data_train is None
    dg.split_sample()
    for fold in ("train", "val", "test"):
        _same(getattr(dg, "data_" + fold), g20, pre + fold + "_")
    assert dg.data_test["statics"].shape[1] == 23 - (n_sample - VAL - TEST) - VAL   # everything behind train + val
    for i in range(3):
        _same(dg.get_mini_batch("train", 5), g20, pre + "mini%d_" % i)
    _same(dg.get_split("val", 2, 1), g20, pre + "split_")
    capsys.readouterr()
    dg.set_train_size(8)
    assert capsys.readouterr().out.strip().split("\n") == [str(l) for l in g20[pre + "set_train_prints"]]
    assert [dg.n_sample, dg.train_size] == list(g20[pre + "after_set_train"]) == [8 + VAL + TEST, 8]
    _same(dg.data_train, g20, pre + "cut_train_")
    assert np.random.rand() == g20[pre + "next_rand"].item()


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals(g20, g20_path):
    with pytest.raises(AssertionError, match=r"\(30, 23, 5\).*\(30, 23, 7\)"):
        generator(g20_path, latent_dim=7)                      # latents are cut from a tensor shaped like the masks
    os.remove(g20_path + "array_at5.pkl")
    with pytest.raises(FileNotFoundError, match="array_at5.pkl"):
        generator(g20_path)
    with open(g20_path + "array_at5.pkl", "wb") as f:
        pickle.dump(g20["in_array_at5"].tolist(), f)
    with pytest.raises(TypeError, match="array_at5.pkl"):
        generator(g20_path)
    with open(g20_path + "array_at5.pkl", "wb") as f:
        pickle.dump(g20["in_array_at5"][:, :, [0, 0]], f)
    with pytest.raises(AssertionError, match=r"actions.*\(30, 23, 2\).*\(30, 23, 1\)"):
        generator(g20_path)


def test_tensor_valued_pickles_load_like_arrays(g20, g20_path, tmp_path):
    os.makedirs(str(tmp_path / "t"))
    tensor_path = write_pickles(tmp_path / "t", {k: g20["in_" + k].astype(np.float64) for k in FILES}, as_tensor=True)
    a, b = generator(g20_path), generator(tensor_path)
    for k in FIELDS:
        assert getattr(b, k).dtype == torch.float32 and torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------- pickling and set_device
def test_pickle_round_trip_keeps_everything(g20_path):
    np.random.seed(SEED)
    dg = generator(g20_path, 20)
    dg.split_sample()
    back = pickle.loads(pickle.dumps(dg))
    assert type(back) is dataloader.DataGeneratorReal and set(back.__dict__) == set(dg.__dict__)
    for k, v in dg.__dict__.items():
        w = back.__dict__[k]
        if torch.is_tensor(v):
            assert torch.equal(v, w) and w.device.type == "cpu", k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, w), k
        elif isinstance(v, dict):
            assert tuple(w) == FIELDS and all(torch.equal(v[f], w[f]) for f in FIELDS), k
        elif k != "roche_config":
            assert v == w, k
    assert tuple(back.roche_config) == tuple(dg.roche_config)
    assert tuple(back.get_split("test", 3, 1)["statics"].shape) == (30, 3, 3)


def test_set_device_moves_statics_everywhere(g20_path):
    dg = generator(g20_path)
    dg.split_sample()
    meta = torch.device("meta")
    dg.set_device(meta)
    assert dg.device == meta
    for k in FIELDS:
        assert getattr(dg, k).device == meta, k
        for fold in (dg.data_train, dg.data_val, dg.data_test):
            assert fold[k].device == meta, k


# ------------------------------------------------------------------------------------------------- device_folds
def test_device_folds_on_the_cpu(g20, g20_path):
    from hode.batches import DeviceFolds
    np.random.seed(SEED)
    dg = generator(g20_path, 20)
    dg.split_sample()
    folds = dg.device_folds()
    assert type(folds) is DeviceFolds and folds.device == CPU and folds.fields == FIELDS
    assert (folds.train_size, folds.val_size, folds.test_size) == (dg.train_size, dg.val_size, dg.test_size) == (10, 4, 6)
    for name in ("train", "val", "test"):
        mine, theirs = getattr(dg, "data_" + name), getattr(folds, "data_" + name)
        assert all(torch.equal(mine[k], theirs[k]) and theirs[k].is_contiguous() for k in FIELDS), name
    assert folds.data_test["statics"].shape[1] == 9
    state = np.random.get_state()
    mine = [dg.get_mini_batch("train", 5) for _ in range(3)]
    np.random.set_state(state)
    for want in mine:
        got = folds.get_mini_batch("train", 5)
        assert tuple(got) == FIELDS
        assert all(torch.equal(got[k], want[k]) and got[k].is_contiguous() for k in FIELDS)
    _same(mine[0], g20, "n20_mini0_")                                    # and those are the reference's patients
    part = folds.get_split("val", 2, 1)
    assert all(torch.equal(part[k], dg.get_split("val", 2, 1)[k]) and part[k].is_contiguous() for k in FIELDS)
    whole = folds.get_split("test", 9, 0)
    assert all(whole[k] is folds.data_test[k] for k in FIELDS)           # a whole fold: the stored tensor itself
    assert dg.device_folds(index_rng="device").index_rng == "device"


# -------------------------------------------------------------------------------------------- run_real.py's flow
T, N, OBS, STATIC, D, T0, BATCH, HORIZONS = 34, 23, 5, 3, 7, 24, 4, (2, 6)


def build_vi(dg, device, kind="hybrid"):
    """``experiments/run_real.py`` :38-72 (shared with tests/test_hip_real_loader.py)."""
    input_dim = dg.obs_dim + dg.action_dim + dg.static_dim + 1
    hidden_dim = int((dg.obs_dim + dg.action_dim + dg.static_dim) * 1.2)
    encoder = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=device)
    if kind == "hybrid":
        decoder = model.DecoderReal(dg.obs_dim, D, dg.action_dim, dg.static_dim, hidden_dim, dg.t_max, dg.step_size,
                                    method="midpoint", ode_step_size=dg.step_size / 1, ode_type="hybrid", t0=T0, device=device)
    else:
        decoder = model.DecoderRealBenchmark(dg.obs_dim, D, dg.action_dim, dg.static_dim, hidden_dim, dg.t_max, dg.step_size,
                                             ode_type=kind, t0=T0, device=device)
    return model.VariationalInferenceReal(encoder, decoder, elbo=False, t0=T0, weight=False)


def train_and_evaluate(source, vi, path, capsys):
    """:85-137 with two iterations: returns (best loss, the ``rmse_x`` lines, evaluate_real's result)."""
    params = list(vi.encoder.parameters()) + list(vi.decoder.parameters())
    optimizer = torch.optim.Adam(params, lr=0.01)
    vi, best, _ = training_utils.variational_training_loop(niters=2, data_generator=source, model=vi, batch_size=BATCH,
                                                           optimizer=optimizer, test_freq=1, path=path, best_on_disk=1e9,
                                                           early_stop=10, shuffle=False)
    capsys.readouterr()
    res = training_utils.evaluate_real(vi, source.data_test, T0, horizons=HORIZONS)
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if l.startswith("rmse_x,")]
    return best, lines, res


def check_lines(lines, res):
    assert len(lines) == len(HORIZONS)
    for line, n, rmse, sd in zip(lines, HORIZONS, res["rmse"], res["rmse_sd"]):
        assert line == "rmse_x,{:.4f},{:.4f},{:.4f}".format(T0 + n, rmse, sd)      # run_real.py:137
        assert np.isfinite(rmse) and np.isfinite(sd)


def test_run_real_flow_on_the_cpu(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(training_utils, "_horizon_sse", lambda *a, **k: tuple(v.float() for v in eager.horizon_sse(*a, **k)))
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    os.makedirs(str(tmp_path / "data"))
    data_path = write_pickles(tmp_path / "data", make_arrays(T, N, OBS, STATIC, seed=21))
    dg = generator(data_path, latent_dim=4)
    dg.split_sample()
    assert (dg.train_size, dg.t_max, dg.step_size, dg.static_dim) == (13, T, 1.0, STATIC)
    vi = build_vi(dg, CPU)
    vi.decoder._odeint = oracle_odeint           # tests only: the product has no CPU solver
    before = [p.detach().clone() for p in vi.parameters()]
    path = str(tmp_path) + "/model/"
    best, lines, res = train_and_evaluate(dg, vi, path, capsys)
    assert np.isfinite(best) and best < 1e9
    ck = torch.load(path + vi.model_name, map_location="cpu")
    assert ck["best_loss"] == best and set(ck["decoder_state_dict"]) == set(vi.decoder.state_dict())
    assert any(not torch.equal(p.detach(), q) for p, q in zip(vi.parameters(), before))
    assert tuple(res["x_hat"].shape) == (T - T0, TEST, OBS) and torch.isfinite(res["x_hat"]).all()
    check_lines(lines, res)
