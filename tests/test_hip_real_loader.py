"""``experiments/run_real.py``'s flow on the HIP device, from four pickles through ``dataloader.DataGeneratorReal`` to the
``rmse_x`` lines: batches from the generator and from its ``device_folds()``, the hybrid decoder and a recurrent baseline;
one loss whichever way the batch was cut; and ``tools/make_real_data.py`` read back by the loader.  GPU only.
Sizes: N = 23 (13 / 4 / 6), T = 34, obs 5, 3 statics, D 7, t0 24, batch 4 (tests/test_real_loader.py holds them)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import binding_cases as bc
import model
import training_utils
from test_real_loader import (BATCH, D, FIELDS, HORIZONS, N, OBS, SEED, STATIC, T, T0, TEST, build_vi, check_lines, generator,
                              make_arrays, train_and_evaluate, write_pickles)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data_path(tmp_path_factory):
    return write_pickles(tmp_path_factory.mktemp("real_data"), make_arrays(T, N, OBS, STATIC, seed=21))


def _generator(data_path, dev):
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    dg = generator(data_path, device=dev)
    dg.split_sample()
    assert all(getattr(dg, k).device == dev for k in FIELDS)
    assert (dg.train_size, dg.val_size, dg.data_test["statics"].shape[1], dg.t_max, dg.static_dim) == (13, 4, TEST, T, STATIC)
    return dg


@pytest.mark.parametrize("source,kind", [("generator", "hybrid"), ("device_folds", "hybrid"), ("generator", "tlstm")])
def test_run_real_flow(data_path, source, kind, tmp_path, capsys):
    dev = _dev()
    dg = _generator(data_path, dev)
    batches = dg if source == "generator" else dg.device_folds()
    vi = build_vi(dg, dev, kind)
    path = str(tmp_path) + "/model/"
    best, lines, res = train_and_evaluate(batches, vi, path, capsys)
    assert np.isfinite(best) and best < 1e9
    ck = torch.load(path + vi.model_name, map_location=dev)
    again = build_vi(dg, dev, kind)
    again.encoder.load_state_dict(ck["encoder_state_dict"])
    again.decoder.load_state_dict(ck["decoder_state_dict"])
    assert ck["best_loss"] == best
    assert all(torch.equal(p, q) for p, q in zip(again.parameters(), vi.parameters()))   # the loop reloads its best checkpoint
    assert tuple(res["x_hat"].shape) == (T - T0, TEST, OBS) and torch.isfinite(res["x_hat"]).all()
    check_lines(lines, res)


def test_one_loss_however_the_batch_was_cut(data_path):
    """The generator's minibatch, ``device_folds()``'s under the same numpy state and the same patients sliced by hand from
    the loaded tensors: the loss runs the LSTM encoder, the real-data hybrid solver and the MLP readout, all listed as
    bit-reproducible in tests/binding_cases.py, so the three losses and their gradients are equal bit for bit."""
    dev = _dev()
    assert all(op in bc.DETERMINISTIC for op in ("lstm_encode", "real", "readout_mlp"))
    dg = _generator(data_path, dev)
    folds = dg.device_folds()
    vi = build_vi(dg, dev)
    state = np.random.get_state()
    idx = torch.as_tensor(np.random.choice(dg.train_size, BATCH, replace=False)).to(dev)
    by_hand = {k: getattr(dg, k)[:, :dg.train_size][:, idx] for k in FIELDS}
    np.random.set_state(state)
    from_generator = dg.get_mini_batch("train", BATCH)
    np.random.set_state(state)
    from_folds = folds.get_mini_batch("train", BATCH)
    results = []
    for batch in (from_generator, from_folds, by_hand):
        assert all(torch.equal(batch[k], by_hand[k]) for k in FIELDS)
        for p in vi.parameters():
            p.grad = None
        loss = vi.loss(batch)
        loss.backward()
        assert torch.isfinite(loss)
        results.append([loss.detach().clone()] + [p.grad.clone() for p in vi.parameters() if p.grad is not None])
    for other in results[1:]:
        assert len(other) == len(results[0]) and all(torch.equal(a, b) for a, b in zip(results[0], other))


def test_make_real_data_is_read_back_by_the_loader(tmp_path):
    dev = _dev()
    spec = importlib.util.spec_from_file_location("make_real_data", os.path.join(ROOT, "tools", "make_real_data.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    outs = [str(tmp_path / name) for name in ("a", "b")]
    for out in outs:
        tool.main(["--out", out, "--patients", str(N), "--hours", str(T), "--labs", str(OBS), "--statics", str(STATIC),
                   "--seed", "7", "--data_type", "5", "--device", str(dev)])
    names = sorted(os.listdir(outs[0]))
    assert names == ["README.txt", "array_at5.pkl", "array_x_constant.pkl", "array_xt5.pkl", "array_xt_mask5.pkl"]
    for name in names:                                            # one seed, one data set
        with open(os.path.join(outs[0], name), "rb") as f, open(os.path.join(outs[1], name), "rb") as g:
            assert f.read() == g.read(), name
    assert "synthetic" in open(os.path.join(outs[0], "README.txt")).read().lower()
    dg = generator(outs[0] + "/", device=dev)
    assert (dg.time_dim, dg.n_sample, dg.obs_dim, dg.static_dim, dg.action_dim) == (T, N, OBS, STATIC, 1)
    for k, last in (("measurements", OBS), ("masks", OBS), ("actions", 1), ("statics", STATIC), ("latents", 4)):
        x = getattr(dg, k)
        assert tuple(x.shape) == (T, N, last) and x.dtype == torch.float32 and x.device == dev and torch.isfinite(x).all(), k
    assert bool(((dg.masks == 0) | (dg.masks == 1)).all()) and 0 < dg.masks.mean() < 1
    roche = tool.generator(N, T, OBS, 7, dev)
    assert torch.equal(dg.actions, roche.actions) and int((roche.actions != 0).sum()) > 0
    assert torch.equal(dg.measurements, roche.measurements) and torch.equal(dg.masks, roche.masks)
    assert torch.equal(dg.statics[0], dg.statics[-1]) and dg.statics.std() > 0.5
