"""``model.LSTMBaseline`` and ``model.EncoderLSTMReal(output_all=True)`` on CPU tensors against G17, the fixture recorded from
the REFERENCE's classes (tests/golden/make_golden_lstm_seq.py; reference model.py:322-380, :180-242), under the bounds
tests/test_golden_real.py holds the encoder fixture to: loss 2e-5 relative, outputs 2e-6 (1 + max|.|) absolute, parameter
gradients 2e-4 rel-L2.  Also the reference's ``state_dict`` keys and shapes and the ``save`` file.  The GPU counterpart on the
same fixture is tests/test_hip_lstm_seq.py, which shares the loaders and the checks below."""
import os

import numpy as np
import pytest
import torch

import model

TOL_LOSS, TOL_OUT, TOL_G = 2e-5, 2e-6, 2e-4   # tests/test_golden_real.py: tol_loss, tol_h, tol_g
BASE_KEYS = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
             "out.0.weight", "out.0.bias", "out.2.weight", "out.2.bias"]


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_lstm_seq.npz"), allow_pickle=False)


def _state(g, prefix):
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def load_data(g, device):
    return {k: torch.from_numpy(g[k]).to(device) for k in ("measurements", "actions", "masks", "statics")}


def load_baseline(g, device):
    T, B, obs, act, stat, H, dz = [int(v) for v in g["meta"]]
    base = model.LSTMBaseline(obs + act + stat, H, obs, device=device)
    base.load_state_dict(_state(g, "base_sd_"), strict=True)   # the reference's own keys
    return base


def load_encoder(g, reverse, device):
    T, B, obs, act, stat, H, dz = [int(v) for v in g["meta"]]
    enc = model.EncoderLSTMReal(obs + act + stat + 1, H, dz, output_all=True, reverse=reverse, device=device)
    enc.load_state_dict(_state(g, "enc_sd_"), strict=True)
    return enc


def close(got, want, tol=TOL_OUT):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= tol * (1 + np.abs(want).max()), err


def check_grads(g, module, prefix, tol=TOL_G):
    for n, p in module.named_parameters():
        w = g[prefix + n.replace(".", "__")]
        assert p.grad is not None, n
        err = np.linalg.norm((p.grad.detach().cpu().numpy() - w).ravel()) / np.linalg.norm(w.ravel())
        assert err <= tol, (n, err)


def check_baseline(g, device):
    base, data = load_baseline(g, device), load_data(g, device)
    a_in = torch.cat([data["actions"], data["statics"]], dim=-1)
    close(base(data["measurements"], a_in, data["masks"]), g["base_forward"])
    loss = base.loss(data)
    loss.backward()
    want = float(g["base_loss"])
    assert abs(loss.item() - want) <= TOL_LOSS * abs(want), (loss.item(), want)
    check_grads(g, base, "base_g_")


def check_encoder(g, reverse, device):
    enc, data = load_encoder(g, reverse, device), load_data(g, device)
    a_in = torch.cat([data["actions"], data["statics"]], dim=-1)
    mu, lv = enc(data["measurements"], a_in, data["masks"])
    r = "enc_r%d_" % int(reverse)
    close(mu, g[r + "mu"])
    close(lv, g[r + "log_var"])
    ((mu * torch.from_numpy(g["enc_cot_mu"]).to(device)).sum() + (lv * torch.from_numpy(g["enc_cot_lv"]).to(device)).sum()).backward()
    check_grads(g, enc, r + "g_")


def test_the_fixture_holds_arrays_only(g17):
    assert [int(v) for v in g17["meta"]] == [7, 5, 24, 1, 11, 44, 20]
    assert all(g17[k].dtype.kind in "fi" for k in g17.files)
    assert float(np.abs(g17["enc_r0_mu"] - g17["enc_r1_mu"]).max()) > 1e-3   # the two directions differ


def test_baseline_matches_the_reference_on_the_cpu(g17):
    check_baseline(g17, torch.device("cpu"))


@pytest.mark.parametrize("reverse", [False, True])
def test_encoder_output_all_matches_the_reference_on_the_cpu(g17, reverse):
    check_encoder(g17, reverse, torch.device("cpu"))


def test_output_all_false_is_the_last_row_of_output_all(g17):
    cpu = torch.device("cpu")
    data = load_data(g17, cpu)
    a_in = torch.cat([data["actions"], data["statics"]], dim=-1)
    for reverse in (False, True):
        every = load_encoder(g17, reverse, cpu)
        last = model.EncoderLSTMReal(every.input_dim, every.hidden_dim, every.output_dim, output_all=False, reverse=reverse, device=cpu)
        last.load_state_dict(every.state_dict())
        mu, lv = every(data["measurements"], a_in, data["masks"])
        mu1, lv1 = last(data["measurements"], a_in, data["masks"])
        assert mu.shape == (7, 5, 20) and mu1.shape == (5, 20)
        assert torch.allclose(mu[-1], mu1, atol=1e-6) and torch.allclose(lv[-1], lv1, atol=1e-6)


def test_state_dict_keys_and_shapes_are_the_reference_s(g17):
    torch.manual_seed(0)
    base = model.LSTMBaseline(36, 44, 24, device=torch.device("cpu"))
    sd = base.state_dict()
    assert list(sd) == BASE_KEYS == [k[len("base_sd_"):].replace("__", ".") for k in g17.files if k.startswith("base_sd_")]
    for k, v in sd.items():
        assert tuple(v.shape) == g17["base_sd_" + k.replace(".", "__")].shape, k
    assert [n for n, _ in base.named_parameters()] == BASE_KEYS   # creation order: lstm, then out
    assert base.model_name == "LSTMBaseline" and base.hidden_dim == 44 and base.output_dim == 24 and base.normalize is True
    assert isinstance(base.out[1], torch.nn.ELU) and base.out[0].out_features == 45


def test_save_writes_the_reference_s_keys_and_loads_back(g17, tmp_path):
    cpu = torch.device("cpu")
    base = load_baseline(g17, cpu)
    base.save(str(tmp_path) + os.sep, 12, 3.5)
    ck = torch.load(str(tmp_path / "LSTMBaseline"), map_location="cpu")
    assert sorted(ck) == ["best_loss", "itr", "state_dict"] and ck["itr"] == 12 and ck["best_loss"] == 3.5
    other = model.LSTMBaseline(36, 44, 24, device=cpu)
    other.load_state_dict(ck["state_dict"], strict=True)
    for k, v in base.state_dict().items():
        assert torch.equal(v, other.state_dict()[k]), k


def test_batch_of_one_is_refused_like_the_encoder_s():
    base = model.LSTMBaseline(4, 8, 3, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="batch size 1"):
        base(torch.zeros(5, 1, 3), torch.zeros(5, 1, 1), torch.ones(5, 1, 3))
