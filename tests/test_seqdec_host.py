"""CPU checks of the real-data recurrent baselines (model.GRUODECell, model.DecoderRealBenchmark): seeded construction and
the cell against golden G9 (recorded from the reference), the eager restatement of tests/seqdec_eager.py against G9 (it
is the CPU reference of tests/test_hip_seqdec.py), the CPU refusal, and the C layout of hode_seqdec_desc."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import seqdec_eager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hode.h")
OBS, ACT, STAT, HIDDEN = 24, 1, 11, 43


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(os.path.join(golden_dir, "g9_seqdec.npz"), allow_pickle=False)


def _cases(g):
    return range(int(g["n_cases"]))


def _build(g, ci):
    import model
    pre = "c%d_" % ci
    D, t0, B, TA, obs, seed = (int(v) for v in g[pre + "meta"])
    kind = str(g[pre + "kind"])
    torch.manual_seed(seed)
    # the exact call of run_real.py:68-70 (positional arguments, device from get_device())
    dec = model.DecoderRealBenchmark(obs, D, ACT, STAT, HIDDEN, TA, 1, ode_type=kind, t0=t0)
    return dec, pre


def test_seeded_construction_matches_the_reference(g9):
    for ci in _cases(g9):
        dec, pre = _build(g9, ci)
        sd = dec.state_dict()
        assert list(sd.keys()) == [str(k) for k in g9[pre + "sd_keys"]]
        for k, v in sd.items():
            np.testing.assert_array_equal(v.cpu().numpy(), g9[pre + "sd_" + k.replace(".", "__")], err_msg=k)
        assert dec.model_name == str(g9[pre + "model_name"])
        np.testing.assert_array_equal(dec.t.cpu().numpy(), g9[pre + "t"])
        assert dec.method == "dopri5" and dec.step_size is None and dec.hidden_dim == HIDDEN


def test_gruode_cell_matches_the_reference(g9):
    import model
    for ci in _cases(g9):
        pre = "c%d_" % ci
        if str(g9[pre + "kind"]) != "gruode":
            continue
        D = int(g9[pre + "meta"][0])
        cell = model.GRUODECell(D)
        cell.lin_hz.weight.data.copy_(torch.from_numpy(g9[pre + "sd_rnn__lin_hz__weight"]))
        cell.lin_hn.weight.data.copy_(torch.from_numpy(g9[pre + "sd_rnn__lin_hn__weight"]))
        h = torch.from_numpy(g9[pre + "cell_h"])
        dh, (h_out, c_out) = cell(torch.from_numpy(g9[pre + "cell_a"]), (h, h))
        np.testing.assert_allclose(dh.detach().numpy(), g9[pre + "cell_dh"], rtol=1e-6, atol=1e-7)
        assert h_out is h and c_out == 0


def test_eager_restatement_reproduces_the_reference(g9):
    """Outputs and every gradient of sum(x_hat * cot) from the test-side restatement equal the reference's."""
    for ci in _cases(g9):
        dec, pre = _build(g9, ci)
        dec = dec.cpu()
        init = torch.from_numpy(g9[pre + "init"]).requires_grad_(True)
        a = torch.from_numpy(g9[pre + "a"])
        x_hat, h = seqdec_eager.decoder_forward(dec, init, a)
        np.testing.assert_allclose(h.detach().numpy(), g9[pre + "h"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(x_hat.detach().numpy(), g9[pre + "x_hat"], rtol=1e-5, atol=1e-6)
        assert x_hat.shape[0] == dec.t.numel()  # no row dropped
        (x_hat * torch.from_numpy(g9[pre + "cot"])).sum().backward()
        np.testing.assert_allclose(init.grad.numpy(), g9[pre + "g_init"], rtol=1e-4, atol=1e-6)
        for n, p in dec.named_parameters():
            np.testing.assert_allclose(p.grad.numpy(), g9[pre + "g_" + n.replace(".", "__")], rtol=1e-4, atol=1e-6, err_msg=n)


def test_cpu_tensors_raise_config_error(g9):
    import hode
    import model
    for kind in ("tlstm", "gruode"):
        dec = model.DecoderRealBenchmark(OBS, 20, ACT, STAT, HIDDEN, 30, 1, ode_type=kind, t0=8, device=torch.device("cpu"))
        with pytest.raises(hode.HodeConfigError, match="no CPU fallback"):
            dec(torch.zeros(3, 20), torch.zeros(30, 3, 1), torch.zeros(30, 3, STAT))
        with pytest.raises(hode.HodeConfigError, match="no CPU fallback"):
            dec.latent(torch.zeros(3, 20), torch.zeros(30, 3, 1), None)


def test_unknown_ode_type_is_refused():
    import hode
    import model
    with pytest.raises(hode.HodeConfigError, match="tlstm"):
        model.DecoderRealBenchmark(OBS, 20, ACT, STAT, HIDDEN, 30, 1, ode_type="neural", device=torch.device("cpu"))


def test_seqdec_desc_layout_matches_the_c_header(tmp_path):
    from hode import _lib as L
    fields = [f[0] for f in L.SeqdecDesc._fields_]
    src = tmp_path / "sd.c"
    body = " ".join('printf("%%zu ", offsetof(hode_seqdec_desc, %s));' % f for f in fields)
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu ", sizeof(hode_seqdec_desc)); %s '
                   'printf("%%d %%d %%d\\n", HODE_SEQDEC_TLSTM, HODE_SEQDEC_GRUODE, HODE_SEQDEC_MAX_LATENT); return 0;}\n'
                   % (HEADER, body))
    exe = tmp_path / "sd"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(L.SeqdecDesc)
    assert vals[1:1 + len(fields)] == [getattr(L.SeqdecDesc, f).offset for f in fields]
    assert vals[1 + len(fields):] == [L.SEQDEC_TLSTM, L.SEQDEC_GRUODE, L.SEQDEC_MAX_LATENT]


def test_seqdec_argument_errors_do_not_launch():
    import hode
    from hode import _lib as L
    lib = hode.lib()
    assert lib.hode_seqdec_fwd(None, None) == -1
    d = L.SeqdecDesc()
    d.struct_size = ctypes.sizeof(L.SeqdecDesc)
    d.kind, d.n_steps, d.n_action_times, d.batch, d.latent_dim, d.action_dim = L.SEQDEC_TLSTM, 4, 4, 5, 30, 1
    assert lib.hode_seqdec_fwd(d, None) == -3 and b"1..29" in lib.hode_last_error_string()
    assert lib.hode_seqdec_workspace_bytes(d) == 0
    d.latent_dim, d.action_dim = 20, 2
    assert lib.hode_seqdec_fwd(d, None) == -3
    d.action_dim = 1
    assert lib.hode_seqdec_fwd(d, None) == -1  # pointers missing
    assert lib.hode_seqdec_workspace_bytes(d) > 0
    d.struct_size = 8
    assert lib.hode_seqdec_bwd(d, None) == -2
