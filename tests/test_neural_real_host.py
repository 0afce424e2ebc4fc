"""CPU checks of the real-data neural ODE baselines (model.NeuralODEReal / NeuralODEReal2nd): seeded construction, the
eager rhs and dose_at_time against golden G10 (recorded from the reference), hode.neural_real.stage_rows against the rows
the reference's rhs used, the eager restatement of tests/neural_real_eager.py against G10 (it is the CPU reference of
tests/test_hip_neural_real.py), the refusals, and the new rhs kinds of the C ABI."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import neural_real_eager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hode.h")
OBS, ACT, STAT = 24, 1, 11
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_neural_real.npz"), allow_pickle=False)


def _case(g, ci):
    pre = "c%d_" % ci
    D, H, div, t0, TA, TMAX, B, obs, seed = (int(v) for v in g[pre + "meta"])
    return pre, str(g[pre + "kind"]), str(g[pre + "method"]), D, H, div, t0, TA, TMAX, seed


def _sd(g, pre):
    return {str(k): torch.from_numpy(g[pre + "sd_" + str(k).replace(".", "__")]) for k in g[pre + "sd_keys"]}


def _ode_cls(kind):
    import model
    return model.NeuralODEReal if kind == "neural" else model.NeuralODEReal2nd


def test_seeded_construction_matches_the_reference(g10):
    """Readout first, then the rhs, from the same seed: the reference DecoderReal's parameter creation order."""
    for ci in range(int(g10["n_cases"])):
        pre, kind, method, D, H, div, t0, TA, TMAX, seed = _case(g10, ci)
        torch.manual_seed(seed)
        of = nn.Sequential(nn.Linear(D, D + 1), nn.ELU(), nn.Linear(D + 1, OBS))
        ode = _ode_cls(kind)(D, ACT, STAT, H, TMAX, 1, device=CPU)
        sd = {"output_function." + k: v for k, v in of.state_dict().items()}
        sd.update({"ode." + k: v for k, v in ode.state_dict().items()})
        assert list(sd) == [str(k) for k in g10[pre + "sd_keys"]]
        for k, v in sd.items():
            np.testing.assert_array_equal(v.numpy(), g10[pre + "sd_" + k.replace(".", "__")], err_msg=k)
        assert ode.ml_net[2].weight.shape == ((D if kind == "neural" else D // 2), H)
        assert ode.action is None and ode.static is None


def test_eager_rhs_and_dose_match_the_reference(g10):
    for ci in range(int(g10["n_cases"])):
        pre, kind, method, D, H, div, t0, TA, TMAX, seed = _case(g10, ci)
        ode = _ode_cls(kind)(D, ACT, STAT, H, TMAX, 1, device=CPU)
        sd = _sd(g10, pre)
        ode.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("ode.")})
        ode.set_action_static(torch.from_numpy(g10[pre + "a"]), torch.from_numpy(g10[pre + "s"]))
        with torch.no_grad():
            f = ode(torch.from_numpy(g10[pre + "rhs_t"]), torch.from_numpy(g10[pre + "rhs_y"]))
            np.testing.assert_array_equal(f.numpy(), g10[pre + "rhs_f"])
            for tv, want in zip(g10[pre + "probe_t"], g10[pre + "probe_dose"]):
                np.testing.assert_array_equal(ode.dose_at_time(torch.tensor(tv)).numpy(), want, err_msg=str(tv))
            # every stage time the reference's solve used (perturbed, fractional)
            for tv, row in zip(g10[pre + "dose_t"][:12], g10[pre + "dose_row"][:12]):
                want = np.cumsum(g10[pre + "a"], axis=0)[row] if row < TA else np.zeros_like(g10[pre + "a"][0])
                np.testing.assert_allclose(ode.dose_at_time(torch.tensor(tv)).numpy(), want, rtol=0, atol=1e-6)
        ode.set_action_static(torch.from_numpy(g10[pre + "a"]), None)  # static is stored and unused
        assert ode.static is None


def test_stage_rows_reproduce_the_reference_sequence(g10):
    from hode import neural_real, substep
    for ci in range(int(g10["n_cases"])):
        pre, kind, method, D, H, div, t0, TA, TMAX, seed = _case(g10, ci)
        t = torch.from_numpy(g10[pre + "t"])
        grid = substep.fixed_grid(t, 1.0 / div)
        st = neural_real.stage_times(grid, method, True)
        rows = neural_real.stage_rows(grid, method, True, TA)
        np.testing.assert_array_equal(st.reshape(-1).numpy(), g10[pre + "dose_t"])
        np.testing.assert_array_equal(rows.reshape(-1).numpy(), g10[pre + "dose_row"])
        idx = neural_real.table_index(rows, TA)
        assert int(idx.min()) >= 0 and int(idx.max()) <= TA
        if int(rows.max()) >= TA:
            assert int(idx.max()) == TA  # the zero row
    # trunc, not floor; negative rows index from the end; rows past the action read the zero row
    grid = torch.tensor([-2.0, -1.0, 0.0, 1.0])
    rows = neural_real.stage_rows(grid, "midpoint", False, 3)
    assert rows.tolist() == [[-2, -1], [-1, 0], [0, 0]]
    assert neural_real.table_index(torch.tensor([-2, -1, 0, 2, 3, 7]), 3).tolist() == [1, 2, 0, 2, 3, 3]
    with pytest.raises(Exception):
        neural_real.stage_rows(torch.tensor([-5.0, -4.0]), "euler", False, 3)


def test_eager_restatement_matches_golden(g10):
    for ci in range(int(g10["n_cases"])):
        pre, kind, method, D, H, div, t0, TA, TMAX, seed = _case(g10, ci)
        sd = {k: v.clone().requires_grad_(True) for k, v in _sd(g10, pre).items()}
        init = torch.from_numpy(g10[pre + "init"]).requires_grad_(True)
        a = torch.from_numpy(g10[pre + "a"])
        t = torch.from_numpy(g10[pre + "t"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x_hat, h, rows = neural_real_eager.decoder(kind, sd, init, a, t, method, 1.0 / div)
        assert rows == g10[pre + "dose_row"].tolist()
        np.testing.assert_allclose(h.detach().numpy(), g10[pre + "h"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(x_hat.detach().numpy(), g10[pre + "x_hat"], rtol=1e-5, atol=1e-5)
        (x_hat * torch.from_numpy(g10[pre + "cot"])).sum().backward()
        np.testing.assert_allclose(init.grad.numpy(), g10[pre + "g_init"], rtol=1e-4, atol=1e-5)
        for k, v in sd.items():
            np.testing.assert_allclose(v.grad.numpy(), g10[pre + "g_" + k.replace(".", "__")], rtol=1e-4, atol=1e-5, err_msg=k)


def test_refusals():
    import hode
    import model
    from hode import neural_real
    for kind in ("neural", "2nd"):
        with pytest.raises(hode.HodeConfigError, match="GPU"):
            model.DecoderReal(OBS, 20 if kind == "neural" else 40, 1, STAT, 43, 40, 1, ode_type=kind, t0=24, device=CPU)
    with pytest.raises(hode.HodeConfigError, match="even"):
        model.DecoderReal(OBS, 41, 1, STAT, 43, 40, 1, ode_type="2nd", t0=24, device=CPU)
    for kind, D, H, A in (("neural", 31, 43, 1), ("neural", 0, 43, 1), ("2nd", 62, 43, 1), ("neural", 20, 65, 1),
                          ("neural", 20, 0, 1), ("neural", 20, 43, 2), ("2nd", 40, 43, 2)):
        with pytest.raises(hode.HodeConfigError):
            model.DecoderReal(OBS, D, A, STAT, H, 40, 1, ode_type=kind, t0=24, device=CPU)
        with pytest.raises(hode.HodeConfigError):
            neural_real.check_config(kind, D, H, A)
    neural_real.check_config("neural", 30, 64, 1)
    neural_real.check_config("2nd", 60, 1, 1)
    ode = model.NeuralODEReal(20, 1, STAT, 43, 40, 1, device=CPU)
    ode.set_action_static(torch.zeros(40, 3, 1), None)
    t = torch.arange(23.0, 40.0)
    with pytest.raises(hode.HodeConfigError, match="dopri5"):
        hode.odeint(ode, torch.zeros(3, 20), t, method="dopri5", options={"step_t": t, "perturb": True})
    with pytest.raises(hode.HodeConfigError):  # CPU tensors: the kernels only
        hode.odeint(ode, torch.zeros(3, 20), t, method="midpoint", options={"step_size": 1.0, "perturb": True})
    ode2 = model.NeuralODEReal2nd(7, 1, STAT, 43, 40, 1, device=CPU)
    ode2.set_action_static(torch.zeros(40, 3, 1), None)
    with pytest.raises(hode.HodeConfigError, match="even"):
        hode.odeint(ode2, torch.zeros(3, 7), t, method="rk4", options={"perturb": True})


def test_header_constants_match_lib():
    from hode import _lib as L
    src = open(HEADER).read()
    consts = dict(re.findall(r"#define (HODE_RHS_[A-Z0-9_]+) (\d+)", src))
    assert int(consts["HODE_RHS_NEURAL_REAL"]) == L.RHS_NEURAL_REAL == 4
    assert int(consts["HODE_RHS_NEURAL_REAL_2ND"]) == L.RHS_NEURAL_REAL_2ND == 5
    assert "7" not in consts.values()


@pytest.fixture(scope="module")
def lib():
    import hode
    if not os.path.exists(hode.library_path()):
        import build_hip
        build_hip.build(verbose=False)
    return hode.lib()


def test_new_kinds_reject_bad_descriptors_without_launching(lib):
    from hode import _lib as L
    for kind in (L.RHS_NEURAL_REAL, L.RHS_NEURAL_REAL_2ND):
        d = L.new_solve_desc()
        d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim = kind, L.METHODS["rk4"], 8, 20, 5, 43
        assert lib.hode_rk_fwd(d, None) == -1 and b"NULL" in lib.hode_last_error_string()
        assert lib.hode_rk_bwd(d, None) == -1
        assert lib.hode_workspace_bytes(d, L.WS_RK_FWD) == 0
        assert lib.hode_workspace_bytes(d, L.WS_RK_BWD) > 0
        d.latent_dim = 21 if kind == L.RHS_NEURAL_REAL_2ND else 31
        assert lib.hode_rk_fwd(d, None) == -3
        d.latent_dim, d.hidden_dim = 20, 65
        assert lib.hode_rk_fwd(d, None) == -3
        d.hidden_dim, d.batch = 43, 0
        assert lib.hode_rk_fwd(d, None) == -2
        d.batch, d.method = 8, 3
        assert lib.hode_rk_fwd(d, None) == -3
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)  # never dereferenced: the call must fail before any launch
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim = L.RHS_NEURAL_REAL, 0, 8, 20, 5, 43
    d.t = d.y0 = d.dosage = d.w1 = d.b1 = d.w2 = d.b2 = d.h = d.grad_h = d.grad_y0 = ptr
    assert lib.hode_rk_bwd(d, None) == -4 and b"workspace" in lib.hode_last_error_string()
