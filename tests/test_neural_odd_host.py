"""CPU checks of the NeuralODE at odd latent sizes (no GPU): libhode_neural_odd.so's C ABI and refusals, its row
of the build table, the kernels its objects contain against the GPU case table (tests/neural_odd_cases.py), the function
that chooses the library per latent size, the error texts for sizes nobody serves, and the D = 15 fixture (G15,
tests/golden/make_golden_neural_odd.py) against the CPU oracle at the bounds tests/test_oracle_golden.py holds G2 / G5 to."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import neural_odd_cases as cases
from oracle import rhs as orhs
from oracle import vi as ovi
from oracle.encoder import EncoderLSTMOracle

ROOT = build_hip.ROOT
LIB = "libhode_neural_odd.so"
FUNCTIONS = {"hode_neural_odd_" + n for n in ("version", "last_error_string", "workspace_bytes", "rk_fwd", "rk_bwd", "dopri5_fwd",
                                               "dopri5_bwd", "dopri5_tape_offsets")}
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from hode import _neural_odd_lib as NL
    return abi_checks.built(NL.LIBRARY)


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
def test_header_functions_are_exported_and_bound(lib):
    from hode import _neural_odd_lib as NL
    declared = abi_checks.declared_functions("hode_neural_odd.h", "hode_neural_odd_")
    assert declared == {name for name, _, _ in NL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    assert "#define HODE_NEURAL_ODD_ABI_VERSION %d\n" % NL.HODE_NEURAL_ODD_ABI_VERSION in abi_checks.header_text("hode_neural_odd.h")
    assert lib.hode_neural_odd_version() == NL.HODE_NEURAL_ODD_ABI_VERSION
    # the descriptor is hode.h's: included, not restated
    src = abi_checks.header_text("hode_neural_odd.h")
    assert '#include "hode.h"' in src and "struct" not in src
    assert NL.DIMS == build_hip.NEURAL_ODD_DIMS == cases.DIMS


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_neural_odd.h" and "include/hode.h" in build_hip.digest_files(LIB)
    assert row.src_dir == build_hip.PKG + "/csrc/neural_odd"
    assert sorted(n for n, _, _ in row.units()) == sorted(["hode_neural_odd"] + ["hode_neural_odd_d%d" % D for D in cases.DIMS])


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    """The kernel symbols of csrc/neural_odd/build/*.o are sizes x the thirteen instantiations, and the GPU case table
    reaches every one of them: an instantiation added to the library without a case fails here."""
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        build_hip.build(verbose=False)
        objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    want = cases.expected_kernels()
    assert len(want) == 13 * len(cases.DIMS)
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    reached = cases.kernels_reached()
    assert compiled <= reached, sorted(compiled - reached)
    assert reached <= compiled, sorted(reached - compiled)


# --------------------------------------------------------------------------------------------- 2. who serves which size
def test_library_selection(lib):
    import hode
    from hode import _neural_odd_lib as NL, adaptive
    for D in adaptive.NEURAL_DIMS + (3, 16, 17, 20):
        assert NL.neural_solver_library(D) is hode.lib()
    assert adaptive.NEURAL_DIMS == (4, 6, 8, 10, 12, 14) and adaptive.NEURAL_ODD_DIMS == NL.DIMS == (5, 7, 9, 11, 13, 15)
    for D in NL.DIMS:
        side = NL.neural_solver_library(D)
        assert side is NL.neural_solver_library(15) and side is not hode.lib()
        for name, restype, _ in NL.SOLVER_ENTRIES:
            assert callable(getattr(side, "hode_" + name))
        assert side.hode_workspace_bytes is lib.hode_neural_odd_workspace_bytes


def test_a_missing_side_library_raises_at_the_first_odd_call_only(tmp_path, monkeypatch):
    import hode
    from hode import HodeConfigError, _neural_odd_lib as NL
    monkeypatch.setattr(NL.LIBRARY, "handle", None)
    monkeypatch.setattr(NL.LIBRARY, "directory", str(tmp_path))
    assert NL.neural_solver_library(14) is hode.lib()
    with pytest.raises(HodeConfigError, match="libhode_neural_odd.so not found"):
        NL.neural_solver_library(15)


def _desc(D, **over):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim, d.max_steps = L.RHS_NEURAL, L.METHODS["rk4"], 17, D, 6, 10 * D, 64
    d.rtol, d.atol = 1e-6, 1e-8
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_the_side_library_reports_its_own_error_text(lib):
    """A failing entry raises through the wrapper with libhode_neural_odd.so's message; libhode.so's text stays untouched."""
    from hode import HodeConfigError, _lib as L, _neural_odd_lib as NL
    side = NL.neural_solver_library(15)
    with pytest.raises(HodeConfigError, match=r"hode_neural_odd_rk_fwd failed \(code -3\): neural odd: lanes_per_patient 1 "):
        side.hode_rk_fwd(_desc(15, lanes_per_patient=1), None)
    assert side.hode_workspace_bytes(_desc(15, lanes_per_patient=1), L.WS_RK_BWD) == 0


def test_argument_errors_do_not_launch(lib):
    from hode import _lib as L
    err = lib.hode_neural_odd_last_error_string
    E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
    fwd, bwd, dfwd, dbwd = lib.hode_neural_odd_rk_fwd, lib.hode_neural_odd_rk_bwd, lib.hode_neural_odd_dopri5_fwd, lib.hode_neural_odd_dopri5_bwd
    for fn in (fwd, bwd, dfwd, dbwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(15, struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        assert fn(_desc(15, rhs_kind=L.RHS_ROCHE), None) == E_UNSUPPORTED and b"rhs_kind 0" in err()
        for D in (3, 4, 6, 14, 16, 17):
            assert fn(_desc(D), None) == E_UNSUPPORTED and b"latent_dim %d " % D in err() and b"5, 7, 9, 11, 13, 15" in err()
        assert fn(_desc(15, hidden_dim=149), None) == E_UNSUPPORTED and b"hidden_dim 149" in err()
        assert fn(_desc(15, lanes_per_patient=1), None) == E_UNSUPPORTED and b"lanes_per_patient 1" in err()
        assert fn(_desc(15), None) == E_NULL                       # a shape of the domain, pointers missing
    assert fwd(_desc(15, method=3), None) == E_UNSUPPORTED and b"method 3" in err()
    assert fwd(_desc(15, flags=L.FLAG_TAPE), None) == E_UNSUPPORTED and b"flags 4" in err()
    assert dfwd(_desc(15, flags=L.FLAG_DETACH_FIRST_STEP), None) == E_UNSUPPORTED and b"flags 8" in err()
    assert dbwd(_desc(15, flags=L.FLAG_NO_TAPE), None) == E_UNSUPPORTED and b"NO_TAPE" in err()
    assert dfwd(_desc(15, max_steps=0), None) == E_SIZE and b"max_steps=0" in err()
    ptrs = {k: 64 for k in ("t", "y0", "dosage", "h", "w1", "b1", "w2", "b2", "grad_h", "grad_y0")}
    assert bwd(_desc(15, **ptrs), None) == E_UNSUPPORTED and b"grad_w1 is NULL" in err() and b"operand-tape" in err()
    assert dbwd(_desc(15, **ptrs), None) == E_UNSUPPORTED and b"grad_w1 is NULL" in err()
    ptrs.update(grad_w1=64)
    assert bwd(_desc(15, **ptrs), None) == E_NULL and b"grad_b1" in err()
    ptrs.update(grad_b1=64, grad_w2=64, grad_b2=64)
    assert bwd(_desc(15, **ptrs), None) == E_WORKSPACE and b"workspace 0 B" in err()
    off = (ctypes.c_size_t * 5)()
    assert lib.hode_neural_odd_dopri5_tape_offsets(_desc(14), off) == E_UNSUPPORTED and b"latent_dim 14 " in err()
    assert lib.hode_neural_odd_dopri5_tape_offsets(_desc(15), None) == E_NULL


def test_workspace_sizes_follow_the_partial_block(lib):
    """Fixed-grid backward: one block of 2 HT 256 + 16 floats per 16-patient wave, plus 16 HT floats of db1 at D = 15 only
    (the size without room for the ones row); nothing for the forward or without grad_w1.  dopri5: the tape offsets are
    ordered and inside the workspace."""
    from hode import _lib as L
    buf = (ctypes.c_float * 4)()
    for D in cases.DIMS:
        HT = (10 * D + 15) // 16
        NP = 2 * HT * 256 + 16 + (16 * HT if D == 15 else 0)
        for B in (1, 16, 17, 65):
            d = _desc(D, batch=B)
            assert lib.hode_neural_odd_workspace_bytes(d, L.WS_RK_FWD) == 0 and lib.hode_neural_odd_workspace_bytes(d, L.WS_RK_BWD) == 0
            d.grad_w1 = ctypes.addressof(buf)  # never dereferenced: only selects the layout
            assert lib.hode_neural_odd_workspace_bytes(d, L.WS_RK_BWD) == ((B + 15) // 16) * NP * 4, (D, B)
            total = lib.hode_neural_odd_workspace_bytes(d, L.WS_DOPRI5_FWD)
            assert total == lib.hode_neural_odd_workspace_bytes(d, L.WS_DOPRI5_BWD) > 0
            off = (ctypes.c_size_t * 5)()
            assert lib.hode_neural_odd_dopri5_tape_offsets(d, off) == 0
            assert list(off) == sorted(off) and off[4] + 65 * B * D * 4 + ((B + 15) // 16) * NP * 4 <= total
    assert lib.hode_neural_odd_workspace_bytes(_desc(14), L.WS_DOPRI5_FWD) == 0


def test_adaptive_workspace_layouts_are_the_recorded_ones(lib):
    """Totals and tape offsets of the dopri5 workspace at D 5 and 15, to the byte (the table libhode.so's sizes are in)."""
    import adaptive_layout_table
    adaptive_layout_table.assert_layouts(lib.hode_neural_odd_workspace_bytes, lib.hode_neural_odd_dopri5_tape_offsets,
                                         {("NEURAL", 5), ("NEURAL", 15)})


# ----------------------------------------------------------------------------------------- 3. sizes nobody serves
@pytest.mark.parametrize("D", [16, 3])
def test_error_text_for_a_size_without_a_kernel(D):
    """The mirror's NeuralODE with dopri5 refuses before any library call, so the text is checked without a GPU."""
    import hode
    import model
    ode = model.NeuralODE(D, 1, 1.0, 0.125, device=CPU)
    ode.set_action(torch.zeros(9, 2, 1))
    with pytest.raises(hode.HodeConfigError) as e:
        ode.hode_solve(torch.zeros(2, D), torch.arange(9.0) * 0.125, 1e-7, 1e-8, "dopri5", {})
    text = str(e.value)
    assert "4, 6, 8, 10, 12, 14" in text and "5, 7, 9, 11, 13, 15" in text and "(got %d)" % D in text


# ------------------------------------------------------------------------------------------ 4. fixture vs CPU oracle
def _load(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_neural_odd.npz"), allow_pickle=False)


def _load_sd(module, g, prefix):
    module.load_state_dict({k[len(prefix):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)},
                           strict=True)


def test_g15_neural_rhs_at_15(golden_dir):
    """The reference's NeuralODE(15) rhs and VJPs against oracle.rhs.NeuralRHS, at G2's bounds; the dose fires at t = 0,
    2 step and 5 step (the last also a midpoint stage time) and not 1e-3 later."""
    g = _load(golden_dir)
    D, T, B = [int(v) for v in g["c0_meta"]]
    assert D == 15
    f = orhs.NeuralRHS(D, float(g["c0_step"]))
    _load_sd(f, g, "c0_sd_")
    f.set_action(torch.from_numpy(g["c0_action"]))
    y, cot = torch.from_numpy(g["c0_y"]), torch.from_numpy(g["c0_cot"])
    fs = g["c0_f"]
    assert np.abs(fs[1] - fs[2]).max() > 1e-3   # 2 step is a dose time of patients 0 and 1, 2 step + 1e-3 is not
    for ti, t in enumerate(g["c0_t"]):
        yy = y.clone().requires_grad_(True)
        f.zero_grad()
        out = f(torch.tensor(float(t), dtype=torch.float32), yy)
        np.testing.assert_allclose(out.detach().numpy(), fs[ti], rtol=1e-6, atol=1e-7)
        (out * cot).sum().backward()
        np.testing.assert_allclose(yy.grad.numpy(), g["c0_gy"][ti], rtol=1e-5, atol=1e-6)
        for n, p in f.named_parameters():
            want = g["c0_g_" + n.replace(".", "__")][ti]
            got = p.grad.numpy() if p.grad is not None else np.zeros_like(want)
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=n)


def test_g15_vi_loss_at_15(golden_dir):
    """VariationalInference.loss as run_simulation --method=neural --encoder_output_dim=15 builds it (dopri5, prior None,
    encoder without normalisation) against oracle.vi at G5's bounds for dopri5."""
    g = _load(golden_dir)
    obs, D, T, B, seed = [int(v) for v in g["vi_meta"]]
    step = float(g["vi_step"])
    assert (D, str(g["vi_method"]), str(g["vi_mode"]), str(g["vi_model_name"])) == (15, "dopri5", "kl_normal", "NeuralODEDecoder")
    enc = EncoderLSTMOracle(obs + 1, obs * 2, D, normalize=False)
    dec = ovi.DecoderOracle(obs, D, (T - 1) * step, step, roche=False, method="dopri5")
    _load_sd(enc, g, "vi_enc_")
    _load_sd(dec, g, "vi_dec_")
    data = {k2: torch.from_numpy(g["vi_" + k]) for k, k2 in (("x", "measurements"), ("a", "actions"), ("mask", "masks"))}
    torch.manual_seed(seed)
    loss = ovi.vi_loss(enc, dec, data, elbo=True, exponential_prior=False)
    np.testing.assert_allclose(loss.item(), float(g["vi_loss"]), rtol=2e-5)
    loss.backward()
    for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
        for n, p in mod.named_parameters():
            want = g["vi_" + tag + n.replace(".", "__")]
            got = p.grad.numpy() if p.grad is not None else np.zeros_like(want)
            np.testing.assert_allclose(got, want, rtol=5e-3, atol=2e-3 * (1 + np.abs(want).max()), err_msg=n)
    assert np.abs(g["vi_gdec_ode__ml_net__0__bias"]).max() > 0   # b1's gradient, the quantity the D = 15 path exists for
