"""CPU-only checks of the C-ABI boundary: the library loads, exports every symbol include/hode.h declares, the ctypes
mirrors have the C struct sizes, and argument errors are reported (no kernel is launched without a GPU)."""
import os
import subprocess
import sys

import pytest

import abi_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tuning variables the library and its wrappers once read from the environment, each at the value that flipped a
# decision: kernel variants are selected through descriptor fields and keyword arguments, and these must change nothing
STALE_ENV = {"HODE_PPW": "1", "HODE_RK_LAYOUT": "q", "HODE_NEURAL_LAYOUT": "t", "HODE_REAL_LAYOUT": "t", "HODE_LSTM_NT": "1",
             "HODE_READOUT_VALU": "1", "HODE_LSTM_GEMM_MN": "1", "HODE_LSTM_SERIAL_FILL": "1"}


@pytest.fixture(scope="module")
def lib():
    from hode import _lib as L
    return abi_checks.built(L.LIBRARY)


def test_header_functions_are_exported_and_bound(lib):
    from hode import _lib as L
    declared = abi_checks.declared_functions("hode.h", "hode_")
    assert {"hode_rk_fwd", "hode_rk_bwd", "hode_dopri5_fwd", "hode_dopri5_bwd", "hode_lstm_fwd", "hode_lstm_bwd",
            "hode_version", "hode_last_error_string", "hode_workspace_bytes"} <= set(declared)
    bound = {name for name, _, _ in L.EXPORTS}
    assert set(declared) == bound, (set(declared) ^ bound)
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.hode_version() == L.HODE_ABI_VERSION


def test_struct_sizes_match_the_c_header(tmp_path):
    from hode import _lib as L
    for c_type, mirror in (("hode_solve_desc", L.SolveDesc), ("hode_lstm_desc", L.LstmDesc), ("hode_readout_desc", L.ReadoutDesc),
                           ("hode_crps_desc", L.CrpsDesc), ("hode_mckl_desc", L.McKlDesc), ("hode_readout_mlp_desc", L.ReadoutMlpDesc),
                           ("hode_dopri5_init_record", L.Dopri5InitRecord), ("hode_seqdec_desc", L.SeqdecDesc)):
        abi_checks.assert_c_layout("hode.h", c_type, mirror, tmp_path)


def test_argument_errors_do_not_launch(lib):
    from hode import _lib as L
    assert lib.hode_rk_fwd(None, None) == -1 and b"NULL" in lib.hode_last_error_string()
    d = L.new_solve_desc()
    d.struct_size = 8
    assert lib.hode_rk_fwd(d, None) == -2 and b"struct_size" in lib.hode_last_error_string()
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.n_dose = 0, 2, 4, 12, 5, 1
    assert lib.hode_rk_fwd(d, None) == -1  # required pointers missing
    d.rhs_kind = 7
    assert lib.hode_rk_fwd(d, None) == -3
    d.rhs_kind, d.batch = 0, 0
    assert lib.hode_rk_fwd(d, None) == -2


def test_workspace_query(lib):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.batch, d.latent_dim, d.n_times = 10000, 12, 100
    P = 8 * 12 + 8 + 15
    assert lib.hode_workspace_bytes(d, L.WS_RK_FWD) == 0
    d.lanes_per_patient = 4  # quad layout: one partial row [w | b | theta] per wave
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    assert n % (P * 4) == 0 and n // (P * 4) >= (10000 + 15) // 16
    d.lanes_per_patient = 0  # default at D = 12: split layout, 3 learned-wave rows + one theta row per 48 patients
    nblk = (10000 + 47) // 48
    n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    assert n % 256 == 0 and n >= nblk * (3 * (8 * 12 + 8) + 15) * 4
    # HODE_FLAG_TAPE: forward and backward share one buffer = partials + 16 B per patient, interval and inner stage
    d.flags, d.method = L.FLAG_TAPE, L.METHODS["rk4"]
    nt = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    # expert stage states (3 x 16 B) + the learned block's last two stage derivatives (2 x 8 floats) per patient and interval
    assert nt == n + 99 * 3 * 10000 * 16 + 99 * 10000 * 8 * 2 * 4 and lib.hode_workspace_bytes(d, L.WS_RK_FWD) == nt
    d.method = L.METHODS["midpoint"]
    assert lib.hode_workspace_bytes(d, L.WS_RK_FWD) == n + 99 * 1 * 10000 * 16
    d.method = L.METHODS["euler"]  # single stage: nothing to tape
    assert lib.hode_workspace_bytes(d, L.WS_RK_FWD) == n
    d.lanes_per_patient = 4  # layouts without a tape ignore the flag
    assert lib.hode_workspace_bytes(d, L.WS_RK_FWD) == 0
    d.flags, d.lanes_per_patient = 0, 0
    d.latent_dim = 20  # no split layout for D = 20: quad
    n20 = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    assert n20 % ((16 * 20 + 16 + 15) * 4) == 0


def test_adaptive_workspace_layouts_are_the_recorded_ones(lib):
    """Totals and tape offsets of the dopri5 workspace, Roche at D 4 / 12 and NeuralODE at D 4 / 14, to the byte."""
    import adaptive_layout_table
    adaptive_layout_table.assert_layouts(lib.hode_workspace_bytes, lib.hode_dopri5_tape_offsets,
                                         {("ROCHE", 4), ("ROCHE", 12), ("NEURAL", 4), ("NEURAL", 14)})


def _variant_sizes(lib, forced):
    """Workspace sizes of five calls whose kernel variant has a switch; `forced` selects the non-default variant through
    the descriptor field (quad Roche layout, lane-per-patient neural / real kernels, NT = 1, the lane readout kernel)."""
    import ctypes as C
    from hode import _lib as L
    buf = (C.c_float * 4)()
    out = {}
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times = L.RHS_ROCHE, L.METHODS["rk4"], 10000, 12, 100
    d.lanes_per_patient = 4 if forced else 0
    out["roche"] = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim = L.RHS_NEURAL, L.METHODS["rk4"], 10000, 8, 100, 80
    d.grad_w1 = C.addressof(buf)  # never dereferenced: only selects the on-chip layout
    d.lanes_per_patient = 1 if forced else 0
    out["neural"] = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times = L.RHS_ROCHE_REAL, L.METHODS["midpoint"], 10000, 20, 100
    d.hidden_dim, d.n_action_times = 17, 100
    d.grad_w1 = C.addressof(buf)
    d.lanes_per_patient = 1 if forced else 0
    out["real"] = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    d = L.new_lstm_desc()
    d.seq_len, d.batch, d.input_dim, d.hidden_dim, d.obs_dim, d.save_tape = 3, 4097, 21, 40, 20, 1
    d.patient_tiles = 1 if forced else 0
    out["lstm"] = lib.hode_lstm_workspace_bytes(d)
    d = L.ReadoutDesc()
    d.struct_size = C.sizeof(L.ReadoutDesc)
    d.latent_dim, d.obs_dim, d.rows = 12, 52, 1000
    d.variant = L.READOUT_VARIANT_VALU if forced else 0
    out["readout"] = lib.hode_readout_workspace_bytes(d)
    assert all(v > 0 for v in out.values()), out
    return out


def test_variants_follow_the_descriptor_not_the_environment(lib, monkeypatch):
    """No launch: with every former tuning variable set to the value that used to flip a decision, the workspace sizes
    are exactly those of a clean environment; the descriptor fields are what selects a variant (each forced size differs)."""
    for name in STALE_ENV:
        monkeypatch.delenv(name, raising=False)
    clean, forced = _variant_sizes(lib, False), _variant_sizes(lib, True)
    for name, value in STALE_ENV.items():
        monkeypatch.setenv(name, value)
    assert _variant_sizes(lib, False) == clean
    assert _variant_sizes(lib, True) == forced
    for k in clean:
        assert forced[k] != clean[k], k


def test_tape_flag_needs_its_workspace(lib):
    """hode_rk_fwd with HODE_FLAG_TAPE and no (or a short) workspace is an argument error, not a launch."""
    import ctypes as C
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.n_dose = 0, L.METHODS["rk4"], 96, 12, 5, 1
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)  # never dereferenced: the call must fail before any launch
    d.t = d.y0 = d.dosage = d.dose_times = d.theta = d.w1 = d.b1 = d.h = ptr
    d.flags = L.FLAG_TAPE
    assert lib.hode_rk_fwd(d, None) == -4 and b"workspace" in lib.hode_last_error_string()
    d.workspace, d.workspace_bytes = ptr, 128
    assert lib.hode_rk_fwd(d, None) == -4


def test_missing_library_fails_loudly(tmp_path):
    code = ("import sys; sys.path.insert(0, %r); import os; os.environ['HODE_LIBRARY'] = %r\n"
            "import hode\n"
            "try:\n    hode.lib()\nexcept hode.HodeConfigError as e:\n    print('RAISED', 'no CPU fallback' in str(e), isinstance(e, RuntimeError))\n"
            % (os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"), str(tmp_path / "nope.so")))
    out = subprocess.check_output([sys.executable, "-c", code]).decode()
    assert "RAISED True False" in out  # a configuration error, not the RuntimeError the training loop treats as divergence


def test_library_was_built_from_the_sources_in_the_tree():
    """build_hip.py stamps libhode.so with a digest of the sources, header and flags it was built from; a library left
    over from other sources (an experiment reverted with `git checkout`, a forgotten rebuild) must not pass as current."""
    import build_hip
    assert os.path.exists(build_hip.OUT), "libhode.so missing: run `python build_hip.py`"
    abi_checks.assert_digest_current("libhode.so")
