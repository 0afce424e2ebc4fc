"""CPU checks of the hybrid decoder's side library (no GPU): libhode_roche_dims.so's C ABI and refusals, its row of
the build table, the kernels its objects contain against the GPU case table (tests/roche_dims_cases.py), the function that
chooses the library per latent size, and what stays as it was: hode.roche_solve alone still refuses a size of the side
library."""
import ctypes
import glob
import os
import sys

import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import roche_dims_cases as cases

ROOT = build_hip.ROOT
LIB = "libhode_roche_dims.so"
FUNCTIONS = {"hode_roche_dims_" + n for n in ("version", "last_error_string", "workspace_bytes", "rk_fwd", "rk_bwd", "dopri5_fwd",
                                              "dopri5_bwd", "dopri5_tape_offsets")}
SIZES = b"5, 7, 9, 10, 11, 13, 14, 15, 16"
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from hode import _roche_dims_lib as RL
    return abi_checks.built(RL.LIBRARY)


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
def test_header_functions_are_exported_and_bound(lib):
    from hode import _roche_dims_lib as RL
    declared = abi_checks.declared_functions("hode_roche_dims.h", "hode_roche_dims_")
    assert declared == {name for name, _, _ in RL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_roche_dims.h")
    assert "#define HODE_ROCHE_DIMS_ABI_VERSION %d\n" % RL.HODE_ROCHE_DIMS_ABI_VERSION in src
    assert lib.hode_roche_dims_version() == RL.HODE_ROCHE_DIMS_ABI_VERSION
    assert '#include "hode.h"' in src and "struct" not in src   # the descriptor is hode.h's: included, not restated


def test_sizes_agree_everywhere():
    from hode import _roche_dims_lib as RL
    assert RL.DIMS == build_hip.ROCHE_DIMS == cases.DIMS == (5, 7, 9, 10, 11, 13, 14, 15, 16)
    assert RL.LIBHODE_RK_DIMS == build_hip.RK_DIMS and RL.LIBHODE_DP_DIMS == build_hip.DP_DIMS
    assert not set(RL.DIMS) & set(build_hip.RK_DIMS)
    internal = open(os.path.join(build_hip.CSRC, "roche_dims", "hode_roche_dims.hpp")).read()
    assert "#define HODE_ROCHE_DIMS(X) " + " ".join("X(%d)" % D for D in RL.DIMS) + "\n" in internal
    assert '#define HODE_ROCHE_DIMS_TEXT "%s"\n' % SIZES.decode() in internal


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_roche_dims.h" and "include/hode.h" in build_hip.digest_files(LIB)
    assert row.src_dir == build_hip.PKG + "/csrc/roche_dims"
    want = ["hode_roche_dims", "hode_roche_dims_dopri5"] + ["hode_roche_dims_%s_d%d" % (k, D) for D in cases.DIMS for k in ("rk", "dp")]
    assert sorted(n for n, _, _ in row.units()) == sorted(want)
    assert build_hip.RK_DIMS == (4, 6, 8, 12, 20) and build_hip.DP_DIMS == (4, 6, 8, 12)


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    """The kernel symbols of csrc/roche_dims/build/*.o are the sizes x the instantiations the case table states, and the
    table reaches every one of them with every rhs body it holds (the two persistent attempt loops of D = 16 aside, which
    no product build launches)."""
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        build_hip.build(verbose=False)
        objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    want = cases.expected_kernels()
    assert len(want) == 1 + len(cases.DIMS) * (36 + 16) + 16 + 2
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    reached = cases.kernels_reached()
    assert reached <= compiled, sorted(reached - compiled)
    assert compiled - reached == cases.UNREACHABLE, sorted(compiled - reached - cases.UNREACHABLE)
    got = cases.bodies_reached()
    missing = [(k, b) for k in sorted(compiled - cases.UNREACHABLE) for b in kv.bodies(k) if (k, b) not in got]
    assert not missing, missing[:10]


def test_the_targeted_cases_name_the_padding_sizes():
    assert {5, 15, 16} <= set(cases.TARGETED_DIMS) <= set(cases.DIMS)
    assert cases.ragged(5) and cases.ragged(15) and cases.ragged(10) and not cases.ragged(16)
    assert (1, cases.T) in cases.EDGE_SHAPES and (cases.N, 1) in cases.EDGE_SHAPES and (cases.N, 2) in cases.EDGE_SHAPES
    assert cases.N % 16 != 0 and cases.N > 64   # a ragged last wave in both layouts, more than one wave


# --------------------------------------------------------------------------------------------- 2. who serves which size
def test_library_selection(lib):
    import hode
    from hode import _roche_dims_lib as RL
    for D in build_hip.RK_DIMS + (3, 17, 18, 24):
        assert RL.roche_solver_library(D) is hode.lib()
    for D in RL.DIMS:
        side = RL.roche_solver_library(D)
        assert side is RL.roche_solver_library(16) and side is not hode.lib()
        for name, restype, _ in RL.SOLVER_ENTRIES:
            assert callable(getattr(side, "hode_" + name))
        assert side.hode_workspace_bytes is lib.hode_roche_dims_workspace_bytes


def test_a_missing_side_library_raises_at_the_first_call_that_needs_it(tmp_path, monkeypatch):
    import hode
    from hode import HodeConfigError, _roche_dims_lib as RL
    monkeypatch.setattr(RL.LIBRARY, "handle", None)
    monkeypatch.setattr(RL.LIBRARY, "directory", str(tmp_path))
    assert RL.roche_solver_library(12) is hode.lib()
    with pytest.raises(HodeConfigError, match="libhode_roche_dims.so not found"):
        RL.roche_solver_library(10)


def _desc(D, **over):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.n_dose, d.max_steps = L.RHS_ROCHE, L.METHODS["rk4"], 17, D, 6, 1, 64
    d.rtol, d.atol = 1e-6, 1e-8
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_the_side_library_reports_its_own_error_text(lib):
    from hode import HodeConfigError, _lib as L, _roche_dims_lib as RL
    side = RL.roche_solver_library(10)
    with pytest.raises(HodeConfigError, match=r"hode_roche_dims_rk_fwd failed \(code -3\): roche dims: lanes_per_patient 16 "):
        side.hode_rk_fwd(_desc(10, lanes_per_patient=16), None)
    assert side.hode_workspace_bytes(_desc(10, lanes_per_patient=16), L.WS_RK_BWD) == 0


def test_argument_errors_do_not_launch(lib):
    from hode import _lib as L
    err = lib.hode_roche_dims_last_error_string
    E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
    fwd, bwd, dfwd, dbwd = lib.hode_roche_dims_rk_fwd, lib.hode_roche_dims_rk_bwd, lib.hode_roche_dims_dopri5_fwd, lib.hode_roche_dims_dopri5_bwd
    for fn in (fwd, bwd, dfwd, dbwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(10, struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        for kind in (L.RHS_NEURAL, L.RHS_ROCHE_REAL):
            assert fn(_desc(10, rhs_kind=kind), None) == E_UNSUPPORTED and b"rhs_kind %d " % kind in err() and SIZES in err()
        for D in (3, 4, 6, 8, 12, 17, 20):   # libhode.so's own sizes included
            assert fn(_desc(D), None) == E_UNSUPPORTED and b"latent_dim %d " % D in err() and SIZES in err()
            assert b"libhode.so has 4, 6, 8, 12, 20" in err()
        for lanes in (16, 48, 2):
            assert fn(_desc(10, lanes_per_patient=lanes), None) == E_UNSUPPORTED and b"lanes_per_patient %d " % lanes in err()
            assert SIZES in err() and b"no MFMA or split layout" in err()
        assert fn(_desc(10), None) in (E_NULL, E_SIZE)              # a shape of the domain, pointers missing
    assert fwd(_desc(10, method=3), None) == E_UNSUPPORTED and b"method 3" in err()
    assert fwd(_desc(10, batch=0), None) == E_SIZE and b"batch=0" in err()
    ptrs = {k: 64 for k in ("t", "y0", "dosage", "dose_times", "theta", "h")}
    assert fwd(_desc(10, **ptrs), None) == E_NULL and b"w1 / b1" in err()
    ptrs.update(w1=64, b1=64)
    assert fwd(_desc(10, flags=L.FLAG_TAPE, **ptrs), None) == E_UNSUPPORTED and b"flags 4" in err() and b"stage tape" in err()
    assert bwd(_desc(10, **ptrs), None) == E_NULL and b"grad_h / grad_y0" in err()
    ptrs.update(grad_h=64, grad_y0=64)
    assert bwd(_desc(10, **ptrs), None) == E_WORKSPACE and b"workspace 0 B" in err()
    assert bwd(_desc(16, **dict(ptrs, y0=68)), None) == E_ALIGN and b"16-byte aligned" in err()   # rows of 16 floats: float4 access
    assert bwd(_desc(10, **dict(ptrs, y0=68)), None) == E_WORKSPACE                               # 10 floats: dword access
    assert dfwd(_desc(10, max_steps=0), None) == E_SIZE and b"max_steps=0" in err()
    assert dbwd(_desc(10, flags=L.FLAG_NO_TAPE, host_n_accepted=ctypes.pointer(ctypes.c_int32(1)), **ptrs), None) == E_UNSUPPORTED
    assert b"NO_TAPE" in err()
    off = (ctypes.c_size_t * 5)()
    assert lib.hode_roche_dims_dopri5_tape_offsets(_desc(12), off) == E_UNSUPPORTED and b"latent_dim 12 " in err()
    assert lib.hode_roche_dims_dopri5_tape_offsets(_desc(10), None) == E_NULL


def test_workspace_sizes_follow_the_layout(lib):
    """Fixed-grid backward: one row of M D + M + 15 floats per wave, with the layout's patients per wave (the whole batch
    here is far below one wave per SIMD, so a wave takes one patient); nothing for the forward.  dopri5: ordered offsets."""
    from hode import _lib as L
    ws = lib.hode_roche_dims_workspace_bytes
    for D in cases.DIMS:
        P = (D - 4) * D + (D - 4) + 15
        for B in (1, 17, 3000):
            for lanes in (0, 1, 4):
                d = _desc(D, batch=B, lanes_per_patient=lanes)
                assert ws(d, L.WS_RK_FWD) == 0
                assert ws(d, L.WS_RK_BWD) == cases.n_waves(B, cases.rk_lpp(D, lanes, B)) * P * 4, (D, B, lanes)
            d = _desc(D, batch=B)
            total = ws(d, L.WS_DOPRI5_FWD)
            assert total == ws(d, L.WS_DOPRI5_BWD) > 0
            off = (ctypes.c_size_t * 5)()
            assert lib.hode_roche_dims_dopri5_tape_offsets(d, off) == 0
            assert list(off) == sorted(off) and off[4] + 65 * B * D * 4 <= total
    assert ws(_desc(12), L.WS_RK_BWD) == 0 and ws(_desc(12), L.WS_DOPRI5_FWD) == 0
    # the default: the quad layout below 131 072 patients at every size but 5 (at 20 000 patients the two layouts differ
    # in their number of waves: 20 per wave on 1 000 waves against 10 per wave on 2 000)
    def same(D, B, lanes):
        return ws(_desc(D, batch=B), L.WS_RK_BWD) == ws(_desc(D, batch=B, lanes_per_patient=lanes), L.WS_RK_BWD)
    for D in cases.DIMS:
        assert not same(D, 20000, 1) or not same(D, 20000, 4)
        assert same(D, 20000, 1 if D == 5 else 4), D
        assert same(D, 131072, 1), D


# ----------------------------------------------------------------------------------------------- 3. what stays as it was
def test_roche_solve_alone_still_refuses_a_size_of_the_side_library():
    """`library=None` is libhode.so: the refusal of D = 7 that tests/test_hip_rk.py::test_errors_are_loud relies on is the
    default's, and the choice of library is the caller's.  (Checked without a GPU through the signature and the C ABI.)"""
    import inspect
    import hode
    from hode import adaptive, _lib as L
    assert inspect.signature(hode.roche_solve).parameters["library"].default is None
    assert inspect.signature(adaptive.roche_dopri5).parameters["library"].default is None
    d = _desc(7, **{k: 64 for k in ("t", "y0", "dosage", "dose_times", "theta", "h", "w1", "b1")})
    assert hode.lib().hode_rk_fwd(d, None) == -3
    assert b"latent_dim 7 has no compiled kernel (have 4, 6, 8, 12, 20)" in hode.lib().hode_last_error_string()
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        hode.roche_solve(torch.zeros(2, 7), torch.zeros(L.N_THETA), torch.zeros(3, 7), torch.zeros(3), torch.arange(3.0),
                         torch.zeros(2), torch.zeros(2, 1))


@pytest.mark.parametrize("D,method", [(17, "rk4"), (3, "rk4"), (20, "dopri5"), (18, "dopri5")])
def test_error_text_for_a_size_nobody_serves(D, method):
    """model.RocheODE refuses before any library call, and names the sizes of both libraries."""
    import hode
    import model
    ode = model.RocheODE(max(D, 4), 1, 1.0, 0.125, device=CPU)
    ode.latent_dim = D
    ode.set_action(torch.zeros(9, 2, 1))
    with pytest.raises(hode.HodeConfigError) as e:
        ode.hode_solve(torch.zeros(2, D), torch.arange(9.0) * 0.125, 1e-7, 1e-8, method, {})
    text = str(e.value)
    assert ("4, 6, 8, 12 (libhode.so)" if method == "dopri5" else "4, 6, 8, 12, 20 (libhode.so)") in text
    assert SIZES.decode() + " (libhode_roche_dims.so)" in text and "(got %d)" % D in text
