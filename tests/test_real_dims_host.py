"""CPU checks of the real-data hybrid decoder's side library (no GPU): libhode_real_dims.so's C ABI and refusals,
its row of the build table, the kernels its objects contain against the GPU case table (tests/real_dims_cases.py), the
function that chooses the library per latent size, the refusal hode.real.real_solve makes before any launch, and what
stays as it was: libhode.so alone still refuses a size of the side library."""
import glob
import inspect
import os
import sys

import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import real_dims_cases as cases

ROOT = build_hip.ROOT
LIB = "libhode_real_dims.so"
FUNCTIONS = {"hode_real_dims_" + n for n in ("version", "last_error_string", "workspace_bytes", "rk_fwd", "rk_bwd")}
SIZES = b"latent_dim 5 .. 20 with hidden_dim 1 .. 64"
LIBHODE = b"libhode.so has latent_dim 4 and 20"
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    from hode import _real_dims_lib as RD
    return abi_checks.built(RD.LIBRARY)


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
def test_header_functions_are_exported_and_bound(lib):
    from hode import _real_dims_lib as RD
    declared = abi_checks.declared_functions("hode_real_dims.h", "hode_real_dims_")
    assert declared == {name for name, _, _ in RD.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_real_dims.h")
    assert "#define HODE_REAL_DIMS_ABI_VERSION %d\n" % RD.HODE_REAL_DIMS_ABI_VERSION in src
    assert lib.hode_real_dims_version() == RD.HODE_REAL_DIMS_ABI_VERSION
    assert '#include "hode.h"' in src and "struct" not in src   # the descriptor is hode.h's: included, not restated


def test_sizes_agree_everywhere():
    from hode import _real_dims_lib as RD
    assert RD.DIMS == cases.DIMS == tuple(range(5, 20))
    assert (RD.MIN_LATENT, RD.MAX_LATENT) == (cases.ACCEPTED[0], cases.ACCEPTED[-1]) == (5, 20)
    assert RD.MAX_HIDDEN == cases.MAX_HIDDEN == 16 * max(cases.HTS) == 16 * max(build_hip.REAL_DIMS_HTS)
    assert build_hip.REAL_DIMS_HTS == cases.HTS
    internal = open(os.path.join(build_hip.CSRC, "real_dims", "hode_real_dims.hpp")).read()
    assert "constexpr int kRealDimsMinLatent = 5, kRealDimsMaxLatent = 20, kRealDimsMaxHidden = 64;" in internal
    assert '#define HODE_REAL_DIMS_TEXT "%s"\n' % SIZES.decode() in internal
    side = open(os.path.join(build_hip.CSRC, "hode_real_side_host.hpp")).read()   # the hidden-tile counts: once, for the three side libraries
    assert "#define HODE_REAL_SIDE_HTS(X) " + " ".join("X(%d)" % n for n in cases.HTS) + "\n" in side
    assert "HODE_REAL_SIDE_HTS(HODE_REAL_DIMS_DECL)" in internal and "HODE_REAL_DIMS_HTS" not in internal
    # libhode.so's own sizes for this rhs, as its check states them
    assert RD.LIBHODE_DIMS == (4, 20)
    assert "(have 4, 20)" in open(os.path.join(build_hip.CSRC, "hode_real.hip")).read()


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    hashed = build_hip.digest_files(LIB)
    assert row.header == "include/hode_real_dims.h" and "include/hode.h" in hashed
    assert row.src_dir == build_hip.PKG + "/csrc/real_dims"
    want = ["hode_real_dims"] + ["hode_real_dims_ht%d" % n for n in cases.HTS]
    assert sorted(n for n, _, _ in row.units()) == sorted(want)
    assert build_hip.PKG + "/csrc/hode_real_mf.hpp" in hashed and build_hip.PKG + "/csrc/hode_rk_host.hpp" in hashed
    assert build_hip.PKG + "/csrc/hode_real_side_host.hpp" in hashed
    host = open(os.path.join(build_hip.CSRC, "real_dims", "hode_real_dims.hip")).read()
    assert "hode_error_state.hpp" in host and "__global__" not in host   # entry points only; the checks and the layout are the shared header's
    # libhode.so keeps its own unit of the shared device code
    assert "hode_real_mf" in [n for n, _, _ in build_hip.LIBRARIES["libhode.so"].units()]


def test_the_device_code_is_shared_not_copied():
    """Both libraries' kernels are wrappers around csrc/hode_real_mf.hpp: the rhs, its VJP and the gradient accumulator are
    defined there and nowhere else."""
    csrc = build_hip.CSRC
    shared = open(os.path.join(csrc, "hode_real_mf.hpp")).read()
    for name in ("struct RealMf", "struct RealGradAcc", "void real_mf_body(", "void real_grad_fold("):
        assert shared.count(name) == 1, name
        for other in ("hode_real_mf.hip", "real_dims/hode_real_dims_ht.hip", "real_dims/hode_real_dims.hip"):
            assert name not in open(os.path.join(csrc, other)).read(), (name, other)
    for unit in ("hode_real_mf.hip", "real_dims/hode_real_dims_ht.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert "real_mf_body<" in src and "real_grad_fold<" in src and "hode_real_mf.hpp" in src


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    """The kernel symbols of csrc/real_dims/build/*.o are the instantiations the case table states (HT x method x forward /
    backward, a fold per HT, the scalars' fold), every one is reached by a case, and every case names a compiled one."""
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        build_hip.build(verbose=False)
        objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    want = cases.expected_kernels()
    assert len(want) == 1 + len(cases.HTS) * (1 + 2 * len(cases.METHODS)) == 29
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert cases.kernels_reached() == compiled
    for group in (cases.COMPARE_CASES, cases.PADDING_CASES):
        assert cases.kernels_reached(group) <= compiled
    # no kernel here carries a name libhode.so's coverage guard reads
    assert not any(kv.family(n) for n in compiled - {"hode::fold_partials_kernel"})


def test_the_case_table_holds_what_it_promises():
    cs = cases.CASES
    assert {c["D"] for c in cs} == set(cases.DIMS)
    assert set(cases.EDGE_D) <= {c["D"] for c in cs} and cases.EDGE_D == (5, 7, 8, 9, 19)
    assert set(cases.EDGE_H) <= {c["H"] for c in cs} and cases.EDGE_H == (1, 16, 17, 43, 64)
    assert set(cases.EDGE_B) <= {c["B"] for c in cs} and cases.EDGE_B == (1, 15, 16, 17, 37)
    assert {(cases.ht(c["H"]), c["method"]) for c in cs} == {(n, m) for n in cases.HTS for m in cases.METHODS}
    assert all(c["B"] <= 37 and c["perturb"] == (c["method"] != "euler") for c in cs + cases.PADDING_CASES + cases.COMPARE_CASES)
    assert cases.TA <= 30 and cases.TA - cases.T0 + 1 >= 3 and cases.T0 >= 3    # >= two steps; doses before and inside
    assert [(c["D"], c["B"]) for c in cases.PADDING_CASES] == [(5, 17), (19, 1)]
    assert all(c["D"] == 20 for c in cases.COMPARE_CASES) and {c["method"] for c in cases.COMPARE_CASES} == set(cases.METHODS)
    assert cases.MODEL_DIMS == (7, 12) and cases.MODEL_STEP_DIVS == (1, 2)


# --------------------------------------------------------------------------------------------- 2. who serves which size
def test_library_selection(monkeypatch, tmp_path):
    """5 .. 19: the side library; everything else libhode.so -- without loading the side library for those."""
    import hode
    from hode import _real_dims_lib as RD
    monkeypatch.setattr(RD.LIBRARY, "handle", None)
    monkeypatch.setattr(RD.LIBRARY, "directory", str(tmp_path))   # nothing to load there
    monkeypatch.setattr(RD, "_as_libhode", None)
    for D in (1, 2, 3, 4, 20, 21, 22, 23, 24):
        assert RD.real_solver_library(D) is hode.lib()
    assert RD.LIBRARY.handle is None
    for D in range(5, 20):
        with pytest.raises(hode.HodeConfigError, match="libhode_real_dims.so not found"):
            RD.real_solver_library(D)
    monkeypatch.undo()
    abi_checks.built(RD.LIBRARY)
    side = RD.real_solver_library(5)
    for D in range(1, 25):
        got = RD.real_solver_library(D)
        assert (got is side and got is not hode.lib() and RD.is_side_library(got)) if 5 <= D <= 19 else (got is hode.lib() and not RD.is_side_library(got))
    for name, _, _ in RD.SOLVER_ENTRIES:
        assert callable(getattr(side, "hode_" + name))
    assert side.hode_workspace_bytes is RD.lib().hode_real_dims_workspace_bytes and side is RD.side_library()


def test_the_bindings_take_the_library_and_add_no_entry_point():
    from hode import real
    assert inspect.signature(real.real_solve).parameters["library"].default is None
    assert list(inspect.signature(real._RealFixedGrid.forward).parameters)[-2:] == ["lanes", "lib"]
    functions = [n for n, f in vars(real).items() if inspect.isfunction(f) and f.__module__ == real.__name__]
    assert sorted(functions) == ["_desc", "contract_tape", "real_solve"]
    classes = [n for n, c in vars(real).items() if inspect.isclass(c) and issubclass(c, torch.autograd.Function)]
    assert classes == ["_RealFixedGrid"]


@pytest.mark.parametrize("D,H,lanes", [(5, 65, 0), (12, 0, 0), (19, 100, 16), (7, 16, 1), (12, 43, 1)])
def test_real_solve_refuses_before_any_launch(D, H, lanes, monkeypatch, tmp_path):
    """A size of the side library with hidden > 64 or lanes_per_patient = 1: HodeConfigError with the sizes of both
    libraries, before a tensor is looked at (CPU tensors here) and before the side library is loaded."""
    import hode
    from hode import real, _real_dims_lib as RD
    monkeypatch.setattr(RD.LIBRARY, "handle", None)
    monkeypatch.setattr(RD.LIBRARY, "directory", str(tmp_path))
    with pytest.raises(hode.HodeConfigError) as e:
        real.real_solve(torch.zeros(2, D), torch.zeros(3), torch.zeros(cases.wflat_len(D, max(H, 0))), torch.arange(3.0),
                        torch.zeros(2, 2), H, lanes_per_patient=lanes)
    text = str(e.value)
    assert "latent_dim %d with hidden_dim %d, lanes_per_patient %d" % (D, H, lanes) in text
    assert "latent_dim 4, 20 at any hidden_dim (libhode.so" in text
    assert "latent_dim 5 .. 19 with hidden_dim 1 .. 64 on the matrix cores only (libhode_real_dims.so)" in text
    assert RD.LIBRARY.handle is None


def test_a_served_size_goes_on_to_the_gpu_check():
    """Inside the domain the next thing checked is the device of the tensors: nothing is refused for its size."""
    import hode
    from hode import real
    for D in (5, 12, 19, 20, 4):
        with pytest.raises(hode.HodeConfigError, match="HIP device"):
            real.real_solve(torch.zeros(2, D), torch.zeros(3), torch.zeros(cases.wflat_len(D, 43)), torch.arange(3.0),
                            torch.zeros(2, 2), 43)


# ----------------------------------------------------------------------------------------------- 3. the library's checks
def _desc(D, **over):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim, d.n_action_times = L.RHS_ROCHE_REAL, L.METHODS["rk4"], 17, D, 6, 43, 10
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_the_side_library_reports_its_own_error_text(lib):
    from hode import HodeConfigError, _lib as L, _real_dims_lib as RD
    side = RD.real_solver_library(10)
    with pytest.raises(HodeConfigError, match=r"hode_real_dims_rk_fwd failed \(code -3\): real dims: lanes_per_patient 1 "):
        side.hode_rk_fwd(_desc(10, lanes_per_patient=1), None)
    assert side.hode_workspace_bytes(_desc(10, lanes_per_patient=1), L.WS_RK_BWD) == 0


def test_argument_errors_do_not_launch(lib):
    from hode import _lib as L
    err = lib.hode_real_dims_last_error_string
    fwd, bwd = lib.hode_real_dims_rk_fwd, lib.hode_real_dims_rk_bwd
    for fn in (fwd, bwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(10, struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        for kind in (L.RHS_ROCHE, L.RHS_ROCHE_ABLATE, L.RHS_NEURAL):
            assert fn(_desc(10, rhs_kind=kind), None) == E_UNSUPPORTED and b"rhs_kind %d " % kind in err() and SIZES in err()
        for D in (0, 3, 4, 21, 24, 36):   # libhode.so's size 4 included; 20 is inside
            assert fn(_desc(D), None) == E_UNSUPPORTED and b"latent_dim %d " % D in err() and SIZES in err() and LIBHODE in err()
        for H in (0, -1, 65, 80):
            assert fn(_desc(10, hidden_dim=H), None) == E_UNSUPPORTED and b"hidden_dim %d " % H in err() and SIZES in err()
            assert LIBHODE in err()
        for lanes in (1, 4, 2, 48):
            assert fn(_desc(10, lanes_per_patient=lanes), None) == E_UNSUPPORTED and b"lanes_per_patient %d " % lanes in err()
            assert SIZES in err() and b"matrix-core layout only" in err()
        assert fn(_desc(10, method=3), None) == E_UNSUPPORTED and b"method 3" in err()
        assert fn(_desc(10, flags=L.FLAG_TAPE), None) == E_UNSUPPORTED and b"flags %d" % L.FLAG_TAPE in err()
        for D in cases.ACCEPTED:   # a shape of the domain, pointers missing
            assert fn(_desc(D), None) == E_NULL and b"must be non-NULL" in err()
        for k in ("batch", "n_times", "n_action_times"):
            assert fn(_desc(10, **{k: 0}), None) == E_SIZE and b"%s=0" % k.encode() in err()
    ptrs = {k: 64 for k in ("t", "y0", "dosage", "theta", "w1", "h")}
    for k in ptrs:
        assert fwd(_desc(10, **dict(ptrs, **{k: None})), None) == E_NULL
    assert fwd(_desc(10, **ptrs), None) == E_WORKSPACE and b"workspace 0 B < required" in err()
    assert bwd(_desc(10, **ptrs), None) == E_NULL and b"grad_h / grad_y0 / grad_theta" in err()
    ptrs.update(grad_h=64, grad_y0=64, grad_theta=64)
    assert bwd(_desc(10, **ptrs), None) == E_UNSUPPORTED and b"grad_w1 is NULL" in err() and b"operand-tape" in err()
    assert b"latent_dim 4 and 20" in err()
    ptrs.update(grad_w1=64)
    assert bwd(_desc(10, **ptrs), None) == E_WORKSPACE and b"workspace 0 B < required" in err()
    need = lib.hode_real_dims_workspace_bytes(_desc(10), L.WS_RK_BWD)
    assert bwd(_desc(10, workspace=64, workspace_bytes=need - 1, **ptrs), None) == E_WORKSPACE
    assert bwd(_desc(10, workspace=68, workspace_bytes=need, **ptrs), None) == E_ALIGN and b"16-byte aligned" in err()


def test_workspace_sizes_follow_the_layout(lib):
    """[ per-wave weight-gradient blocks of (4 HT + 3) 256 + 16 floats | three floats per wave | dose table 2 (Ta + 1) B
    floats ], each rounded up to 256 bytes; the forward holds the dose table alone.  The latent size does not enter."""
    from hode import _lib as L
    ws = lib.hode_real_dims_workspace_bytes

    def up(n):
        return -(-n // 256) * 256
    for D in cases.ACCEPTED:
        for H in (1, 16, 17, 43, 64):
            for B in (1, 16, 17, 37, 3000):
                for Ta in (1, 30):
                    d = _desc(D, hidden_dim=H, batch=B, n_action_times=Ta)
                    dose, nw = up(2 * (Ta + 1) * B * 4), -(-B // 16)
                    assert ws(d, L.WS_RK_FWD) == dose, (D, H, B, Ta)
                    assert ws(d, L.WS_RK_BWD) == up(nw * ((4 * cases.ht(H) + 3) * 256 + 16) * 4) + up(nw * 12) + dose, (D, H, B, Ta)
    for which in (L.WS_DOPRI5_FWD, L.WS_DOPRI5_BWD):
        assert ws(_desc(10), which) == 0
    for bad in (_desc(4), _desc(21), _desc(10, hidden_dim=65), _desc(10, lanes_per_patient=1), _desc(10, batch=0),
                _desc(10, rhs_kind=L.RHS_ROCHE)):
        assert ws(bad, L.WS_RK_FWD) == 0 and ws(bad, L.WS_RK_BWD) == 0
    # at size 20 the layout is libhode.so's own on-chip one (the same kernels' partial blocks)
    import hode
    d = _desc(20, grad_w1=64)
    assert ws(d, L.WS_RK_BWD) == hode.lib().hode_workspace_bytes(d, L.WS_RK_BWD)
    assert ws(d, L.WS_RK_FWD) == hode.lib().hode_workspace_bytes(d, L.WS_RK_FWD)


# ----------------------------------------------------------------------------------------------- 4. what stays as it was
def test_libhode_alone_still_refuses_a_size_of_the_side_library():
    import hode
    ptrs = {k: 64 for k in ("t", "y0", "dosage", "theta", "w1", "h")}
    for D in (5, 12, 19):
        assert hode.lib().hode_rk_fwd(_desc(D, **ptrs), None) == E_UNSUPPORTED
        assert b"latent_dim %d has no compiled kernel (have 4, 20)" % D in hode.lib().hode_last_error_string()
