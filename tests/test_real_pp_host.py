"""CPU checks of dopri5 with per-patient step control for the real-data hybrid rhs (no GPU): libhode_real_pp.so's C ABI, its
row in build_hip.PATIENT_LIBRARIES with its digest, stamp and loader refusals, the compiled kernels against the case table
(tests/real_pp_cases.py), "compiled, not copied", the library's own refusals, the switch RocheODEReal.step_control with its
refusals and the unchanged ones, and the case table's guard on the float64 eager controller (tests/real_pp_eager.py)."""
import ctypes
import glob
import importlib.util
import os
import re
import shutil
import sys

import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import model
import real_pp_cases as cases
import real_pp_eager as eager
import reference_checks as rc

ROOT = build_hip.ROOT
LIB = "libhode_real_pp.so"
FUNCTIONS = {"hode_real_pp_" + n for n in ("version", "last_error_string", "workspace_bytes", "fwd", "bwd", "tape_offsets")}
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
CPU = torch.device("cpu")
SIZES = "latent_dim 5 .. 20 with hidden_dim 1 .. 64, dopri5 with per-patient step control"


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _real_pp_lib as PL
    if not os.path.exists(PL.LIBRARY.path()):
        build_hip.build(verbose=False)
    return PL.LIBRARY.load()


def test_header_functions_are_exported_and_bound(lib):
    from hode import _flow_lib, _lib, _real_pp_lib as PL
    declared = abi_checks.declared_functions("hode_real_pp.h", "hode_real_pp_")
    assert declared == {name for name, _, _ in PL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    assert "#define HODE_REAL_PP_ABI_VERSION %d\n" % PL.HODE_REAL_PP_ABI_VERSION in abi_checks.header_text("hode_real_pp.h")
    assert lib.hode_real_pp_version() == PL.HODE_REAL_PP_ABI_VERSION
    assert (PL.MIN_LATENT, PL.MAX_LATENT, PL.MAX_HIDDEN) == (cases.MIN_LATENT, cases.MAX_LATENT, cases.MAX_HIDDEN)
    assert build_hip.REAL_PP_HTS == cases.HTS
    assert "5 .. 20" in PL.sizes_text() and "1 .. 64" in PL.sizes_text() and LIB in PL.sizes_text()
    assert (PL.LIBRARY.file_name, PL.LIBRARY.env, PL.LIBRARY.check_digest) == (LIB, "HODE_REAL_PP_LIBRARY", True)
    assert not FUNCTIONS & {e[0] for e in _lib.EXPORTS + _flow_lib.EXPORTS}


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _real_pp_lib as PL
    abi_checks.assert_c_layout("hode_real_pp.h", "hode_real_pp_desc", PL.RealPpDesc, tmp_path)
    assert PL.new_desc().struct_size == ctypes.sizeof(PL.RealPpDesc)
    assert [n for n, _ in PL.RealPpDesc._fields_] == [
        "struct_size", "batch", "latent_dim", "hidden_dim", "n_times", "n_action_times", "max_steps", "max_attempts", "flags",
        "rtol", "atol", "t", "y0", "act", "theta", "wflat", "h", "status", "n_accepted", "n_rejected", "patient_status",
        "grad_h", "grad_y0", "grad_wflat", "grad_theta", "workspace", "workspace_bytes"]


def test_the_row_is_in_a_fourth_table_and_the_first_three_are_as_they_were():
    assert list(build_hip.MORE_LIBRARIES) == ["libhode_dose.so"] and list(build_hip.LATER_LIBRARIES) == ["libhode_real_dose.so"]
    assert list(build_hip.PATIENT_LIBRARIES) == [LIB]
    assert [r.name for r in build_hip.every_library()] == list(build_hip.LIBRARIES) + ["libhode_dose.so", "libhode_real_dose.so"]
    assert [r.name for r in build_hip.built_libraries()] == [r.name for r in build_hip.every_library()] + [LIB]
    assert len(build_hip.built_libraries()) == 17 == len({r.name for r in build_hip.built_libraries()})
    row = build_hip.PATIENT_LIBRARIES[LIB]
    assert isinstance(row, build_hip.Library) and build_hip.library(LIB) is row
    assert all(build_hip.library(r.name) is r for r in build_hip.built_libraries())
    with pytest.raises(KeyError):
        build_hip.library("libhode_nothing.so")
    assert row.name == LIB and row.out == os.path.join(ROOT, build_hip.PKG, "hode", LIB)
    assert row.header == "include/hode_real_pp.h" and row.src_dir == build_hip.PKG + "/csrc/real_pp"
    assert row.obj == os.path.join(ROOT, row.src_dir, "build")
    units = [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()]
    assert units[0] == ("hode_real_pp", row.src_dir + "/hode_real_pp.hip", ["-Wno-unused-function"])
    assert units[1:] == [("hode_real_pp_ht%d" % n, row.src_dir + "/hode_real_pp_ht.hip", ["-DHODE_REAL_PP_HT=%d" % n])
                         for n in build_hip.REAL_PP_HTS]
    # build() covers the fourth table: compile, link, stamp
    src = open(os.path.join(ROOT, "build_hip.py")).read()
    body = src[src.index("def build("):src.index("def build_variant(")]
    assert body.count("for lib in built_libraries():") == 2 and "every_library()" not in body


def test_the_device_code_is_compiled_not_copied():
    """The controller, the clipping, the tape and the sweep are this directory's; the rhs, its VJP, the accumulator, its fold,
    the dose table and the state I/O are hode_real_mf.hpp's / hode_real_args.hpp's, the tableau, the stage times and the step
    factor hode_dopri5_kernels.hpp's: named here, defined there."""
    src = open(os.path.join(build_hip.CSRC, "real_pp", "hode_real_pp_ht.hip")).read()
    for name in ("RealMf<HT, RealTileRagged>", "nn.rhs(", "nn.vjp(", "RealGradAcc<HT>", "acc.add(", "acc.store(", "real_grad_fold<HT>",
                 "real_dose_table(", "real_set_dose(", "real_load_state(", "real_store_state(", "kDpBeta[", "kDpErr[",
                 "dp_step_factor(", "dp_stage_time(", '#include "../hode_real_mf.hpp"', '#include "../hode_dopri5_kernels.hpp"',
                 "__launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))", "__builtin_amdgcn_ballot_w64(run)"):
        assert name in src, name
    for definition in ("struct RealMf", "struct RealGradAcc", "HODE_DEV void real_grad_fold", "HODE_DEV void real_load_state",
                       "HODE_DEV void real_store_state", "HODE_DEV void real_set_dose", "HODE_DEV void real_dose_table",
                       "HODE_DEV DoseK real_dose", "mfma4(", "kDpBeta[6][6]", "kDpAlpha[6]", "kDpErr[7] =", "double dp_step_factor",
                       "float dp_stage_time", "35.0 / 384", "tanh_scaled4(", "atomicAdd"):
        assert definition not in src, definition
    assert src.count("atomic") == 1 and "atomicOr(a.status, status)" in src   # the status word alone; no atomics on gradients
    shared = open(os.path.join(build_hip.CSRC, "hode_real_mf.hpp")).read() + open(os.path.join(build_hip.CSRC, "hode_real_args.hpp")).read()
    for definition in ("struct RealMf", "struct RealGradAcc", "HODE_DEV void real_grad_fold", "HODE_DEV void real_load_state",
                       "HODE_DEV void real_store_state", "HODE_DEV void real_set_dose", "HODE_DEV void real_dose_table"):
        assert definition in shared, definition
    dp = open(os.path.join(build_hip.CSRC, "hode_dopri5_kernels.hpp")).read()
    for definition in ("kDpBeta[6][6]", "kDpErr[7]", "HODE_DEV double dp_step_factor", "HODE_DEV float dp_stage_time"):
        assert definition in dp, definition
    # every loop of the kernels is bounded by max_attempts, max_steps or T, or has a compile-time trip count
    assert "it >= a.max_attempts" in src and "n_acc >= a.max_steps" in src and "min(max(a.n_acc[p], 0), a.max_steps)" in src
    assert not re.search(r"while\s*\(", src)
    host = open(os.path.join(build_hip.CSRC, "real_pp", "hode_real_pp.hip")).read()
    assert "hode_error_state.hpp" in host and "__global__" not in host
    for shared_host in ("real_side_check_domain(", "real_side_check_sizes(", "real_side_check_workspace(", "real_side_layout(",
                        "real_side_launch(", "real_side_blocks("):
        assert shared_host in host, shared_host
    files = build_hip.digest_files(LIB)
    for f in ("hode_real_mf.hpp", "hode_real_args.hpp", "hode_common.hpp", "hode_rk_host.hpp", "hode_error_state.hpp", "hode_host.hpp",
              "hode_real_side_host.hpp", "hode_dopri5_kernels.hpp", "real_pp/hode_real_pp.hpp", "real_pp/hode_real_pp_ht.hip",
              "real_pp/hode_real_pp.hip"):
        assert build_hip.PKG + "/csrc/" + f in files, f
    assert "include/hode_real_pp.h" in files and "include/hode.h" in files


# ------------------------------------------------------------------------------------------- 2. digest, stamp, loader
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """build_hip.py of a copy of the sources elsewhere.  A test that edits a file of the copy puts it back."""
    tmp = tmp_path_factory.mktemp("tree")
    shutil.copy(os.path.join(ROOT, "build_hip.py"), tmp / "build_hip.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp / "include")
    shutil.copytree(build_hip.CSRC, tmp / build_hip.PKG / "csrc", ignore=shutil.ignore_patterns("build"))
    spec = importlib.util.spec_from_file_location("_build_hip_real_pp_copy", str(tmp / "build_hip.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert module.ROOT == str(tmp) != ROOT
    return module


def _edited(tree, paths, fn):
    kept = {p: open(os.path.join(tree.ROOT, p), "rb").read() for p in paths}
    try:
        for p, text in kept.items():
            open(os.path.join(tree.ROOT, p), "wb").write(text + b"\n")
        return fn()
    finally:
        for p, text in kept.items():
            open(os.path.join(tree.ROOT, p), "wb").write(text)


def test_digest_follows_an_edit_of_each_of_its_files_and_of_no_other(tree):
    files = tree.digest_files(LIB)
    assert files == build_hip.digest_files(LIB) == sorted(files)
    before = tree.digest(LIB)
    assert before == build_hip.digest(LIB)  # and it does not depend on where the tree lives
    for f in files:
        assert _edited(tree, [f], lambda: tree.digest(LIB)) != before, f
    others = [os.path.relpath(os.path.join(d, f), tree.ROOT).replace(os.sep, "/")
              for top in ("include", build_hip.PKG) for d, _, fs in os.walk(os.path.join(tree.ROOT, top)) for f in fs]
    others = sorted(set(others) - set(files))
    assert others and _edited(tree, others, lambda: tree.digest(LIB)) == before
    own = [f for f in files if "/real_pp/" in f or f.endswith("hode_real_pp.h")]
    assert len(own) == 4
    for name in ("libhode.so", "libhode_real_dims.so", "libhode_real_dose.so", "libhode_dopri5_pp.so"):
        was = tree.digest(name)
        assert _edited(tree, own, lambda: tree.digest(name)) == was, name


def test_library_digest_matches_sources(lib):
    out = build_hip.library(LIB).out
    assert os.path.exists(out + ".digest"), "%s has no source digest: rebuild with `python build_hip.py`" % LIB
    assert open(out + ".digest").read().strip() == build_hip.digest(LIB), "%s is stale: run `python build_hip.py`" % LIB


def test_a_missing_and_a_stale_library_are_refused_with_a_message(lib, tmp_path, monkeypatch):
    from hode import HodeConfigError
    from hode import _real_pp_lib as PL
    library, out = PL.LIBRARY, build_hip.library(LIB).out
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "directory", str(tmp_path))
    monkeypatch.delenv("HODE_REAL_PP_LIBRARY", raising=False)
    with pytest.raises(HodeConfigError, match=r"libhode_real_pp\.so not found -- build it with `python build_hip\.py`.*no CPU fallback for %s"
                       % re.escape(library.noun)):
        library.load()
    shutil.copy(out, tmp_path / LIB)
    (tmp_path / (LIB + ".digest")).write_text("0" * 64 + "\n")
    with pytest.raises(HodeConfigError, match=r"libhode_real_pp\.so is stale .*rebuild with `python build_hip\.py`"):
        library.load()
    shutil.copy(out + ".digest", tmp_path / (LIB + ".digest"))
    assert library.load().hode_real_pp_version() == library.abi_version
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "abi_version", library.abi_version + 1)
    with pytest.raises(HodeConfigError, match=r"libhode_real_pp\.so ABI version 1 != expected 2"):
        library.load()


def test_importing_loads_nothing():
    abi_checks.assert_import_does_not_load(["hode._real_pp_lib"], modules=("hode", "model", "hode.real_pp"))


# ---------------------------------------------------------------------------------- 3. compiled kernels / case table
def _objects():
    objs = sorted(glob.glob(os.path.join(build_hip.library(LIB).obj, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    return [(dem, kd) for o in objs for dem, kd in kernel_descriptors(o)]


def test_every_compiled_kernel_is_named_by_a_case_and_every_case_names_one():
    compiled = {kv.kernel_name(dem) for dem, _ in _objects()}
    want = cases.expected_kernels()
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert cases.kernels_reached(cases.CASES) == want and len(want) == 3 * 4 + 1


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    assert len(set(map(cases.case_id, cs))) == len(cs) <= 16
    assert {c["B"] for c in cs} == set(cases.EDGE_B) and cases.EDGE_B == (1, 15, 16, 17, 33)
    assert {c["D"] for c in cs} == set(cases.EDGE_D) and cases.EDGE_D == (5, 12, 20)
    assert {c["H"] for c in cs} == set(cases.EDGE_H) and cases.EDGE_H == (1, 16, 17, 43, 64)
    assert {cases.ht(c["H"]) for c in cs} == set(cases.HTS) == {cases.ht(c["H"]) for c in cs if c["stiff"]}
    for g in ("uniform", "ragged", "offset+"):
        assert {c["T"] for c in cs if c["grid"] == g and not c["stiff"]} >= set(cases.EDGE_T), g
    assert any(c["grid"] == "offset-" for c in cs)
    assert {(c["rtol"], c["atol"]) for c in cs} == {cases.TOL, cases.DECODER_TOL} == {(1e-5, 1e-7), (1e-7, 1e-8)}
    assert sum((c["rtol"], c["atol"]) == cases.DECODER_TOL for c in cs) == 1
    assert all(c["B"] > cases.STIFF and c["grid"] == "late" for c in cs if c["stiff"])
    for c in cs:
        _, p = cases.inputs(c)
        B, D, T, Ta = c["B"], c["D"], c["T"], cases.n_action_rows(c)
        assert p["a"].shape == (Ta, B, 1) and p["y0"].shape == (B, D) and p["cot"].shape == (T, B, D) and p["t"].shape == (T,)
        assert p["wflat"].numel() == cases.wflat_len(D, c["H"]) and all(v.dtype == torch.float32 for v in p.values())
        assert bool((p["t"][1:] > p["t"][:-1]).all()) and Ta >= float(p["t"][-1])   # Ta >= the last hour
        assert float(p["a"][0, 0]) > 0.5 and float(p["a"][Ta - 1, 0]) > 0.3           # a dose in the first and in the last hour
        if B > 1:
            assert not p["a"][:, cases.ZERO_PATIENT].any()
        if Ta > 2:
            assert not p["a"][cases.ZERO_HOUR].any()


# ------------------------------------------------------------------------------------------ 4. the library's refusals
def _desc(**kw):
    from hode import _real_pp_lib as PL
    d = PL.new_desc()
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times, d.max_steps = 5, 9, 17, 6, 12, 100
    d.rtol, d.atol = 1e-5, 1e-7
    for k in ("t", "y0", "act", "theta", "wflat", "h", "status", "n_accepted", "n_rejected", "patient_status", "grad_h", "grad_y0",
              "grad_wflat", "grad_theta", "workspace"):
        setattr(d, k, 4096)  # never dereferenced: every call below is refused before a launch
    d.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, d, code, text, entries=("fwd", "bwd")):
    for e in entries:
        assert getattr(lib, "hode_real_pp_" + e)(ctypes.byref(d), None) == code, e
        assert text in lib.hode_real_pp_last_error_string().decode(), lib.hode_real_pp_last_error_string()


def test_every_argument_error_returns_its_code_without_a_launch(lib):
    for D in (4, 3, 21, 24):
        d = _desc(latent_dim=D)
        _refused(lib, d, E_UNSUPPORTED, "real per-patient dopri5: latent_dim %d has no compiled kernel (have %s)" % (D, SIZES))
        assert lib.hode_real_pp_workspace_bytes(ctypes.byref(d)) == 0
    for H in (0, 65, 80):
        d = _desc(hidden_dim=H)
        _refused(lib, d, E_UNSUPPORTED, "real per-patient dopri5: hidden_dim %d has no compiled kernel (have %s)" % (H, SIZES))
        assert lib.hode_real_pp_workspace_bytes(ctypes.byref(d)) == 0
    _refused(lib, _desc(flags=4), E_UNSUPPORTED, "real per-patient dopri5: flags 4 (have HODE_FLAG_NO_TAPE)")
    _refused(lib, _desc(flags=16), E_UNSUPPORTED, "there is no tape to sweep", entries=("bwd",))
    _refused(lib, _desc(struct_size=8), E_SIZE, "ABI mismatch")
    for field in ("batch", "n_times", "n_action_times"):
        _refused(lib, _desc(**{field: 0}), E_SIZE, "bad sizes: batch=")
    _refused(lib, _desc(max_steps=0), E_SIZE, "bad sizes: max_steps=0")
    _refused(lib, _desc(max_attempts=-1), E_SIZE, "max_attempts=-1")
    _refused(lib, _desc(rtol=0.0), E_SIZE, "rtol must be > 0 and atol >= 0")
    _refused(lib, _desc(atol=-1.0), E_SIZE, "rtol must be > 0 and atol >= 0")
    _refused(lib, _desc(rtol=float("nan")), E_SIZE, "rtol must be > 0 and atol >= 0")
    for field in ("t", "y0", "act", "theta", "wflat", "h"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "t / y0 / act (dose table) / theta / wflat (flat weights) / h must be non-NULL")
    for field in ("status", "n_accepted", "n_rejected", "patient_status"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "status / n_accepted / n_rejected / patient_status must be non-NULL")
    for field in ("grad_h", "grad_y0", "grad_wflat", "grad_theta"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "grad_h / grad_y0 / grad_wflat / grad_theta required by the backward", entries=("bwd",))
    _refused(lib, _desc(workspace_bytes=64), E_WORKSPACE, "workspace 64 B < required")
    _refused(lib, _desc(workspace=0), E_WORKSPACE, "< required")
    for off in (4, 8):
        _refused(lib, _desc(workspace=4096 + off), E_ALIGN, "workspace must be 16-byte aligned")
    assert lib.hode_real_pp_fwd(None, None) == E_NULL and lib.hode_real_pp_bwd(None, None) == E_NULL
    assert lib.hode_real_pp_workspace_bytes(None) == 0
    off = (ctypes.c_size_t * 4)()
    assert lib.hode_real_pp_tape_offsets(ctypes.byref(_desc()), None) == E_NULL
    assert lib.hode_real_pp_tape_offsets(ctypes.byref(_desc(latent_dim=4)), off) == E_UNSUPPORTED

    # the layout, restated: gradient blocks | the three scalars' rows | tape_t | tape_dt | tape_j | tape_y | the dose table
    def al(n):
        return -(-n // 256) * 256
    for B, D, H, Ta, steps, flags in ((5, 9, 17, 12, 100, 0), (37, 20, 64, 3, 7, 0), (1, 5, 1, 1, 1, 0), (1027, 12, 43, 40, 33, 16)):
        waves, n_ht = -(-B // 16), -(-H // 16)
        cells = 0 if flags else steps * B
        head = al(waves * ((4 * n_ht + 3) * 256 + 16) * 4) + al(waves * 3 * 4)
        tapes = [al(cells * 8), al(cells * 8), al(cells * 4), al(cells * D * 4)]
        want = head + sum(tapes) + al(2 * (Ta + 1) * B * 4)
        d = _desc(batch=B, latent_dim=D, hidden_dim=H, n_action_times=Ta, max_steps=steps, flags=flags)
        assert lib.hode_real_pp_workspace_bytes(ctypes.byref(d)) == want
        assert lib.hode_real_pp_tape_offsets(ctypes.byref(d), off) == 0
        assert list(off) == [head, head + tapes[0], head + sum(tapes[:2]), head + sum(tapes[:3])]


# ------------------------------------------------------------------------- 5. the switch, and refusals before a load
@pytest.fixture
def no_library(monkeypatch):
    from hode import _real_pp_lib as PL

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(PL.LIBRARY, "load", boom)
    monkeypatch.setattr(PL, "lib", boom)


def _ode(D=7, H=16, action_dim=1):
    torch.manual_seed(0)
    return model.RocheODEReal(D, action_dim, 3, H, 12, 1, device=CPU)


def _action(Ta=12, B=3, cols=1, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(Ta, B, cols, generator=gen) < 0.3).float() * torch.rand(Ta, B, cols, generator=gen)


T_OUT = torch.arange(5.0, 12.0)


def test_the_config_errors(no_library):
    import hode
    from hode import real_pp
    ode = _ode()
    assert ode.step_control == "batch" and "step_control" not in dict(ode.named_parameters())
    ode.set_action_static(_action(), None)
    y0 = torch.rand(3, 7) * 0.1
    # kept as they are: dopri5 with the default control; a fixed-grid method with "patient"; dopri5 with a 3-D init
    with pytest.raises(hode.HodeConfigError, match=r"RocheODEReal is built for the fixed-grid methods \(euler, midpoint, rk4\); dopri5"):
        hode.odeint(ode, y0, T_OUT, method="dopri5")
    with pytest.raises(hode.HodeConfigError, match=r"RocheODEReal is built for the fixed-grid methods \(euler, midpoint, rk4\); dopri5"):
        hode.odeint(ode, y0, T_OUT, method="dopri5", options={"step_control": "batch"})
    for method in ("euler", "midpoint", "rk4"):
        with pytest.raises(hode.HodeConfigError, match="RocheODEReal has no per-patient step control"):
            hode.odeint(ode, y0, T_OUT, method=method, options={"step_control": "patient"})
    ode.step_control = "patient"
    with pytest.raises(hode.HodeConfigError, match=r"RocheODEReal is built for the fixed-grid methods \(euler, midpoint, rk4\); dopri5"):
        ode.hode_solve_steps(torch.zeros(6, 3, 7), T_OUT, "dopri5", {})
    with pytest.raises(hode.HodeConfigError, match="is not one of"):
        hode.odeint(ode, y0, T_OUT, method="dopri5", options={"step_control": "lane"})
    # new, each before anything is loaded: the sizes
    for D, H, got in ((4, 16, "latent dimension 4"), (21, 16, "latent dimension 21"), (24, 9, "latent dimension 24"),
                      (7, 65, "hidden dimension 65"), (20, 80, "hidden dimension 80")):
        bad = _ode(D, H)
        bad.step_control = "patient"
        bad.set_action_static(_action(), None)
        with pytest.raises(hode.HodeConfigError, match=r"latent dimensions 5 \.\. 20 with hidden_dim 1 \.\. 64 .*\(libhode_real_pp\.so\) \(got %s\)" % got):
            hode.odeint(bad, torch.rand(3, D) * 0.1, T_OUT, method="dopri5")
    with pytest.raises(hode.HodeConfigError, match="5 .. 20"):
        real_pp.check_domain(4, 16)
    with pytest.raises(hode.HodeConfigError, match="1 .. 64"):
        real_pp.check_domain(12, 0)
    real_pp.check_domain(5, 1)
    real_pp.check_domain(20, 64)
    # a step_t that is not the output grid
    for step_t in (torch.arange(5.0, 12.0, 0.5), torch.arange(5.0, 11.0), T_OUT + 0.25):
        with pytest.raises(hode.HodeConfigError, match=r"options\['step_t'\] must be the output grid"):
            hode.odeint(ode, y0, T_OUT, method="dopri5", options={"step_t": step_t})
    # dose_grad with a differentiable action
    ode.dose_grad = True
    ode.set_action_static(_action().requires_grad_(True), None)
    with pytest.raises(hode.HodeConfigError, match=r"dose_grad serves the fixed-grid methods .*has no dose-table gradient"):
        hode.odeint(ode, y0, T_OUT, method="dopri5", options={"step_t": T_OUT})
    ode.dose_grad = False
    # CPU tensors: the solver path's own refusal (step_t as the same tensor, as an equal one, or absent; step_size / perturb ignored)
    for options in ({}, {"step_t": T_OUT}, {"step_t": T_OUT.clone(), "step_size": 0.5, "perturb": True}):
        with pytest.raises(hode.HodeConfigError, match="HIP device"):
            hode.odeint(ode, y0, T_OUT, method="dopri5", options=options)
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        real_pp.real_patient_dopri5_forward(y0, torch.ones(3), torch.zeros(cases.wflat_len(7, 16)), T_OUT, torch.zeros(12, 3), 16)


def test_switch_on_reaches_the_function_and_switch_off_does_not(monkeypatch):
    import hode
    from hode import real
    seen = {"pp": [], "plain": []}

    class Fake:
        @staticmethod
        def apply(y0, theta, wflat, t, act, hidden, rtol, atol, grad_enabled):
            seen["pp"].append((hidden, t.numel(), tuple(act.shape), act.requires_grad, rtol, atol, grad_enabled, act.detach().clone()))
            return torch.zeros(t.numel(), *y0.shape)

    def plain(y0, theta, wflat, grid, act, hidden, method="midpoint", perturb=True, lanes_per_patient=0, library=None):
        seen["plain"].append((method, perturb))
        return torch.zeros(grid.numel(), *y0.shape)
    monkeypatch.setattr(model, "_RocheRealPatientDopri5", Fake)
    monkeypatch.setattr(real, "real_solve", plain)
    monkeypatch.setattr(hode.solver, "_require_gpu", lambda *a: None)
    ode = _ode()
    y0 = torch.rand(3, 7) * 0.1
    a = _action().requires_grad_(True)
    ode.set_action_static(a, None)
    hode.odeint(ode, y0, T_OUT, method="rk4")  # the default: today's call
    assert seen["pp"] == [] and seen["plain"] == [("rk4", False)]
    h = hode.odeint(ode, y0, T_OUT, rtol=1e-6, atol=1e-9, method="dopri5", options={"step_control": "patient", "step_t": T_OUT})
    assert h.shape == (7, 3, 7) and seen["pp"][0][:7] == (16, 7, (12, 3), False, 1e-6, 1e-9, True)
    assert torch.equal(seen["pp"][0][7], a.detach()[..., 0])   # the dose table travels detached: no gradient for the action
    ode.step_control = "patient"
    with torch.no_grad():
        hode.odeint(ode, y0, T_OUT, method="dopri5")
    assert seen["pp"][1][6] is False and len(seen["plain"]) == 1
    # the whole opt-in of a user: one attribute on a default-constructed decoder
    dec = model.DecoderReal(5, 7, 1, 3, 16, 12, 1, t0=6, ode_type="hybrid", device=CPU)
    assert dec.method == "dopri5" and dec.options["step_t"] is dec.t and (dec.rtol, dec.atol) == (1e-7, 1e-8)
    with pytest.raises(hode.HodeConfigError, match="RocheODEReal is built for the fixed-grid methods"):
        dec.latent(torch.zeros(3, 7), _action(), None)
    dec.ode.step_control = "patient"
    assert dec.latent(torch.zeros(3, 7), _action(), None).shape == (dec.t.numel(), 3, 7)
    assert seen["pp"][2][:3] == (16, dec.t.numel(), (12, 3)) and seen["pp"][2][4:6] == (1e-7, 1e-8)
    # a two-column action is summed before the call
    ode2 = _ode(action_dim=2)
    ode2.step_control = "patient"
    a2 = _action(cols=2, seed=1)
    ode2.set_action_static(a2, None)
    hode.odeint(ode2, y0, T_OUT, method="dopri5")
    assert torch.equal(seen["pp"][3][7], a2.sum(-1))


def test_the_autograd_function_lives_next_to_the_module_it_serves():
    """tests/test_binding_case_coverage.py walks hode/*.py: only launch functions there, the Function in model.py."""
    import test_binding_case_coverage as cov
    assert not [b for b in cov.bindings() if b.startswith(("real_pp.", "_real_pp_lib."))]
    assert issubclass(model._RocheRealPatientDopri5, torch.autograd.Function)
    assert not cov.pointer_problems()


# ------------------------------------------------------------------------------------------ 6. the case table's guard
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_the_cases_are_guarded_by_the_float64_eager_controller(c):
    """A condition, not a measurement.  The float64 eager run finishes every patient inside max_steps with a clipped tape; a
    stiff case has the promised spread (the scaled-up patient has rejections, the step counts differ inside its tile, the first
    attempt of some patients is rejected and of others accepted); the float64 replay yields finite, non-zero gradients.  Measured
    beside it (printed): the float32 eager replay against the float64 one on the same tapes, which has to stay inside a tenth
    of the family bounds of tests/reference_checks.py for those bounds to be used unwidened."""
    runs = cases.controller(c)
    _, p = cases.inputs(c)
    assert all(r["status"] == 0 and c["T"] - 1 <= r["n_accepted"] <= cases.max_steps(c) for r in runs)
    assert all(eager.tape_is_clipped(r["tape"], p["t"]) for r in runs)
    assert all(bool(torch.isfinite(r["h"]).all()) for r in runs)
    if c["stiff"]:
        tile = runs[:16]
        counts = [r["n_accepted"] for r in tile]
        first = [r["ratios"][0] > 1 for r in runs]
        assert max(counts) > min(counts) and runs[cases.STIFF]["n_rejected"] > 0
        assert any(first) and not all(first)
    tapes = [r["tape"] for r in runs]
    r64, r32 = cases.replay(c, tapes), cases.replay(c, tapes, torch.float32)
    for k in ("h", "gy0", "gw", "gth"):
        assert bool(torch.isfinite(r64[k]).all()) and float(r64[k].abs().max()) > 0, k
    assert torch.equal(r64["h"], torch.cat([r["h"] for r in runs], dim=1))   # the replay walks the controller's own steps
    herr = float((r32["h"].double() - r64["h"]).abs().max()) / (1 + float(r64["h"].abs().max()))
    errs = {k: cases.rel_l2(r32[k], r64[k]) for k in ("gy0", "gw", "gth")}
    print("%s: float32 replay vs float64: h %.2e, %s" % (cases.case_id(c), herr, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert herr <= rc.TRAJ_TOL / 10 and all(v <= rc.GRAD_TOL / 10 for v in errs.values())


def test_a_first_attempt_of_the_scaled_up_patient_itself_is_rejected_in_some_case():
    hit = [cases.case_id(c) for c in cases.CASES if c["stiff"] and cases.controller(c)[cases.STIFF]["ratios"][0] > 1]
    assert hit, "no stiff case rejects the first attempt of patient STIFF"
