"""CPU checks of the real-data dose-table gradient (no GPU): libhode_real_dose.so's C ABI, its row in
build_hip.LATER_LIBRARIES with its digest, stamp and loader refusals, the compiled kernels against the case table
(tests/real_dose_cases.py), the library's own refusals, the switch RocheODEReal.dose_grad and its refusals, the case table
against the oracle's own fp32 error, and the tap / reverse scan restated in numpy against the oracle's autograd."""
import ctypes
import glob
import importlib.util
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import model
import real_dose_cases as cases

ROOT = build_hip.ROOT
LIB = "libhode_real_dose.so"
FUNCTIONS = {"hode_real_dose_" + n for n in ("version", "last_error_string", "workspace_bytes", "bwd")}
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
CPU = torch.device("cpu")
SIZES = "latent_dim 5 .. 20 with hidden_dim 1 .. 64, methods euler / midpoint / rk4"


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _real_dose_lib as DL
    if not os.path.exists(DL.LIBRARY.path()):
        build_hip.build(verbose=False)
    return DL.LIBRARY.load()


def test_header_functions_are_exported_and_bound(lib):
    from hode import _flow_lib, _lib, _real_dose_lib as DL
    declared = abi_checks.declared_functions("hode_real_dose.h", "hode_real_dose_")
    assert declared == {name for name, _, _ in DL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    assert "#define HODE_REAL_DOSE_ABI_VERSION %d\n" % DL.HODE_REAL_DOSE_ABI_VERSION in abi_checks.header_text("hode_real_dose.h")
    assert lib.hode_real_dose_version() == DL.HODE_REAL_DOSE_ABI_VERSION
    assert (DL.MIN_LATENT, DL.MAX_LATENT, DL.MAX_HIDDEN) == (cases.MIN_LATENT, cases.MAX_LATENT, cases.MAX_HIDDEN)
    assert DL.METHODS == tuple(cases.METHODS) and build_hip.REAL_DOSE_HTS == cases.HTS
    assert "5 .. 20" in DL.sizes_text() and "1 .. 64" in DL.sizes_text() and LIB in DL.sizes_text()
    assert (DL.LIBRARY.file_name, DL.LIBRARY.env, DL.LIBRARY.check_digest) == (LIB, "HODE_REAL_DOSE_LIBRARY", True)
    # no export shares a name with libhode.so's or libhode_flow.so's (tests/test_binding_case_coverage.py walks for those)
    assert not FUNCTIONS & {e[0] for e in _lib.EXPORTS + _flow_lib.EXPORTS}


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _real_dose_lib as DL
    abi_checks.assert_c_layout("hode_real_dose.h", "hode_real_dose_desc", DL.RealDoseDesc, tmp_path)
    assert DL.new_desc().struct_size == ctypes.sizeof(DL.RealDoseDesc)
    assert [n for n, _ in DL.RealDoseDesc._fields_] == [
        "struct_size", "method", "perturb", "batch", "latent_dim", "hidden_dim", "n_times", "n_action_times", "flags",
        "t", "h", "act", "theta", "wflat", "grad_h", "grad_y0", "grad_act", "grad_wflat", "grad_theta", "workspace", "workspace_bytes"]


def test_the_row_is_in_the_third_table_and_the_first_two_are_as_they_were():
    assert sorted(build_hip.LIBRARIES) == [
        "libhode.so", "libhode_blend.so", "libhode_datagen.so", "libhode_dopri5_pp.so", "libhode_flow.so", "libhode_lstm_seq.so",
        "libhode_mix.so", "libhode_neural_odd.so", "libhode_probe.so", "libhode_real_dims.so", "libhode_real_step.so",
        "libhode_roche_dims.so", "libhode_snf.so", "libhode_sylvester.so"]
    assert list(build_hip.MORE_LIBRARIES) == ["libhode_dose.so"] and list(build_hip.LATER_LIBRARIES) == [LIB]
    assert [r.name for r in build_hip.all_libraries()] == list(build_hip.LIBRARIES) + ["libhode_dose.so"]
    assert [r.name for r in build_hip.every_library()] == list(build_hip.LIBRARIES) + ["libhode_dose.so", LIB]
    assert len(build_hip.every_library()) == 16 == len({r.name for r in build_hip.every_library()})
    assert build_hip.OUT == build_hip.LIBRARIES["libhode.so"].out and build_hip.OBJ == build_hip.LIBRARIES["libhode.so"].obj
    row = build_hip.LATER_LIBRARIES[LIB]
    assert isinstance(row, build_hip.Library) and build_hip.library(LIB) is row
    assert all(build_hip.library(r.name) is r for r in build_hip.every_library())
    with pytest.raises(KeyError):
        build_hip.library("libhode_nothing.so")
    assert row.name == LIB and row.out == os.path.join(ROOT, build_hip.PKG, "hode", LIB)
    assert row.header == "include/hode_real_dose.h" and row.src_dir == build_hip.PKG + "/csrc/real_dose"
    assert row.obj == os.path.join(ROOT, row.src_dir, "build")
    units = [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()]
    assert units[0] == ("hode_real_dose", row.src_dir + "/hode_real_dose.hip", ["-Wno-unused-function"])
    assert units[1:] == [("hode_real_dose_ht%d" % n, row.src_dir + "/hode_real_dose_ht.hip", ["-DHODE_REAL_DOSE_HT=%d" % n])
                         for n in build_hip.REAL_DOSE_HTS]


def test_the_device_code_is_compiled_not_copied():
    """The dose hook is this directory's; the reverse time loop with the rhs, its VJP, the accumulator, the state I/O, the
    dose and the two step macros is hode_real_mf.hpp's real_mf_body, compiled again with the hook and not restated."""
    src = open(os.path.join(build_hip.CSRC, "real_dose", "hode_real_dose_ht.hip")).read()
    for name in ("real_mf_body<HT, METHOD, true, true>(a, RealTileRagged{M}, lds, RealDoseGrad{grad_act})", "RealGradAcc<HT>",
                 "real_grad_fold<HT>", "static constexpr bool kGrad = true;",
                 "__launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))", '#include "../hode_real_mf.hpp"'):
        assert name in src, name
    for restated in ("HODE_REAL_STEP_STAGES(", "HODE_REAL_STEP_CHAIN(", "nn.vjp(", "acc.add(", "real_load_state(", "real_store_state(",
                     "real_set_dose(", "real_dose_table(", "RealMf<", "wave_sum(", "a.partials", "acc.store("):
        assert restated not in src, restated
    assert not re.search(r"for\s*\([^)]*a\.T\b", src)   # no loop over the time grid
    shared = open(os.path.join(build_hip.CSRC, "hode_real_mf.hpp")).read()
    body = shared[shared.index("void real_mf_body("):]
    for name in ("RealMf<HT, Tile>", "real_load_state(", "real_store_state(", "real_set_dose(", "real_dose_table(", "HODE_REAL_STEP_STAGES(",
                 "HODE_REAL_STEP_CHAIN(", "nn.vjp(", "acc.add(", "for (int n = a.T - 2; n >= 0; --n)"):
        assert name in body, name
    # the hook's three calls, compiled out of every kernel without one
    assert body.count("if constexpr (DOSE::kGrad) dose.") == 3 and "static constexpr bool kGrad = false;" in shared
    for call in ("dose.begin(a, p, g0 && live, nn.kel);", "dose.tap(st, q, gX[3]);", "dose.finish();"):
        assert body.count(call) == 1, call
    assert body.index("acc.add(") < body.index("dose.tap(") < body.index("dose.finish()") < body.index("store_state(a.grad_y0")
    for definition in ("struct RealMf", "struct RealGradAcc", "HODE_DEV void real_grad_fold", "HODE_DEV void real_load_state",
                       "HODE_DEV void real_store_state", "HODE_DEV void real_set_dose", "#define HODE_REAL_STEP", "mfma4(",
                       "struct RStageTimes", "HODE_DEV void real_dose_table", "0.375f", "kRealThird", "atomic"):
        assert definition not in src, definition
    host = open(os.path.join(build_hip.CSRC, "real_dose", "hode_real_dose.hip")).read()
    assert "hode_error_state.hpp" in host and "__global__" not in host
    side = open(os.path.join(build_hip.CSRC, "hode_real_side_host.hpp")).read()   # the checks, the layout and the dispatch of the three real_* libraries
    assert "real_side_launch(" in host and "launch_fold_partials(" in side and "__global__" not in side
    files = build_hip.digest_files(LIB)
    for f in ("hode_real_mf.hpp", "hode_real_args.hpp", "hode_common.hpp", "hode_rk_host.hpp", "hode_error_state.hpp", "hode_host.hpp",
              "hode_real_side_host.hpp", "real_dose/hode_real_dose.hpp", "real_dose/hode_real_dose_ht.hip", "real_dose/hode_real_dose.hip"):
        assert build_hip.PKG + "/csrc/" + f in files, f
    assert "include/hode_real_dose.h" in files and "include/hode.h" in files


# ------------------------------------------------------------------------------------------- 2. digest, stamp, loader
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """build_hip.py of a copy of the sources elsewhere.  A test that edits a file of the copy puts it back."""
    tmp = tmp_path_factory.mktemp("tree")
    shutil.copy(os.path.join(ROOT, "build_hip.py"), tmp / "build_hip.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp / "include")
    shutil.copytree(build_hip.CSRC, tmp / build_hip.PKG / "csrc", ignore=shutil.ignore_patterns("build"))
    spec = importlib.util.spec_from_file_location("_build_hip_real_dose_copy", str(tmp / "build_hip.py"))
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
    assert tree.digest(LIB) == before
    # the other libraries' digests do not follow an edit of this library's own files
    own = [f for f in files if "/real_dose/" in f or f.endswith("hode_real_dose.h")]
    assert len(own) == 4
    for name in ("libhode.so", "libhode_real_dims.so", "libhode_real_step.so", "libhode_dose.so"):
        was = tree.digest(name)
        assert _edited(tree, own, lambda: tree.digest(name)) == was, name


def test_library_digest_matches_sources(lib):
    out = build_hip.library(LIB).out
    assert os.path.exists(out + ".digest"), "%s has no source digest: rebuild with `python build_hip.py`" % LIB
    assert open(out + ".digest").read().strip() == build_hip.digest(LIB), "%s is stale: run `python build_hip.py`" % LIB


def test_every_compiled_file_of_the_repository_is_in_the_library_digest():
    row = build_hip.library(LIB)
    hashed = set(build_hip.digest_files(LIB))
    checked = 0
    for unit, src, _ in row.units():
        dfile = os.path.join(row.obj, unit + ".d")
        if not os.path.exists(dfile):
            continue
        deps = {os.path.normpath(x) for x in open(dfile).read().replace("\\\n", " ").split() if not x.endswith(":")}
        tail = os.sep + os.path.relpath(src, ROOT)
        roots = {d[:-len(tail)] for d in deps if d.endswith(tail)}
        assert len(roots) == 1, (unit, sorted(roots))
        root = roots.pop()
        inside = {os.path.relpath(d, root).replace(os.sep, "/") for d in deps if d.startswith(root + os.sep)}
        assert inside and inside <= hashed, (unit, sorted(inside - hashed))
        checked += 1
    if not checked:
        pytest.skip("no depfile is there (library shipped pre-built)")
    assert checked == len(row.units())


def test_a_missing_and_a_stale_library_are_refused_with_a_message(lib, tmp_path, monkeypatch):
    from hode import HodeConfigError
    from hode import _real_dose_lib as DL
    library, out = DL.LIBRARY, build_hip.library(LIB).out
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "directory", str(tmp_path))
    monkeypatch.delenv("HODE_REAL_DOSE_LIBRARY", raising=False)
    with pytest.raises(HodeConfigError, match=r"libhode_real_dose\.so not found -- build it with `python build_hip\.py`.*no CPU fallback for %s"
                       % re.escape(library.noun)):
        library.load()
    shutil.copy(out, tmp_path / LIB)
    (tmp_path / (LIB + ".digest")).write_text("0" * 64 + "\n")
    with pytest.raises(HodeConfigError, match=r"libhode_real_dose\.so is stale .*rebuild with `python build_hip\.py`"):
        library.load()
    shutil.copy(out + ".digest", tmp_path / (LIB + ".digest"))
    assert library.load().hode_real_dose_version() == library.abi_version
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "abi_version", library.abi_version + 1)
    with pytest.raises(HodeConfigError, match=r"libhode_real_dose\.so ABI version 1 != expected 2"):
        library.load()


def test_importing_loads_nothing():
    abi_checks.assert_import_does_not_load(["hode._real_dose_lib"], modules=("hode", "model", "hode.real_dose"))


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
    assert cases.kernels_reached(cases.CASES) == want and len(want) == 12 + 4 + 1


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    assert len(set(map(cases.case_id, cs + cases.ZERO_CASES))) == len(cs) + len(cases.ZERO_CASES) < 40
    assert {(cases.ht(c["H"]), c["method"]) for c in cs if c["grid"] == "unit" and not c["step_size"]} == \
        {(n, m) for n in cases.HTS for m in cases.METHODS}
    assert set(cases.EDGE_D) <= {c["D"] for c in cs} and cases.EDGE_D == (5, 7, 8, 9, 19, 20)
    assert set(cases.EDGE_H) <= {c["H"] for c in cs} and cases.EDGE_H == (1, 16, 17, 43, 64)
    assert set(cases.EDGE_B) <= {c["B"] for c in cs} and cases.EDGE_B == (1, 15, 16, 17, 37)
    for g in ("ragged", "offset+", "offset-"):
        assert sorted(c["method"] for c in cs if c["grid"] == g) == sorted(cases.METHODS), g
    assert sorted((c["step_size"], c["method"]) for c in cs if c["step_size"]) == [(0.5, "midpoint"), (0.5, "rk4")]
    assert all(c["perturb"] == (c["method"] != "euler") for c in cs if c["grid"] == "unit")
    assert all(cases.MIN_LATENT <= c["D"] <= cases.MAX_LATENT and 1 <= c["H"] <= cases.MAX_HIDDEN for c in cs)
    # the six cases the oracle was measured on before any kernel existed
    have = {(c["D"], c["H"], c["B"], c["method"]) for c in cs if c["grid"] == "unit" and not c["step_size"]}
    assert {(5, 1, 17, "euler"), (7, 16, 15, "rk4"), (12, 43, 33, "midpoint"), (19, 64, 37, "rk4"), (20, 43, 37, "midpoint"),
            (10, 32, 1, "rk4")} <= have


def test_case_inputs_hold_what_they_name():
    import real_dims_cases as rd
    import time_grids as tg
    from test_hip_real_dims import _inputs as unit_inputs
    for c in cases.CASES + cases.ZERO_CASES:
        _, p = cases.inputs(c)
        B, D, Ta = c["B"], c["D"], cases.n_action_rows(c)
        assert p["a"].shape == (Ta, B, 1) and p["y0"].shape == (B, D) and p["cot"].shape == (p["t"].numel(), B, D)
        assert p["wflat"].numel() == cases.wflat_len(D, c["H"]) and all(v.dtype == torch.float32 for v in p.values())
        assert bool((p["t"][1:] > p["t"][:-1]).all())
        if c["grid"] == "unit":
            assert Ta == rd.TA == 12 and torch.equal(p["t"], torch.arange(5.0, 12.0))
            if not c["zero"]:  # the inputs of tests/test_hip_real_dims.py, untouched
                assert all(torch.equal(p[k], v) for k, v in unit_inputs(D, c["H"], B)[1].items())
        else:
            assert torch.equal(p["t"], tg.grid(c["grid"], tg.REAL_T)) and Ta == tg.REAL_TA[c["grid"]]
            lo, hi = float(p["t"][0]), float(p["t"][-1])
            assert cases.never_dosed(c) == (hi < 1.0) and (c["grid"] != "offset-" or lo < 0)
            assert c["grid"] != "offset+" or np.floor(hi) > Ta  # stages past the last action row
        if c["zero"]:
            assert not p["a"][:, cases.ZERO_PATIENT].any() and bool(p["a"].any())
        if c["grid"] == "unit" and B > 1:
            assert 0.05 < float((p["a"] != 0).float().mean()) < 0.6


# ------------------------------------------------------------------------------------------ 4. the library's refusals
def _desc(**kw):
    from hode import _real_dose_lib as DL
    d = DL.new_desc()
    d.batch, d.latent_dim, d.hidden_dim, d.n_times, d.n_action_times, d.method = 5, 9, 17, 6, 12, 2
    for k in ("t", "h", "act", "theta", "wflat", "grad_h", "grad_y0", "grad_act", "grad_wflat", "grad_theta", "workspace"):
        setattr(d, k, 4096)  # never dereferenced: every call below is refused before a launch
    d.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, d, code, text):
    assert lib.hode_real_dose_bwd(ctypes.byref(d), None) == code
    assert text in lib.hode_real_dose_last_error_string().decode(), lib.hode_real_dose_last_error_string()


def test_every_argument_error_returns_its_code_without_a_launch(lib):
    for D in (4, 3, 21, 24):
        d = _desc(latent_dim=D)
        _refused(lib, d, E_UNSUPPORTED, "real dose: latent_dim %d has no compiled kernel (have %s)" % (D, SIZES))
        assert lib.hode_real_dose_workspace_bytes(ctypes.byref(d)) == 0
    for H in (0, 65, 80):
        d = _desc(hidden_dim=H)
        _refused(lib, d, E_UNSUPPORTED, "real dose: hidden_dim %d has no compiled kernel (have %s)" % (H, SIZES))
        assert lib.hode_real_dose_workspace_bytes(ctypes.byref(d)) == 0
    for method in (-1, 3, 7):
        _refused(lib, _desc(method=method), E_UNSUPPORTED, "real dose: unknown fixed-grid method %d (have %s)" % (method, SIZES))
    _refused(lib, _desc(flags=4), E_UNSUPPORTED, "real dose: flags 4 have no meaning")
    _refused(lib, _desc(struct_size=8), E_SIZE, "ABI mismatch")
    for field in ("batch", "n_times", "n_action_times"):
        _refused(lib, _desc(**{field: 0}), E_SIZE, "bad sizes: batch=")
    for field in ("t", "h", "act", "theta", "wflat", "grad_h"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "t / h / act (dose table) / theta / wflat (flat weights) / grad_h must be non-NULL")
    for field in ("grad_y0", "grad_act", "grad_wflat", "grad_theta"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "grad_y0 / grad_act / grad_wflat / grad_theta required")
    _refused(lib, _desc(workspace_bytes=64), E_WORKSPACE, "workspace 64 B < required")
    _refused(lib, _desc(workspace=0), E_WORKSPACE, "< required")
    for off in (4, 8):
        _refused(lib, _desc(workspace=4096 + off), E_ALIGN, "workspace must be 16-byte aligned")
    assert lib.hode_real_dose_bwd(None, None) == E_NULL and lib.hode_real_dose_workspace_bytes(None) == 0
    # the layout, restated: per-wave gradient blocks | per-wave rows of the three scalars | the dose table, each rounded up to 256 B
    def al(n):
        return -(-n // 256) * 256
    for B, D, H, Ta in ((5, 9, 17, 12), (37, 20, 64, 3), (1, 5, 1, 1), (1027, 12, 43, 40)):
        waves, n_ht = -(-B // 16), -(-H // 16)
        want = al(waves * ((4 * n_ht + 3) * 256 + 16) * 4) + al(waves * 3 * 4) + al(2 * (Ta + 1) * B * 4)
        assert lib.hode_real_dose_workspace_bytes(ctypes.byref(_desc(batch=B, latent_dim=D, hidden_dim=H, n_action_times=Ta))) == want


# ------------------------------------------------------------------------- 5. the switch, and refusals before a load
@pytest.fixture
def no_library(monkeypatch):
    from hode import _real_dose_lib as DL

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(DL.LIBRARY, "load", boom)
    monkeypatch.setattr(DL, "lib", boom)


def _ode(D=7, H=16, action_dim=1):
    torch.manual_seed(0)
    return model.RocheODEReal(D, action_dim, 3, H, 12, 1, device=CPU)


def _action(Ta=12, B=3, cols=1, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(Ta, B, cols, generator=gen) < 0.3).float() * torch.rand(Ta, B, cols, generator=gen)


T_OUT = torch.arange(5.0, 12.0)


def test_the_config_errors(no_library):
    import hode
    from hode import real_dose
    ode = _ode()
    assert ode.dose_grad is False and "dose_grad" not in dict(ode.named_parameters())
    ode.dose_grad = True
    ode.set_action_static(_action().requires_grad_(True), None)
    y0 = torch.rand(3, 7) * 0.1
    with pytest.raises(hode.HodeConfigError, match=r"RocheODEReal is built for the fixed-grid methods \(euler, midpoint, rk4\); dopri5"):
        hode.odeint(ode, y0, T_OUT, method="dopri5")   # the existing message, kept
    for D, H, got in ((4, 16, "latent dimension 4"), (21, 16, "latent dimension 21"), (24, 9, "latent dimension 24"),
                      (7, 65, "hidden dimension 65"), (20, 80, "hidden dimension 80")):
        ode = _ode(D, H)
        ode.dose_grad = True
        ode.set_action_static(_action().requires_grad_(True), None)
        with pytest.raises(hode.HodeConfigError, match=r"latent dimensions 5 \.\. 20 with hidden_dim 1 \.\. 64 .*\(libhode_real_dose\.so\) \(got %s\)" % got):
            hode.odeint(ode, torch.rand(3, D) * 0.1, T_OUT, method="midpoint")
    with pytest.raises(hode.HodeConfigError, match="5 .. 20"):
        real_dose.check_domain(4, 16)
    with pytest.raises(hode.HodeConfigError, match="1 .. 64"):
        real_dose.check_domain(12, 0)
    real_dose.check_domain(5, 1)
    real_dose.check_domain(20, 64)
    with pytest.raises(hode.HodeConfigError, match="not a fixed-grid method"):
        real_dose.real_dose_backward(torch.zeros(2, 3, 7), None, None, None, None, None, 16, method="dopri5")
    # the one-step-ahead solve: a 3-D init with the switch on and an action that requires grad
    ode = _ode()
    ode.dose_grad = True
    ode.set_action_static(_action().requires_grad_(True), None)
    with pytest.raises(hode.HodeConfigError, match=r"dose_grad serves the chained solve .*one-step-ahead solve \(a 3-D init\) has no dose-table gradient"):
        ode.hode_solve_steps(torch.zeros(6, 3, 7), T_OUT, "midpoint", {})
    # CPU tensors: the solver path's own refusal, from the forward
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        hode.odeint(ode, y0, T_OUT, method="midpoint")


def test_switch_on_reaches_the_function_and_switch_off_does_not(monkeypatch):
    import hode
    from hode import real, real_step
    seen = {"dose": [], "plain": [], "steps": []}

    class Fake:
        @staticmethod
        def apply(y0, theta, wflat, grid, act, hidden, method, perturb):
            seen["dose"].append((method, perturb, hidden, grid.numel(), tuple(act.shape), act.requires_grad, act.detach().clone()))
            return torch.zeros(grid.numel(), *y0.shape)

    def plain(y0, theta, wflat, grid, act, hidden, method="midpoint", perturb=True, lanes_per_patient=0, library=None):
        seen["plain"].append((method, perturb, hidden, grid.numel(), tuple(act.shape), act.requires_grad, library))
        return torch.zeros(grid.numel(), *y0.shape)
    monkeypatch.setattr(model, "_RocheRealDoseGrad", Fake)
    monkeypatch.setattr(real, "real_solve", plain)
    monkeypatch.setattr(real_step, "real_step_solve", lambda init, *a, **kw: seen["steps"].append(kw["method"]) or torch.zeros(init.shape[0] + 1, *init.shape[1:]))
    ode = _ode()
    y0 = torch.rand(3, 7) * 0.1
    a = _action().requires_grad_(True)
    ode.set_action_static(a, None)
    hode.odeint(ode, y0, T_OUT, method="rk4")  # switch off: today's call, whatever the action
    assert seen["dose"] == [] and seen["plain"] == [("rk4", False, 16, 7, (12, 3), True, None)]
    ode.dose_grad = True
    ode.set_action_static(_action(), None)  # an action that needs no gradient: today's call
    hode.odeint(ode, y0, T_OUT, method="midpoint", options={"perturb": True})
    assert seen["dose"] == [] and seen["plain"][1] == ("midpoint", True, 16, 7, (12, 3), False, None)
    ode.hode_solve_steps(torch.zeros(6, 3, 7), T_OUT, "midpoint", {})  # ... and the one-step-ahead solve is served as today
    assert seen["steps"] == ["midpoint"]
    ode.set_action_static(a, None)
    with torch.no_grad():  # no graph, no gradient to ask for: today's call
        hode.odeint(ode, y0, T_OUT, method="euler")
    assert seen["dose"] == [] and len(seen["plain"]) == 3
    assert hode.odeint(ode, y0, T_OUT, method="euler", options={"perturb": True}).shape == (7, 3, 7)
    assert seen["dose"][0][:6] == ("euler", True, 16, 7, (12, 3), True) and torch.equal(seen["dose"][0][6], a.detach()[..., 0])
    h = hode.odeint(ode, y0, T_OUT, method="rk4", options={"step_size": 0.5})  # the solve stays substep's callable
    assert h.shape == (7, 3, 7) and seen["dose"][1][:6] == ("rk4", False, 16, 13, (12, 3), True)
    hode.odeint(ode, y0, T_OUT, method="midpoint", options={"step_size": 1.0})  # the uniform-grid shortcut: the output grid itself
    assert seen["dose"][2][:4] == ("midpoint", False, 16, 7) and len(seen["plain"]) == 3
    # a two-column action is summed before the call, by a torch op: both columns receive the same gradient
    ode2 = _ode(action_dim=2)
    ode2.dose_grad = True
    a2 = _action(cols=2, seed=1).requires_grad_(True)
    ode2.set_action_static(a2, None)
    hode.odeint(ode2, y0, T_OUT, method="midpoint")
    assert seen["dose"][3][4] == (12, 3) and torch.equal(seen["dose"][3][6], a2.detach().sum(-1))
    dose = a2.sum(-1)
    (g,) = torch.autograd.grad((dose * torch.arange(36.0).reshape(12, 3)).sum(), a2)
    assert torch.equal(g[..., 0], g[..., 1])
    assert not hasattr(model.NeuralODE(6, 1, 1.0, 0.1, device=CPU), "dose_grad")


def test_the_autograd_function_lives_next_to_the_module_it_serves():
    """tests/test_binding_case_coverage.py walks hode/*.py: only a launch function there, the Function in model.py."""
    import test_binding_case_coverage as cov
    assert not [b for b in cov.bindings() if b.startswith(("real_dose.", "_real_dose_lib."))]
    assert issubclass(model._RocheRealDoseGrad, torch.autograd.Function)
    assert not cov.pointer_problems()


# ----------------------------------------------------------------------------------- 6. the case table's own error
@pytest.mark.parametrize("c", cases.CASES + cases.ZERO_CASES, ids=cases.case_id)
def test_the_inputs_are_guarded_by_the_oracle_alone(c):
    """Finite; the oracle's own fp32 run within a tenth of the GPU bound of its float64 run; at least half of d loss / d act
    non-zero (exactly zero everywhere on the grid that never reaches hour 1); on the unit grid rows 10 and 11 exactly zero."""
    r64, r32 = cases.oracle(c), cases.oracle(c, torch.float32)
    assert r64["gact"].dtype == torch.float64 and r64["gact"].shape == (cases.n_action_rows(c), c["B"])
    for k in ("h", "gact", "gy0", "gw", "gth"):
        assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
    errs = {k: cases.rel_l2(r32[k], r64[k]) for k in ("gact", "gy0", "gw", "gth")}
    print("%s: fp32 oracle rel-L2 %s; non-zero %.2f" % (cases.case_id(c), ", ".join("%s %.2e" % kv for kv in errs.items()),
                                                         float((r64["gact"] != 0).double().mean())))
    if cases.never_dosed(c):
        assert not r64["gact"].any() and not r32["gact"].any()
        del errs["gact"]
    else:
        assert float((r64["gact"] != 0).double().mean()) >= 0.5
    for k, v in errs.items():
        assert v <= cases.ORACLE_TOL == 1e-5, (k, v)
    if c["grid"] == "unit":
        assert not r64["gact"][10:].any() and not r32["gact"][10:].any() and bool(r64["gact"][:10].any())
    if c["zero"]:
        assert float(r64["gact"][:, cases.ZERO_PATIENT].abs().max()) > 0


@pytest.mark.parametrize("c", cases.CASES + cases.ZERO_CASES, ids=cases.case_id)
def test_the_tap_and_the_reverse_scan_reproduce_the_oracles_gradient(c):
    """The formula, independently of the kernel: the fused (n_cur, R) sweep in numpy, fed the float64 oracle's own stage
    cotangents of KX[3], gives the oracle's autograd gradient of the action to 1e-12."""
    stages, ref = cases.stage_cotangents(c)
    f, _ = cases.inputs(c)
    n_stages = {"euler": 1, "midpoint": 2, "rk4": 4}[c["method"]]
    steps = 12 if c["step_size"] else 6 if c["grid"] == "unit" else 12
    assert len(stages) == n_stages * steps
    ts = [s[0] for s in stages]
    assert ts == sorted(ts)  # the grid is increasing and so are the stage times: the reverse sweep never goes back up
    got = cases.tap_and_scan(stages, float(f.kel.detach()), cases.n_action_rows(c), c["B"])
    want = ref["gact"].numpy()
    if cases.never_dosed(c):
        assert not got.any() and not want.any()
        return
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 1e-12, err
    assert np.array_equal(got == 0, want == 0)
