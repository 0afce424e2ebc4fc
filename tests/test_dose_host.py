"""CPU checks of the dose-gradient path (no GPU): libhode_dose.so's C ABI, its row in build_hip.MORE_LIBRARIES with its
digest, stamp and loader refusals (written here: the helpers of tests/abi_checks.py index build_hip.LIBRARIES directly), the
compiled kernels against the GPU case table (tests/dose_cases.py), the library's own refusals, RocheODE.set_action and the
refusals of RocheODE.dose_grad, and the case table against the oracle's own fp32 error."""
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
import dose_cases as cases
import kernel_variants as kv
import model
import reference_checks as rc

ROOT = build_hip.ROOT
LIB = "libhode_dose.so"
FUNCTIONS = {"hode_dose_" + n for n in ("version", "last_error_string", "workspace_bytes", "bwd")}
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _dose_lib as DL
    if not os.path.exists(DL.LIBRARY.path()):
        build_hip.build(verbose=False)
    return DL.LIBRARY.load()


def test_header_functions_are_exported_and_bound(lib):
    from hode import _dose_lib as DL
    declared = abi_checks.declared_functions("hode_dose.h", "hode_dose_")
    assert declared == {name for name, _, _ in DL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    assert "#define HODE_DOSE_ABI_VERSION %d\n" % DL.HODE_DOSE_ABI_VERSION in abi_checks.header_text("hode_dose.h")
    assert lib.hode_dose_version() == DL.HODE_DOSE_ABI_VERSION
    assert DL.DIMS == build_hip.DP_DIMS == cases.DIMS and DL.METHODS == cases.METHODS
    assert all(str(d) in DL.sizes_text() for d in DL.DIMS) and LIB in DL.sizes_text()
    assert (DL.LIBRARY.file_name, DL.LIBRARY.env, DL.LIBRARY.check_digest) == (LIB, "HODE_DOSE_LIBRARY", True)


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _dose_lib as DL
    abi_checks.assert_c_layout("hode_dose.h", "hode_dose_desc", DL.DoseDesc, tmp_path)
    assert DL.new_desc().struct_size == ctypes.sizeof(DL.DoseDesc)


def test_the_first_table_is_as_it_was_and_the_row_is_in_the_second():
    assert sorted(build_hip.LIBRARIES) == [
        "libhode.so", "libhode_blend.so", "libhode_datagen.so", "libhode_dopri5_pp.so", "libhode_flow.so", "libhode_lstm_seq.so",
        "libhode_mix.so", "libhode_neural_odd.so", "libhode_probe.so", "libhode_real_dims.so", "libhode_real_step.so",
        "libhode_roche_dims.so", "libhode_snf.so", "libhode_sylvester.so"]
    assert list(build_hip.MORE_LIBRARIES) == [LIB] and not set(build_hip.MORE_LIBRARIES) & set(build_hip.LIBRARIES)
    row = build_hip.MORE_LIBRARIES[LIB]
    assert isinstance(row, build_hip.Library) and build_hip.library(LIB) is row
    assert all(build_hip.library(n) is r for n, r in build_hip.LIBRARIES.items())
    assert [r.name for r in build_hip.all_libraries()] == list(build_hip.LIBRARIES) + [LIB]
    with pytest.raises(KeyError):
        build_hip.library("libhode_nothing.so")
    assert row.name == LIB and row.out == os.path.join(ROOT, build_hip.PKG, "hode", LIB)
    assert row.header == "include/hode_dose.h" and row.src_dir == build_hip.PKG + "/csrc/dose" and row.obj == os.path.join(ROOT, row.src_dir, "build")
    units = [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()]
    assert units[0] == ("hode_dose", row.src_dir + "/hode_dose.hip", ["-Wno-unused-function"])
    assert units[1:] == [("hode_dose_d%d" % d, row.src_dir + "/hode_dose_dim.hip", ["-DHODE_DIM=%d" % d]) for d in build_hip.DP_DIMS]


def test_the_device_code_is_compiled_not_copied():
    """The sweep is the fixed-grid adjoint's own, instantiated with the dose hook: the rhs, its VJP, the dose schedule, the
    stage times, the stage algebra, the lane map and the fold are the existing headers' code and are not restated."""
    src = open(os.path.join(build_hip.CSRC, "dose", "hode_dose_kernels.hpp")).read()
    for name in ("rk_bwd_body<D, 1, METHOD, ABLATE,", "DoseSched<", "DoseVal", "LaneMap<1>", "RkArgs", "kGrad = true"):
        assert name in src, name
    for definition in ("HODE_DEV void roche_rhs", "HODE_DEV void roche_vjp", "struct GradAcc", "struct DoseSched", "struct StageTimes",
                       "struct LaneMap", "fold_partials_kernel", "struct RkArgs", "HODE_DEV void rk_bwd_body", "roche_vjp<", "roche_rhs<",
                       "0.375f", "kOneThird", "wave_sum(", "StageTimes st(", "load_vec<", "store_vec<", "GradAcc<"):
        assert definition not in src, definition
    # what the dose header used to name itself is what the shared sweep names
    sweep = open(os.path.join(build_hip.CSRC, "hode_rk_kernels.hpp")).read()
    sweep = sweep[sweep.index("struct NoDoseGrad"):sweep.index("void rk_bwd_kernel")]
    for name in ("roche_rhs<", "roche_vjp<", "GradAcc<", "MlSlice<", "DoseSched<", "load_theta(", "load_dose<", "StageTimes st(",
                 "LaneMap<LPP>", "n_partials<D, LPP>()", "load_vec<D>", "store_vec<D, LPP>", "wave_sum(", "class DOSE = NoDoseGrad"):
        assert name in sweep, name
    assert sweep.count("if constexpr (DOSE::kGrad) dose.tap(") == sweep.count("roche_vjp<") == 7  # every stage VJP is tapped
    assert sweep.count("stage_dose(dose, ds, ") == 5 and sweep.count("ds.at(") == 1  # ... and every stage dose is the hook's (ds.at: stage_dose itself)
    host = open(os.path.join(build_hip.CSRC, "dose", "hode_dose.hip")).read()
    assert "launch_fold_partials(" in host and "patients_per_wave(" in host and "hode_side_error.hpp" in host and "__global__" not in host
    files = build_hip.digest_files(LIB)
    for f in ("hode_roche.hpp", "hode_lanes.hpp", "hode_common.hpp", "hode_rk_kernels.hpp", "hode_rk_host.hpp", "hode_side_error.hpp",
              "dose/hode_dose_kernels.hpp", "dose/hode_dose_dim.hip", "dose/hode_dose.hip"):
        assert build_hip.PKG + "/csrc/" + f in files, f
    assert "include/hode_dose.h" in files and "include/hode.h" in files


# ------------------------------------------------------------------------------------------- 2. digest, stamp, loader
@pytest.fixture(scope="module")
def copy(tmp_path_factory):
    """build_hip.py of a copy of the sources elsewhere.  A test that edits a file of the copy puts it back."""
    tmp = tmp_path_factory.mktemp("tree")
    shutil.copy(os.path.join(ROOT, "build_hip.py"), tmp / "build_hip.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp / "include")
    shutil.copytree(build_hip.CSRC, tmp / build_hip.PKG / "csrc", ignore=shutil.ignore_patterns("build"))
    spec = importlib.util.spec_from_file_location("_build_hip_dose_copy", str(tmp / "build_hip.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert module.ROOT == str(tmp) != ROOT
    return module


def test_digest_follows_an_edit_of_each_of_its_files_and_of_no_other(copy):
    files = copy.digest_files(LIB)
    assert files == build_hip.digest_files(LIB) == sorted(files)
    before = copy.digest(LIB)
    assert before == build_hip.digest(LIB)  # and it does not depend on where the tree lives

    def edited(paths):
        kept = {p: open(os.path.join(copy.ROOT, p), "rb").read() for p in paths}
        try:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text + b"\n")
            return copy.digest(LIB)
        finally:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text)

    for f in files:
        assert edited([f]) != before, f
    others = [os.path.relpath(os.path.join(d, f), copy.ROOT).replace(os.sep, "/")
              for top in ("include", build_hip.PKG) for d, _, fs in os.walk(os.path.join(copy.ROOT, top)) for f in fs]
    others = sorted(set(others) - set(files))
    assert others and edited(others) == before
    assert copy.digest(LIB) == before
    # the other libraries' digests do not follow an edit of this library's own files
    own = [f for f in files if "/dose/" in f or f.endswith("hode_dose.h")]
    assert len(own) == 4
    for name in ("libhode.so", "libhode_dopri5_pp.so", "libhode_roche_dims.so"):
        was = copy.digest(name)
        kept = {p: open(os.path.join(copy.ROOT, p), "rb").read() for p in own}
        try:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text + b"\n")
            assert copy.digest(name) == was, name
        finally:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text)


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
    from hode import _dose_lib as DL
    library, out = DL.LIBRARY, build_hip.library(LIB).out
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "directory", str(tmp_path))
    monkeypatch.delenv("HODE_DOSE_LIBRARY", raising=False)
    with pytest.raises(HodeConfigError, match=r"libhode_dose\.so not found -- build it with `python build_hip\.py`.*no CPU fallback for %s"
                       % re.escape(library.noun)):
        library.load()
    shutil.copy(out, tmp_path / LIB)
    (tmp_path / (LIB + ".digest")).write_text("0" * 64 + "\n")
    with pytest.raises(HodeConfigError, match=r"libhode_dose\.so is stale .*rebuild with `python build_hip\.py`"):
        library.load()
    shutil.copy(out + ".digest", tmp_path / (LIB + ".digest"))
    assert library.load().hode_dose_version() == library.abi_version


def test_importing_loads_nothing():
    abi_checks.assert_import_does_not_load(["hode._dose_lib"], modules=("hode", "model", "hode.dose"))


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
    want = cases.all_kernels() | {"hode::fold_partials_kernel"}
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert {cases.kernel(c) for c in cases.CASES} == cases.all_kernels() and len(cases.all_kernels()) == 48


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    assert len(set(map(cases.case_id, cs))) == len(cs) < 80
    assert {c["D"] for c in cs} == set(cases.DIMS) and {c["method"] for c in cs} == set(cases.METHODS)
    assert {c["B"] for c in cs} == {5, 63, 64, 65, 130, 16, cases.TWO_PER_WAVE} and {c["K"] for c in cs} == {1, 2, 3}
    assert {c["T"] for c in cs} == {1, 2, 9, 12} and min(c["B"] for c in cs) >= 5
    assert {cases.body(c) for c in cs} == {(True, True), (True, False), (False, False)}
    for D in cases.DIMS:  # every body, perturb, ablate and the sweep without the expert gradient at every size
        on = [c for c in cs if c["D"] == D]
        assert {cases.body(c) for c in on} == {(True, True), (True, False), (False, False)}, D
        assert any(c["perturb"] for c in on) and any(c["ablate"] for c in on) and any(not c["need_theta"] for c in on), D
        assert any(c["grid"] != "uniform" for c in on) and any(c["edge"] for c in on), D
    assert {c["grid"] for c in cs} == {"uniform", "offset+", "offset-", "clustered"}
    assert {c["method"] for c in cs if c["edge"]} == set(cases.METHODS) and not any(c["perturb"] for c in cs if c["edge"])
    # the host's grid rule, restated: two patients per wave from 1025 on, the last wave partly filled
    simds = 1024
    assert -(-cases.TWO_PER_WAVE // simds) == 2 and cases.TWO_PER_WAVE % 2 == 1 and -(-130 // simds) == 1


def test_case_inputs_hold_what_they_name():
    import time_grids as tg
    for c in cases.CASES:
        p = cases.setup(c)
        B, T, K = c["B"], c["T"], c["K"]
        assert p["y0"].shape == (B, c["D"]) and p["t"].shape == (T,) and p["times"].shape == (B, K) and p["dosage"].shape == (B,)
        assert p["cot"].shape == (T, B, c["D"]) and all(v.dtype == torch.float32 for v in (p["y0"], p["t"], p["times"], p["dosage"]))
        assert bool((p["t"][1:] > p["t"][:-1]).all())
        assert p["f"].ablate == c["ablate"] and (float(p["f"].HillCure.detach()) == 2.0) == (c["hill"] == "two")
        z, late = cases.zero_row(c), cases.late_row(c)
        assert float(p["dosage"][z]) == 0.0 and bool((p["times"][late] > p["t"][-1]).all())
        assert int((p["dosage"] == 0).sum()) == 1
        if c["grid"] != "uniform":
            assert torch.equal(p["t"], tg.grid(c["grid"], T))
        if c["edge"]:
            t0 = p["t"][3]
            first = p["times"][:, 0]
            assert first[0] == t0 and first[1] == torch.nextafter(t0, t0 + 1) and first[2] == torch.nextafter(t0, t0 - 1)
            stages = torch.tensor(tg.stage_times32(p["t"].numpy(), c["method"], False)[3])
            if c["method"] == "midpoint":
                assert first[3] == stages[1] == t0 + 0.0625 and first[4] > stages[1] > first[5]
            if c["method"] == "rk4":
                assert first[3] == torch.nextafter(stages[1], stages[1] + 1) and first[6] == torch.nextafter(stages[2], stages[2] - 1)


# ------------------------------------------------------------------------------------------ 4. the library's refusals
def _desc(**kw):
    from hode import _dose_lib as DL
    d = DL.new_desc()
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.method = 5, 8, 6, 1, 2
    for k in ("t", "h", "dosage", "dose_times", "theta", "w1", "b1", "grad_h", "grad_y0", "grad_dosage", "grad_w1", "grad_b1",
              "grad_theta", "workspace"):
        setattr(d, k, 4096)  # never dereferenced: every call below is refused before a launch
    d.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, d, code, text):
    assert lib.hode_dose_bwd(ctypes.byref(d), None) == code
    assert text in lib.hode_dose_last_error_string().decode(), lib.hode_dose_last_error_string()


def test_every_argument_error_returns_its_code_without_a_launch(lib):
    for D in (5, 7, 10, 16, 20, 3):
        d = _desc(latent_dim=D)
        _refused(lib, d, E_UNSUPPORTED, "latent_dim %d has no compiled kernel (have latent_dim 4, 6, 8, 12" % D)
        assert lib.hode_dose_workspace_bytes(ctypes.byref(d)) == 0
    for kind in (2, 3, 4, 5):
        _refused(lib, _desc(rhs_kind=kind), E_UNSUPPORTED, "rhs_kind %d is not served here (have latent_dim 4, 6, 8, 12" % kind)
    for method in (-1, 3):
        _refused(lib, _desc(method=method), E_UNSUPPORTED, "unknown fixed-grid method %d (have latent_dim 4, 6, 8, 12" % method)
    _refused(lib, _desc(struct_size=8), E_SIZE, "ABI mismatch")
    for field in ("batch", "n_times", "n_dose"):
        _refused(lib, _desc(**{field: 0}), E_SIZE, "bad sizes: batch=")
    _refused(lib, _desc(flags=4), E_UNSUPPORTED, "flags 4")
    for field in ("t", "h", "dosage", "dose_times", "theta"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "t / h / dosage / dose_times / theta must be non-NULL")
    _refused(lib, _desc(w1=0), E_NULL, "w1 / b1 required")
    for field in ("grad_h", "grad_y0", "grad_dosage"):
        _refused(lib, _desc(**{field: 0}), E_NULL, "grad_h / grad_y0 / grad_dosage required")
    _refused(lib, _desc(grad_b1=0), E_NULL, "grad_w1 / grad_b1 required")
    _refused(lib, _desc(need_theta_grad=1, grad_theta=0), E_NULL, "grad_theta required")
    for field in ("h", "grad_h", "grad_y0"):  # check_rk's alignment refusals: float4 rows where D % 4 == 0 ...
        for off in (4, 8):
            _refused(lib, _desc(**{field: 4096 + off}), E_ALIGN, "h / grad_h / grad_y0 must be 16-byte aligned (latent_dim 8)")
        d = _desc(latent_dim=6, workspace_bytes=0, **{field: 4100})  # ... and none where the rows are read as dwords
        _refused(lib, d, E_WORKSPACE, "workspace 0 B < required")
    _refused(lib, _desc(workspace_bytes=0), E_WORKSPACE, "workspace 0 B < required 1024 B (batch=5 latent_dim=8)")
    _refused(lib, _desc(workspace=0), E_WORKSPACE, "< required")
    assert lib.hode_dose_bwd(None, None) == E_NULL
    # the size the refusal names: [waves][partials] floats, a wave per patient up to 1024 patients, rounded up to 256 bytes
    for B, D, waves in ((5, 8, 5), (130, 12, 130), (1027, 4, 514), (1, 6, 1)):
        P = (D - 4) * D + (D - 4) + 15
        assert lib.hode_dose_workspace_bytes(ctypes.byref(_desc(batch=B, latent_dim=D))) == -(-waves * P * 4 // 256) * 256


# ------------------------------------------------------------------------- 5. refusals before anything is loaded
@pytest.fixture
def no_library(monkeypatch):
    from hode import _dose_lib as DL

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(DL.LIBRARY, "load", boom)
    monkeypatch.setattr(DL, "lib", boom)


def _action(T=11, B=3, K=2, equal=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = torch.zeros(T, B, 1)
    for p in range(B):
        idx = torch.randperm(T - 1, generator=gen)[:K]
        a[idx, p, 0] = 2.5 if equal else torch.rand(K, generator=gen) + 0.5
    return a


def _ode(D=6, cls=model.RocheODE, **kw):
    torch.manual_seed(0)
    return cls(D, 1, 1.0, 0.1, device=CPU, **kw)


def test_the_two_config_errors(no_library):
    import hode
    from hode import dose
    ode = _ode(6)
    assert ode.dose_grad is False
    ode.dose_grad = True
    ode.set_action(_action().requires_grad_(True))
    y0, t = torch.rand(3, 6) * 0.01, torch.arange(11, dtype=torch.float32) * 0.1
    for options in ({}, {"step_control": "batch"}, {"step_control": "patient"}):
        with pytest.raises(hode.HodeConfigError, match=r"dose_grad serves the fixed-grid methods euler / midpoint / rk4.*dopri5"):
            hode.odeint(ode, y0, t, method="dopri5", options=options)
    for D in (5, 7, 16, 20):
        ode = _ode(D)
        ode.dose_grad = True
        ode.set_action(_action().requires_grad_(True))
        with pytest.raises(hode.HodeConfigError, match=r"latent dimensions 4, 6, 8, 12 .*\(libhode_dose\.so\) \(got latent dimension %d\)" % D):
            hode.odeint(ode, torch.rand(3, D) * 0.01, t, method="rk4")
    with pytest.raises(hode.HodeConfigError, match="4, 6, 8, 12"):
        dose.check_domain(5)
    with pytest.raises(hode.HodeConfigError, match="at least one dose"):
        dose.check_domain(8, 0)
    dose.check_domain(12, 3)
    with pytest.raises(hode.HodeConfigError, match="not a fixed-grid method"):
        dose.dose_backward(torch.zeros(2, 3, 4), None, None, None, None, None, None, None, method="dopri5")
    # CPU tensors: the solver path's own refusal, from the forward
    ode = _ode(6)
    ode.dose_grad = True
    ode.set_action(_action().requires_grad_(True))
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        hode.odeint(ode, y0, t, method="rk4")


def test_switch_on_reaches_the_function_and_switch_off_does_not(monkeypatch):
    import hode
    seen = {"dose": [], "plain": []}

    class Fake:
        @staticmethod
        def apply(y0, theta, w, b, grid, dosage, times, method, ablate, perturb, check_finite, library):
            seen["dose"].append((method, perturb, grid.numel(), dosage.requires_grad, tuple(times.shape)))
            return torch.zeros(grid.numel(), *y0.shape)
    monkeypatch.setattr(model, "_RocheDoseGrad", Fake)
    monkeypatch.setattr(hode, "roche_solve", lambda *a, **kw: seen["plain"].append(kw["method"]) or torch.zeros(a[4].numel(), *a[0].shape))
    ode = _ode(6)
    y0, t = torch.rand(3, 6) * 0.01, torch.arange(11, dtype=torch.float32) * 0.1
    a = _action().requires_grad_(True)
    ode.set_action(a)
    hode.odeint(ode, y0, t, method="rk4")  # switch off: today's path, whatever the action
    assert seen == {"dose": [], "plain": ["rk4"]}
    ode.dose_grad = True
    ode.set_action(_action())  # an action that needs no gradient: today's path
    hode.odeint(ode, y0, t, method="midpoint")
    assert seen == {"dose": [], "plain": ["rk4", "midpoint"]}
    ode.set_action(a)
    assert hode.odeint(ode, y0, t, method="euler", options={"perturb": True}).shape == (11, 3, 6)
    h = hode.odeint(ode, y0, t, method="rk4", options={"step_size": 0.05})  # the solve stays substep's callable
    assert h.shape == (11, 3, 6)
    assert seen["dose"][0] == ("euler", True, 11, True, (3, 2)) and len(seen["dose"]) == 2 and len(seen["plain"]) == 2
    method, perturb, n_grid, needs_grad, shape = seen["dose"][1]
    assert (method, perturb, needs_grad, shape) == ("rk4", False, True, (3, 2)) and n_grid >= 21
    assert not hasattr(model.NeuralODE(6, 1, 1.0, 0.1, device=CPU), "dose_grad")


def test_the_autograd_function_lives_next_to_the_module_it_serves():
    """tests/test_binding_case_coverage.py walks hode/*.py: only a launch function there, the Function in model.py."""
    import test_binding_case_coverage as cov
    assert not [b for b in cov.bindings() if b.startswith(("dose.", "_dose_lib."))]
    assert issubclass(model._RocheDoseGrad, torch.autograd.Function)
    assert not cov.pointer_problems()


# -------------------------------------------------------------------------------------------------- 6. set_action
def _today(action, step_size):
    """What set_action gives today (the parent commit's lines)."""
    from hode.solver import dose_schedule_index
    dosage, idx = dose_schedule_index(action)
    return dosage, idx * step_size


@pytest.mark.parametrize("equal", [False, True])
def test_set_action_with_the_switch_on_routes_the_gradient_to_one_entry_per_patient(equal):
    from hode.solver import dose_schedule_index
    plain = _action(equal=equal)
    want_d, want_t = _today(plain, 0.1)
    for route in ("computed", "attached", "cached"):
        ode = _ode(6)
        ode.dose_grad = True
        a = plain.clone().requires_grad_(True)
        if route == "attached":  # the attached schedule may supply the indices, never the dosage
            a.hode_schedule = (torch.full_like(want_d, 7.0), dose_schedule_index(plain)[1])
        if route == "cached":
            ode.set_action(a)
            assert ode._schedule_cache[0] is a and not ode._schedule_cache[2].requires_grad
        ode.set_action(a)
        assert ode.dosage.requires_grad and torch.equal(ode.dosage.detach(), want_d) and torch.equal(ode.times, want_t), route
        (g,) = torch.autograd.grad(ode.dosage.sum(), a)
        assert g.shape == a.shape and bool(((g == 0) | (g == 1)).all()), route
        assert torch.equal(g[..., 0].sum(0), torch.ones(3)), route  # one-hot per patient, also among equal doses
        hot = g[..., 0].argmax(dim=0)
        assert torch.equal(a.detach()[hot, torch.arange(3), 0], want_d), route  # on an entry that holds the maximum
        assert not ode.times.requires_grad


def test_set_action_with_the_switch_off_is_bit_for_bit_todays():
    from hode.solver import dose_schedule_index
    plain = _action(seed=3)
    want_d, want_t = _today(plain, 0.1)
    for needs_grad in (False, True):
        for cls in (model.RocheODE, model.NeuralODE):
            ode = _ode(6, cls=cls)
            a = plain.clone().requires_grad_(needs_grad)
            ode.set_action(a)
            assert torch.equal(ode.dosage, want_d) and torch.equal(ode.times, want_t) and ode.dosage.requires_grad == needs_grad
            assert ode._schedule_cache[2] is ode.dosage  # the cache holds the very tensor, as today
            ode.set_action(a)  # the cache route
            assert torch.equal(ode.dosage, want_d) and torch.equal(ode.times, want_t) and ode.dosage is ode._schedule_cache[2]
            b = plain.clone().requires_grad_(needs_grad)
            attached = (torch.full_like(want_d, 7.0), dose_schedule_index(plain)[1])
            b.hode_schedule = attached
            ode.set_action(b)  # the attached route: the dosage is the attached one
            assert ode.dosage is attached[0] and torch.equal(ode.times, want_t)
    # switch on, but an action that needs no gradient: today's too
    ode = _ode(6)
    ode.dose_grad = True
    a = plain.clone()
    ode.set_action(a)
    assert torch.equal(ode.dosage, want_d) and not ode.dosage.requires_grad and ode._schedule_cache[2] is ode.dosage


# ----------------------------------------------------------------------------------- 7. the case table's own error
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_the_fp32_oracle_stays_a_tenth_of_the_bound_from_float64(c):
    """The inputs themselves stay inside the bound: the oracle's own fp32 run is within GRAD_TOL / 10 rel-L2 of its float64
    run for the dose gradient, which is not 0 (under ablate, and with a single output time, it is exactly 0 in both)."""
    r64, r32 = cases.oracle(c), cases.oracle(c, torch.float32)
    for k in ("gy0", "gdosage", "gw", "gb") + (("gth",) if c["need_theta"] else ()):  # what the GPU test compares
        assert k not in r64 or (bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all())), k
    g64 = r64["gdosage"]
    assert g64.dtype == torch.float64 and bool(torch.isfinite(g64).all())
    if c["ablate"] or c["T"] == 1:
        assert not g64.any() and not r32["gdosage"].any()
        return
    assert float(g64.norm()) > 0 and float(g64[cases.zero_row(c)].abs()) > 0 and float(g64[cases.late_row(c)]) == 0.0
    err = cases.rel_l2(r32["gdosage"], g64)
    print("%s: fp32 oracle rel-L2 %.3e" % (cases.case_id(c), err))
    assert err <= rc.GRAD_TOL / 10, err
    # the other gradients the GPU test holds to GRAD_TOL: finite in both, and the fp32 oracle inside the bound itself
    for k in ("gy0", "gw", "gb") + (("gth",) if c["need_theta"] else ()):
        if k in r64 and float(r64[k].norm()) > 0:
            assert bool(torch.isfinite(r32[k]).all()) and cases.rel_l2(r32[k], r64[k]) <= rc.GRAD_TOL, (k, cases.rel_l2(r32[k], r64[k]))
