"""CPU checks of the per-patient dopri5 path (no GPU): libhode_dopri5_pp.so's C ABI and build-table row,
the compiled kernels against the GPU case table (tests/dopri5_pp_cases.py), the library's own refusals, the
refusals that happen before anything is loaded, and the dispatch from hode.odeint / model.RocheODE.step_control."""
import copy
import ctypes
import functools
import glob
import os
import sys

import pytest
import torch

import abi_checks
import build_hip
import dopri5_pp_audit as audit
import dopri5_pp_cases as cases
import kernel_variants as kv
import model

ROOT = build_hip.ROOT
LIB = "libhode_dopri5_pp.so"
FUNCTIONS = {"hode_dopri5_pp_" + n for n in ("version", "last_error_string", "workspace_bytes", "fwd", "bwd", "tape_offsets")}
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _dopri5_pp_lib as PL
    return abi_checks.built(PL.LIBRARY)


def test_header_functions_are_exported_and_bound(lib):
    from hode import _dopri5_pp_lib as PL
    declared = abi_checks.declared_functions("hode_dopri5_pp.h", "hode_dopri5_pp_")
    assert declared == {name for name, _, _ in PL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_dopri5_pp.h")
    assert "#define HODE_DOPRI5_PP_ABI_VERSION %d\n" % PL.HODE_DOPRI5_PP_ABI_VERSION in src
    assert lib.hode_dopri5_pp_version() == PL.HODE_DOPRI5_PP_ABI_VERSION
    assert PL.DIMS == build_hip.DP_DIMS == cases.DIMS
    assert all(str(d) in PL.sizes_text() for d in PL.DIMS) and LIB in PL.sizes_text()


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _dopri5_pp_lib as PL
    abi_checks.assert_c_layout("hode_dopri5_pp.h", "hode_dopri5_pp_desc", PL.PpDesc, tmp_path)
    assert PL.new_desc().struct_size == ctypes.sizeof(PL.PpDesc)


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_dopri5_pp.h" and row.src_dir == build_hip.PKG + "/csrc/dopri5_pp"
    units = [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()]
    assert units[0] == ("hode_dopri5_pp", row.src_dir + "/hode_dopri5_pp.hip", ["-Wno-unused-function"])
    # one compile unit per latent size
    assert units[1:] == [("hode_dopri5_pp_d%d" % d, row.src_dir + "/hode_dopri5_pp_dim.hip", ["-DHODE_DIM=%d" % d]) for d in build_hip.DP_DIMS]
    from hode import _dopri5_pp_lib as PL
    assert PL.LIBRARY.noun == "the dopri5 solve with per-patient step control"   # what the loader says has no CPU fallback


def test_the_device_code_is_compiled_not_copied():
    """The rhs, its VJP, the stages, the step factor, the tableau and the partial rows are the existing headers' own."""
    src = open(os.path.join(build_hip.CSRC, "dopri5_pp", "hode_dopri5_pp_kernels.hpp")).read()
    for name in ("roche_rhs<", "roche_vjp<", "GradAcc<", "MlSlice<", "DoseSched<", "load_theta(", "dp_stages<", "dp_step_factor(",
                 "store_grad_partials<", "load_dose<", "kDpErr[", "kDpMid[", "kDpBeta[", "LaneMap<1>"):
        assert name in src, name
    for definition in ("HODE_DEV void roche_rhs", "HODE_DEV void roche_vjp", "HODE_DEV void dp_stages", "HODE_DEV double dp_step_factor",
                       "constexpr float kDp", "struct GradAcc", "HODE_DEV void store_grad_partials", "DoseSched<K1> load_dose(", "dp_store_grad_partials", "dp_load_dose",
                       "pp_load_dose", "fold_partials_kernel"):
        assert definition not in src, definition
    host = open(os.path.join(build_hip.CSRC, "dopri5_pp", "hode_dopri5_pp.hip")).read()
    assert "launch_fold_partials(" in host and "hode_side_error.hpp" in host and "__global__" not in host


# ---------------------------------------------------------------------------------- 2. compiled kernels / case table
def _objects():
    objs = sorted(glob.glob(os.path.join(build_hip.LIBRARIES[LIB].obj, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    return [(dem, kd) for o in objs for dem, kd in kernel_descriptors(o)]


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    compiled = {kv.kernel_name(dem) for dem, _ in _objects()}
    want = cases.all_kernels() | {"hode::fold_partials_kernel"}
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert set().union(*(cases.kernels(c) for c in cases.CASES)) == cases.all_kernels()
    assert set().union(*(cases.kernels(c) for c in cases.CASES + cases.GRID_CASES)) == cases.all_kernels()
    assert len(cases.all_kernels()) == 24


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    assert {c["D"] for c in cs} == set(cases.DIMS) and {c["B"] for c in cs} == {1, 3, 21, 70}
    assert {c["K"] for c in cs} == {1, 2} and {c["ablate"] for c in cs} == {False, True}
    ts = {c["T"] for c in cs}
    assert 1 in ts and 2 in ts and 20 in ts and max(ts) == 20
    assert any(c["D"] == 12 and c["B"] == 70 and c["T"] == 20 for c in cs)
    # every rhs body -- (Hill exponents == 2, one dose), (== 2, dose list), general -- at more than one size, both ways
    assert {cases.bodies(c) for c in cs} == {(True, True), (True, False), (False, False)}
    assert len({c["D"] for c in cs if cases.bodies(c) == (False, False)}) >= 3
    assert len(set(map(cases.case_id, cs))) == len(cs) < 30
    assert all(len(cases.subset(c["B"])) <= 5 for c in cs) and cases.subset(70) == [0, 23, 63, 64, 69] and cases.subset(3) == [0, 1, 2]


def test_case_inputs_have_the_doses_they_name():
    from oracle.rhs import dose_schedule
    for c in cases.CASES:
        inp, f = cases.setup(c)
        dosage, times = dose_schedule(inp["actions"], f.step_size)
        assert inp["z0"].shape == (c["B"], c["D"]) and inp["t"].numel() == c["T"] and times.shape == (c["B"], c["K"]), cases.case_id(c)
        assert f.ablate == c["ablate"] and (float(f.HillCure) == 2.0) == (c["hill"] == "two")


# ------------------------------------------------------------------------------------------ 3. the library's refusals
def _desc(lib, **kw):
    from hode import _dopri5_pp_lib as PL
    d = PL.new_desc()
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.max_steps, d.rtol, d.atol = 5, 8, 6, 1, 40, 1e-7, 1e-8
    for k in ("t", "y0", "dosage", "dose_times", "theta", "w1", "b1", "h", "status", "n_accepted", "n_rejected", "patient_status"):
        setattr(d, k, 4096)  # never dereferenced: every call below is refused before a launch
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, d, code, text, bwd=False):
    fn = lib.hode_dopri5_pp_bwd if bwd else lib.hode_dopri5_pp_fwd
    assert fn(ctypes.byref(d), None) == code
    assert text in lib.hode_dopri5_pp_last_error_string().decode(), lib.hode_dopri5_pp_last_error_string()


def test_the_library_refuses_what_it_does_not_hold(lib):
    for D in (5, 7, 10, 16, 20, 3):
        d = _desc(lib, latent_dim=D)
        _refused(lib, d, E_UNSUPPORTED, "latent_dim %d has no compiled kernel (have latent_dim 4, 6, 8, 12" % D)
        assert lib.hode_dopri5_pp_workspace_bytes(ctypes.byref(d)) == 0
    for kind in (2, 3, 4, 5):
        _refused(lib, _desc(lib, rhs_kind=kind), E_UNSUPPORTED, "rhs_kind %d is not served here" % kind)
    _refused(lib, _desc(lib, struct_size=8), E_SIZE, "ABI mismatch")
    for field in ("batch", "n_times", "n_dose", "max_steps"):
        _refused(lib, _desc(lib, **{field: 0}), E_SIZE, "bad sizes")
    _refused(lib, _desc(lib, max_attempts=-1), E_SIZE, "bad sizes")
    _refused(lib, _desc(lib, flags=8), E_UNSUPPORTED, "flags 8")
    _refused(lib, _desc(lib, rtol=0.0), E_SIZE, "rtol must be > 0")
    _refused(lib, _desc(lib, h=0), E_NULL, "must be non-NULL")
    _refused(lib, _desc(lib, w1=0), E_NULL, "w1 / b1 required")
    _refused(lib, _desc(lib, patient_status=0), E_NULL, "patient_status")
    _refused(lib, _desc(lib, y0=4100), E_ALIGN, "16-byte aligned")
    _refused(lib, _desc(lib), E_WORKSPACE, "workspace 0 B < required")
    _refused(lib, _desc(lib), E_NULL, "grad_h / grad_y0 required", bwd=True)
    d = _desc(lib, flags=16, grad_h=4096, grad_y0=4096, grad_w1=4096, grad_b1=4096)
    _refused(lib, d, E_UNSUPPORTED, "no tape to sweep", bwd=True)
    assert lib.hode_dopri5_pp_fwd(None, None) == E_NULL


def test_workspace_layout(lib):
    """The tape is [max_steps][B] per array behind the per-wave partial rows; without a tape the partials alone, whatever
    the step bound."""
    d = _desc(lib, batch=70, latent_dim=12, max_steps=100)
    off = (ctypes.c_size_t * 5)()
    assert lib.hode_dopri5_pp_tape_offsets(ctypes.byref(d), off) == 0
    cells = 100 * 70
    partials = 2 * (8 * 12 + 8 + 15) * 4
    assert off[0] == 0 and off[1] >= partials and off[2] - off[1] >= 8 * cells and off[3] - off[2] >= 8 * cells
    assert off[4] - off[3] >= 8 * cells and all(o % 256 == 0 for o in off)
    total = lib.hode_dopri5_pp_workspace_bytes(ctypes.byref(d))
    assert off[4] + cells * 12 * 4 <= total < off[4] + cells * 12 * 4 + 256
    d.flags = 16
    small = lib.hode_dopri5_pp_workspace_bytes(ctypes.byref(d))
    d.max_steps = 1 << 20
    assert lib.hode_dopri5_pp_workspace_bytes(ctypes.byref(d)) == small < 2048


# ------------------------------------------------------------------------- 4. refusals before anything is loaded
@pytest.fixture
def no_library(monkeypatch):
    from hode import _dopri5_pp_lib as PL

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(PL.LIBRARY, "load", boom)
    monkeypatch.setattr(PL, "lib", boom)


def _ode(D=6, cls=model.RocheODE, **kw):
    torch.manual_seed(0)
    ode = cls(D, 1, 1.0, 0.1, device=CPU, **kw)
    a = torch.zeros(11, 3, 1)
    a[2, :, 0] = 1.0
    ode.set_action(a)
    return ode, torch.rand(3, D) * 0.01, torch.arange(11, dtype=torch.float32) * 0.1


def test_unsupported_sizes_are_refused_naming_the_sizes_held(no_library):
    import hode
    from hode import patient_dopri5
    for D in (5, 7, 16, 20):
        ode, y0, t = _ode(D)
        ode.step_control = "patient"
        with pytest.raises(hode.HodeConfigError, match=r"latent dimensions 4, 6, 8, 12 \(libhode_dopri5_pp\.so\) \(got latent dimension %d\)" % D):
            hode.odeint(ode, y0, t, method="dopri5")
    with pytest.raises(hode.HodeConfigError, match="4, 6, 8, 12"):
        patient_dopri5.check_domain(5)
    with pytest.raises(hode.HodeConfigError, match="at least one dose"):
        patient_dopri5.check_domain(8, 0)
    patient_dopri5.check_domain(12, 3)


def test_cpu_tensors_are_refused(no_library):
    import hode
    ode, y0, t = _ode(6)
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        hode.odeint(ode, y0, t, method="dopri5", options={"step_control": "patient"})
    ode.step_control = "patient"
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        hode.odeint(ode, y0, t, method="dopri5")


def test_a_bad_step_control_is_refused(no_library):
    import hode
    ode, y0, t = _ode(6)
    for bad in ("Patient", "per-patient", "", None, 1):
        with pytest.raises(hode.HodeConfigError, match="step_control .* is not one of 'batch', 'patient'"):
            hode.odeint(ode, y0, t, method="dopri5", options={"step_control": bad})
        ode.step_control = bad
        with pytest.raises(hode.HodeConfigError, match="is not one of"):
            hode.odeint(ode, y0, t, method="rk4")
        ode.step_control = "batch"
    assert model.STEP_CONTROLS == ("batch", "patient") and model.RocheODE(4, 1, 1.0, 0.1, device=CPU).step_control == "batch"


def test_the_other_rhs_families_name_what_serves_it(no_library):
    import hode
    ode, y0, t = _ode(6, cls=model.NeuralODE)
    for method in ("dopri5", "rk4"):
        with pytest.raises(hode.HodeConfigError, match=r"NeuralODE has no per-patient step control.*RocheODE.*4, 6, 8, 12"):
            hode.odeint(ode, y0, t, method=method, options={"step_control": "patient"})
    ode.step_control = "patient"
    with pytest.raises(hode.HodeConfigError, match="NeuralODE has no per-patient step control"):
        hode.odeint(ode, y0, t, method="dopri5")
    real = model.RocheODEReal(6, 1, 1, 8, 4.0, 1.0, device=CPU)
    real.set_action_static(torch.zeros(4, 3, 1), None)
    with pytest.raises(hode.HodeConfigError, match="RocheODEReal has no per-patient step control"):
        real.hode_solve(torch.zeros(3, 6), torch.arange(3.0), 1e-7, 1e-8, "midpoint", {"step_control": "patient"})


# ----------------------------------------------------------------------------------------------------- 5. dispatch
def test_step_control_patient_reaches_the_launch_function_and_the_default_does_not(monkeypatch):
    import hode
    from hode import adaptive, patient_dopri5
    calls = {"patient": [], "batch": 0}

    def fake_forward(y0, theta, w, b, t, dosage, dose_times, **kw):
        calls["patient"].append(kw)
        B, D = y0.shape
        return torch.zeros(t.numel(), B, D), torch.zeros(4, dtype=torch.int32), {"n_accepted": torch.zeros(B, dtype=torch.int32), "max_steps": 7}

    def fake_batch(y0, *a, **kw):
        calls["batch"] += 1
        return torch.zeros(11, *y0.shape)
    monkeypatch.setattr(patient_dopri5, "patient_dopri5_forward", fake_forward)
    monkeypatch.setattr(adaptive, "roche_dopri5", fake_batch)
    ode, y0, t = _ode(6)
    hode.odeint(ode, y0, t, method="dopri5")
    hode.odeint(ode, y0, t, method="dopri5", options={"step_control": "batch"})
    assert calls["batch"] == 2 and not calls["patient"]
    h = hode.odeint(ode, y0, t, rtol=1e-7, atol=1e-8, method="dopri5", options={"step_control": "patient"})
    assert h.shape == (11, 3, 6) and calls["batch"] == 2 and len(calls["patient"]) == 1
    kw = calls["patient"][0]
    assert kw["rtol"] == 1e-7 and kw["atol"] == 1e-8 and kw["ablate"] is False and kw["no_tape"] is False  # parameters need gradients
    ode.step_control = "patient"
    with torch.no_grad():
        hode.odeint(ode, y0, t)  # dopri5 is odeint's default method
    assert len(calls["patient"]) == 2 and calls["patient"][1]["no_tape"] is True  # grad mode sampled by the caller
    hode.odeint(ode, y0, t, options={"step_control": "batch"})  # the option overrides the attribute for that call
    assert calls["batch"] == 3 and len(calls["patient"]) == 2
    # the decoder reaches it through hode_solve: decoder.ode.step_control = "patient" is all a user sets
    torch.manual_seed(1)
    dec = model.RocheExpertDecoder(5, 6, 1, 1.0, 0.1, method="dopri5", device=CPU)
    a = torch.zeros(11, 3, 1)
    a[4, :, 0] = 2.0
    dec.latent(torch.rand(3, 6) * 0.01, a)
    assert calls["batch"] == 4
    dec.ode.step_control = "patient"
    dec.latent(torch.rand(3, 6) * 0.01, a)
    assert len(calls["patient"]) == 3 and calls["batch"] == 4


def test_the_fixed_grid_methods_ignore_it(monkeypatch):
    import hode
    seen = []
    monkeypatch.setattr(hode, "roche_solve", lambda *a, **kw: seen.append(kw["method"]) or torch.zeros(11, 3, 6))
    ode, y0, t = _ode(6)
    ode.step_control = "patient"
    hode.odeint(ode, y0, t, method="rk4")
    hode.odeint(ode, y0, t, method="euler", options={"step_control": "patient"})
    assert seen == ["rk4", "euler"]


def test_the_autograd_function_lives_next_to_the_module_it_serves():
    """tests/test_binding_case_coverage.py walks hode/*.py: only launch functions there, the Function in model.py."""
    import test_binding_case_coverage as cov
    found = cov.bindings()
    assert not [b for b in found if b.startswith(("patient_dopri5.", "_dopri5_pp_lib."))], found
    assert issubclass(model._RochePatientDopri5, torch.autograd.Function)
    assert not cov.pointer_problems()


# ------------------------------------------------------------------------------------- 6. the grid cases' table
def test_the_grid_table_holds_what_the_issue_lists():
    gs = cases.GRID_CASES
    assert {c["grid"] for c in gs} == set(cases.GRIDS) and all(c["T"] == cases.GRID_T == 12 for c in gs)
    assert {c["B"] for c in gs} == {1, 3, 70} and {c["K"] for c in gs} == {1, 2, 3}
    for g in cases.GRIDS:
        on = [c for c in gs if c["grid"] == g]
        assert {c["D"] for c in on} == set(cases.DIMS), g
        assert any(c["ablate"] for c in on) and any(c["hill"] == "general" for c in on) and any(not c["need_theta"] for c in on), g
    assert {cases.bodies(c) for c in gs} == {cases.bodies(c) for c in cases.CASES} == {(True, True), (True, False), (False, False)}
    ids = list(map(cases.case_id, cases.CASES + gs))
    assert len(set(ids)) == len(ids) and len(gs) <= 18
    assert len(set(map(cases.audit_id, cases.AUDIT_CASES))) == len(cases.AUDIT_CASES)


def test_grid_case_inputs_are_time_grids_own_and_hold_the_doses_they_name():
    import time_grids as tg
    from oracle.rhs import THETA_NAMES
    for c in cases.GRID_CASES + cases.AUDIT_CASES:
        inp, f = cases.setup(c)
        p = tg._roche_inputs(c["D"], c["ablate"], c["K"], c["grid"], c["T"])
        B, rows = c["B"], slice(c["first"], c["first"] + c["B"])
        assert torch.equal(inp["t"], tg.grid(c["grid"], 12)) and torch.equal(inp["times"], p["times"][rows]) and inp["times"].shape == (B, c["K"])
        assert torch.equal(inp["dosage"], p["dosage"][rows])  # a quarter of synth's amounts, as time_grids takes them
        if "stiff" not in c:
            assert torch.equal(inp["z0"], p["y0"][rows])
        assert f.ablate == c["ablate"] and (float(f.HillCure) == 2.0) == (c["hill"] == "two")
        if c["hill"] == "general":
            assert [float(getattr(f, n)) for n in THETA_NAMES] == [pytest.approx(v) for v in cases.THETA_GENERAL]
        t0, S = float(inp["t"][0]), cases.subset(B)
        inside = [x for x in inp["times"].double().flatten().tolist() if x not in inp["t"].double().tolist() and x > t0]
        assert inside or B == 1, cases.case_id(c)  # doses strictly inside grid steps
        if c["grid"] != "clustered":  # among the replayed patients: a dose before t[0] and a dose exactly on it
            assert bool((inp["times"][S] == t0 - tg.BEFORE).any()) and bool((inp["times"][S] == t0).any()), cases.case_id(c)
    assert float(tg.grid("offset-", 12)[0]) < 0 < float(tg.grid("offset-", 12)[-1]) and float(tg.grid("offset+", 12)[0]) == 2.5
    # the cached problem of time_grids was not written into
    c = cases.AUDIT_CASES[1]
    assert "stiff" in c and float(cases.setup(c)[0]["z0"][cases.STIFF].abs().max()) > 100 * float(
        tg._roche_inputs(c["D"], c["ablate"], c["K"], c["grid"], c["T"])["y0"][c["first"] + cases.STIFF].abs().max())


# ------------------------------------------------------------------------------------- 7. the controller audit
HEADROOM = 0.5  # the fp32 oracle has to pass at this share of RATIO_MARGIN and DT_RTOL (as tests/test_time_grid_cases.py)


@functools.lru_cache(maxsize=None)
def _oracle_runs(i):
    """The free-running oracle at batch one, in float64 and in fp32, on every audited patient of AUDIT_CASES[i]."""
    c = cases.AUDIT_CASES[i]
    inp, f = cases.setup(c)
    dosage, times = cases.schedule(inp, f)
    out = []
    for p in cases.subset(c["B"]):
        run = {"p": p, "y0": inp["z0"][p], "t": inp["t"], "rhs64": audit.patient_rhs(f, dosage, times, p)}
        _, run["st64"], run["tape64"] = audit.free_run(run["rhs64"], run["y0"], run["t"], c["rtol"], c["atol"])
        _, run["st32"], run["tape32"] = audit.free_run(audit.patient_rhs(f, dosage, times, p, torch.float32), run["y0"], run["t"],
                                                       c["rtol"], c["atol"])
        out.append(run)
    return out


def _audit(c, run, tape, n_rejected, share=1.0):
    return audit.audit(run["rhs64"], run["y0"], run["t"], c["rtol"], c["atol"], tape, n_rejected, share * cases.RATIO_MARGIN,
                       share * cases.DT_RTOL)


def test_the_audit_table_holds_what_the_issue_lists():
    cs = cases.AUDIT_CASES
    assert 8 <= len(cs) <= 10 and all(c["B"] == 70 and not c["ablate"] for c in cs)
    assert {c["grid"] for c in cs} == set(cases.GRIDS) and {c["D"] for c in cs} >= {4, 12} and {c["D"] for c in cs} & {6, 8}
    tols = {(c["rtol"], c["atol"]) for c in cs}
    assert len(tols) == 2 and (cases.RTOL, cases.ATOL) not in tols and len({r / a for r, a in tols}) == 2
    assert all(r != a for r, a in tols)  # swapping the two changes the problem
    assert any("stiff" in c for c in cs) and all(c["stiff"][0] == cases.STIFF in cases.subset(70) for c in cs if "stiff" in c)
    assert cases.RATIO_MARGIN == 8 * cases.MEASURED_RATIO_DIST and cases.DT_RTOL == 8 * cases.MEASURED_DT_DIST


@pytest.mark.parametrize("i", range(len(cases.AUDIT_CASES)), ids=[cases.audit_id(c) for c in cases.AUDIT_CASES])
def test_the_float64_oracle_decides_every_attempt_and_the_fp32_oracle_passes_the_audit(i, record_property):
    """The inputs were chosen so that the float64 oracle, free-running, has no attempt whose ratio is within RATIO_MARGIN of
    1 on any audited patient (so no patient is undecidable before fp32 comes in), and its own tape passes the audit.  The
    fp32 oracle -- the stand-in for the device the two constants were measured on -- stays within HEADROOM of both, and its
    tape passes the audit at HEADROOM of both."""
    c = cases.AUDIT_CASES[i]
    worst = {"ratio": 0.0, "dt": 0.0}
    for run in _oracle_runs(i):
        clear = min(abs(r - 1.0) / max(1.0, r) for _, _, _, r in run["st64"]["attempts"])
        assert clear > cases.RATIO_MARGIN, (run["p"], clear)
        rep = _audit(c, run, run["tape64"], run["st64"]["n_rejected"])
        assert rep["ok"] and not rep["left_out"], (run["p"], rep)
        dist = max(audit.ratio_distances(run["rhs64"], run["t"], c["rtol"], c["atol"], run["st32"]))
        rep = _audit(c, run, run["tape32"], run["st32"]["n_rejected"], HEADROOM)
        assert rep["ok"] and not rep["left_out"], (run["p"], rep)
        worst["ratio"], worst["dt"] = max(worst["ratio"], dist, rep["ratio_dist"]), max(worst["dt"], rep["dt_dist"])
    record_property("fp32_oracle_ratio_dist", worst["ratio"])
    record_property("fp32_oracle_dt_dist", worst["dt"])
    assert worst["ratio"] <= HEADROOM * cases.RATIO_MARGIN and worst["dt"] <= HEADROOM * cases.DT_RTOL, worst


def test_the_audited_inputs_exercise_the_controller():
    """On the oracle's counts: patients reject, take different numbers of steps, the scaled patients' first attempt is
    rejected, some audited patient's rejected count is held exactly and is not zero, most steps' proposals are followed
    through, and on the clustered grid one step covers at least 3 output times while at least 2 cover none."""
    import time_grids as tg
    exact, steps, open_steps = [], 0, 0
    for i, c in enumerate(cases.AUDIT_CASES):
        runs = _oracle_runs(i)
        counts = [(r["st32"]["n_accepted"], r["st32"]["n_rejected"]) for r in runs]
        assert len({a for a, _ in counts}) > 1 and any(b > 0 for _, b in counts), (cases.audit_id(c), counts)
        for run in runs:
            if "stiff" in c and run["p"] == cases.STIFF:
                assert not run["st32"]["first_attempt_accepted"] and not run["st64"]["first_attempt_accepted"]
            elif c["grid"] == "clustered":
                cover = tg.outputs_per_step(run["st32"]["tape"], run["t"].numpy())
                assert max(cover) >= 3 and sum(1 for n in cover if n == 0) >= 2, (cases.audit_id(c), run["p"], cover)
            rep = _audit(c, run, run["tape32"], run["st32"]["n_rejected"])
            steps, open_steps = steps + rep["steps"], open_steps + rep["open_steps"]
            if rep["exact"]:
                exact.append(rep["n_rejected"])
    assert any("stiff" in c for c in cases.AUDIT_CASES)
    assert len(exact) >= 5 and sum(1 for n in exact if n > 0) >= 2, exact
    assert open_steps <= 0.4 * steps, (open_steps, steps)


def _wrong_controller(c, run, other, kind):
    """oracle.solvers._odeint_dopri5's loop in fp32 on one patient with one thing wrong; returns (tape, n_rejected) of the
    patient as a device would report them.  `kind`: "joint" (the norm over this patient and `other` together, count 2 D),
    "swap" (rtol and atol swapped), "safety" (0.8 instead of 0.9), "tol_y" (tol from |y| alone), "half" (a first step of
    0.5 x Hairer's), None (nothing wrong)."""
    from oracle import solvers as S
    rtol, atol = (c["atol"], c["rtol"]) if kind == "swap" else (c["rtol"], c["atol"])
    inp, f0_ = cases.setup(c)
    dosage, times = cases.schedule(inp, f0_)
    rows = [run["p"], other] if kind == "joint" else [run["p"]]
    fm = copy.deepcopy(f0_)
    fm.dosage, fm.times = dosage[rows], times[rows]
    f, tab, t = S._Rhs(fm), audit.tableau(torch.float32), run["t"].double()
    with torch.no_grad():
        y = inp["z0"][rows].clone()
        fy = f(t[0], y)
        dt = S._initial_step(f, t[0], y, 4, rtol, atol, fy) * (0.5 if kind == "half" else 1.0)
        t_hi, tape, rejected = t[0], {"t": [], "dt": [], "y": []}, 0
        while t_hi < t[-1]:
            y1, f1, err, _ = S._dp_attempt(f, y, fy, t_hi, dt, t_hi + dt, tab)
            tol = atol + rtol * (y.abs() if kind == "tol_y" else torch.max(y.abs(), y1.abs()))
            ratio = S._rms(err / tol).abs()
            if ratio <= 1:
                tape["t"].append(float(t_hi)), tape["dt"].append(float(dt)), tape["y"].append(y[:1].clone())
                t_hi, y, fy = t_hi + dt, y1, f1
            else:
                rejected += 1
            dt = S._next_dt(dt, ratio, safety=0.8 if kind == "safety" else 0.9)
    tape["y"] = torch.cat(tape["y"], dim=0)
    return tape, rejected


def test_the_restated_loop_is_the_oracles():
    """_wrong_controller with nothing wrong gives the fp32 oracle's own tape and count, bit for bit."""
    for i in (0, 3):
        c = cases.AUDIT_CASES[i]
        for run in _oracle_runs(i)[:2]:
            tape, rejected = _wrong_controller(c, run, None, None)
            assert tape["t"] == run["tape32"]["t"] and tape["dt"] == run["tape32"]["dt"] and rejected == run["st32"]["n_rejected"]
            assert torch.equal(tape["y"], run["tape32"]["y"])


#: which audited case catches which wrong controller (found on the CPU; the test below holds it)
CAUGHT_BY = {"joint": 0, "swap": 3, "safety": 4, "tol_y": 5, "half": 2}


@pytest.mark.parametrize("kind", sorted(CAUGHT_BY))
def test_a_wrong_controller_fails_the_audit(kind):
    i = CAUGHT_BY[kind]
    c, runs = cases.AUDIT_CASES[i], _oracle_runs(i)
    failed = []
    for k, run in enumerate(runs):
        tape, rejected = _wrong_controller(c, run, runs[(k + 1) % len(runs)]["p"], kind)
        rep = _audit(c, run, tape, rejected)
        if not rep["ok"] and not rep["left_out"]:
            failed.append((run["p"], rep["why"]))
    print(kind, cases.audit_id(c), failed)
    assert failed, (kind, cases.audit_id(c))
