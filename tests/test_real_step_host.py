"""CPU checks of the one-step-ahead solve's side library (no GPU): libhode_real_step.so's C ABI, its row of the build
table, the kernels its objects contain against the GPU case table (tests/real_step_cases.py), the library's own argument
checks, workspace layout and launch rule, the adapter that presents it under libhode.so's names, and the grid-table builder
of hode.real_step against hode.substep.fixed_grid."""
import glob
import os
import sys

import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import real_step_cases as cases

ROOT = build_hip.ROOT
LIB = "libhode_real_step.so"
FUNCTIONS = {"hode_real_step_" + n for n in ("version", "last_error_string", "workspace_bytes", "intervals_per_wave", "rk_fwd", "rk_bwd")}
SIZES = b"latent_dim 5 .. 20 with hidden_dim 1 .. 64 and 1 .. 8 solver steps per interval"
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    from hode import _real_step_lib as RS
    return abi_checks.built(RS.LIBRARY)


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
def test_header_functions_are_exported_and_bound(lib):
    from hode import _real_step_lib as RS
    declared = abi_checks.declared_functions("hode_real_step.h", "hode_real_step_")
    assert declared == {name for name, _, _ in RS.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_real_step.h")
    assert "#define HODE_REAL_STEP_ABI_VERSION %d\n" % RS.HODE_REAL_STEP_ABI_VERSION in src
    assert lib.hode_real_step_version() == RS.HODE_REAL_STEP_ABI_VERSION
    assert '#include "hode.h"' in src and "struct" not in src   # the descriptor is hode.h's: included, not restated


def test_sizes_agree_everywhere():
    from hode import _real_step_lib as RS
    assert (RS.MIN_LATENT, RS.MAX_LATENT, RS.MAX_HIDDEN, RS.MAX_SUBSTEPS) == (5, 20, 64, 8)
    assert (cases.MIN_LATENT, cases.MAX_LATENT, cases.MAX_HIDDEN, cases.MAX_SUBSTEPS) == (5, 20, 64, 8)
    assert RS.MAX_HIDDEN == 16 * max(cases.HTS) == 16 * max(build_hip.REAL_STEP_HTS) and build_hip.REAL_STEP_HTS == cases.HTS
    internal = open(os.path.join(build_hip.CSRC, "real_step", "hode_real_step.hpp")).read()
    assert "constexpr int kRealStepMinLatent = 5, kRealStepMaxLatent = 20, kRealStepMaxHidden = 64, kRealStepMaxSub = 8;" in internal
    assert '#define HODE_REAL_STEP_TEXT "%s"\n' % SIZES.decode() in internal
    side = open(os.path.join(build_hip.CSRC, "hode_real_side_host.hpp")).read()   # the hidden-tile counts: once, for the three side libraries
    assert "#define HODE_REAL_SIDE_HTS(X) " + " ".join("X(%d)" % n for n in cases.HTS) + "\n" in side
    assert "HODE_REAL_SIDE_HTS(HODE_REAL_STEP_DECL)" in internal and "HODE_REAL_STEP_HTS" not in internal
    assert "5 .. 20" in RS.sizes_text() and "1 .. 64" in RS.sizes_text() and "1 .. 8" in RS.sizes_text()


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    hashed = build_hip.digest_files(LIB)
    assert row.header == "include/hode_real_step.h" and "include/hode.h" in hashed
    assert row.src_dir == build_hip.PKG + "/csrc/real_step"
    want = ["hode_real_step"] + ["hode_real_step_ht%d" % n for n in cases.HTS]
    assert sorted(n for n, _, _ in row.units()) == sorted(want)
    assert build_hip.PKG + "/csrc/hode_real_mf.hpp" in hashed and build_hip.PKG + "/csrc/hode_rk_host.hpp" in hashed
    assert build_hip.PKG + "/csrc/hode_real_side_host.hpp" in hashed
    host = open(os.path.join(build_hip.CSRC, "real_step", "hode_real_step.hip")).read()
    assert "hode_error_state.hpp" in host and host.count("__global__") == 1 and "void real_step_dose_kernel(" in host   # the dose-table prelude alone


def test_the_device_code_is_shared_not_copied():
    """The step kernels are a walk over intervals around csrc/hode_real_mf.hpp: the rhs, its VJP, the gradient accumulator,
    the fold and the stage arithmetic of a solver step are defined there and nowhere in csrc/real_step/."""
    csrc = build_hip.CSRC
    shared = open(os.path.join(csrc, "hode_real_mf.hpp")).read()
    names = ("struct RealMf", "struct RealGradAcc", "void real_grad_fold(", "void real_step_fwd(", "define HODE_REAL_STEP_STAGES(",
             "define HODE_REAL_STEP_CHAIN(", "void real_load_state(", "void real_store_state(")
    for name in names:
        assert shared.count(name) == 1, name
        for other in ("real_step/hode_real_step_ht.hip", "real_step/hode_real_step.hip", "real_step/hode_real_step.hpp"):
            assert name not in open(os.path.join(csrc, other)).read(), (name, other)
    src = open(os.path.join(csrc, "real_step", "hode_real_step_ht.hip")).read()
    for use in ("real_step_fwd<", "HODE_REAL_STEP_STAGES(", "HODE_REAL_STEP_CHAIN(", "real_grad_fold<", "RealTileRagged", "hode_real_mf.hpp"):
        assert use in src, use
    assert "real_dose_table(" not in src   # the solve kernels only read the table
    body = shared[shared.index("void real_mf_body("):]
    for use in ("real_step_fwd<", "HODE_REAL_STEP_STAGES(", "HODE_REAL_STEP_CHAIN("):
        assert use in body, use   # the chained solve runs the same pieces


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        build_hip.build(verbose=False)
        objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    want = cases.expected_kernels()
    assert len(want) == 2 + len(cases.HTS) * (1 + 2 * len(cases.METHODS)) == 30
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert cases.kernels_reached() == compiled
    for group in (cases.COMPARE_CASES, cases.PADDING_CASES):
        assert cases.kernels_reached(group) <= compiled
    assert not any(kv.family(n) for n in compiled - {"hode::fold_partials_kernel"})


def test_the_case_table_holds_what_it_promises():
    cs = cases.CASES
    assert {c["D"] for c in cs} == set(cases.EDGE_D) == {5, 7, 8, 9, 12, 19, 20}
    assert {c["H"] for c in cs} >= set(cases.EDGE_H) and cases.EDGE_H == (1, 16, 17, 43, 64)
    assert {c["B"] for c in cs} >= set(cases.EDGE_B) and cases.EDGE_B == (1, 15, 16, 17, 37)
    assert {c["N"] for c in cs} == set(cases.EDGE_N) == {1, 2, 7} and {c["S"] for c in cs} == set(cases.EDGE_S) == {1, 2, 3}
    assert {(cases.ht(c["H"]), c["method"]) for c in cs} == {(n, m) for n in cases.HTS for m in cases.METHODS}
    forced = {(c["C"], c["N"]) for c in cs}
    assert {c for c, _ in forced} >= {0, 1, 2, 3} and any(c == n for c, n in forced) and any(c > n for c, n in forced)
    assert any(0 < c < n and n % c for c, n in forced) and any(0 < c < n and n % c == 0 for c, n in forced)   # runs end inside / on N
    everything = cs + cases.PADDING_CASES + cases.COMPARE_CASES
    assert all(c["B"] <= 37 and c["perturb"] == (c["method"] != "euler") and cases.T_START + c["N"] <= cases.TA for c in everything)
    assert {(c["D"], c["B"]) for c in cases.PADDING_CASES} == {(5, 17), (19, 1), (5, 1), (19, 17)}
    assert all(c["S"] == 1 for c in cases.COMPARE_CASES) and {c["method"] for c in cases.COMPARE_CASES} == set(cases.METHODS)
    assert {c["D"] == 20 for c in cases.COMPARE_CASES} == {True, False}
    assert cases.MODEL_DIMS == (7, 20) and cases.MODEL_STEP_DIVS == (1, 2)


# ------------------------------------------------------------------------------------------------ 2. the library's checks
def _desc(D=10, **over):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim, d.n_action_times = L.RHS_ROCHE_REAL, L.METHODS["rk4"], 17, D, 6, 43, 10
    d.n_dose = 2
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_argument_errors_do_not_launch(lib):
    from hode import _lib as L
    err = lib.hode_real_step_last_error_string
    fwd, bwd = lib.hode_real_step_rk_fwd, lib.hode_real_step_rk_bwd
    for fn in (fwd, bwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        for kind in (L.RHS_ROCHE, L.RHS_NEURAL):
            assert fn(_desc(rhs_kind=kind), None) == E_UNSUPPORTED and b"rhs_kind %d " % kind in err() and SIZES in err()
        for D in (0, 4, 21, 36):
            assert fn(_desc(D), None) == E_UNSUPPORTED and b"latent_dim %d " % D in err() and SIZES in err()
        for H in (0, -1, 65):
            assert fn(_desc(hidden_dim=H), None) == E_UNSUPPORTED and b"hidden_dim %d " % H in err() and SIZES in err()
        for S in (0, -1, 9, 100):
            assert fn(_desc(n_dose=S), None) == E_UNSUPPORTED and b"%d solver steps per interval" % S in err() and SIZES in err()
        for lanes in (1, 4, 48):
            assert fn(_desc(lanes_per_patient=lanes), None) == E_UNSUPPORTED and b"lanes_per_patient %d " % lanes in err()
        assert fn(_desc(method=3), None) == E_UNSUPPORTED and b"method 3" in err()
        assert fn(_desc(flags=L.FLAG_TAPE), None) == E_UNSUPPORTED and b"flags %d" % L.FLAG_TAPE in err()
        for D in range(5, 21):   # a shape of the domain, pointers missing
            assert fn(_desc(D), None) == E_NULL and b"must be non-NULL" in err()
        for k in ("batch", "n_times", "n_action_times"):
            assert fn(_desc(**{k: 0}), None) == E_SIZE and b"%s=0" % k.encode() in err()
        assert fn(_desc(max_steps=-1), None) == E_SIZE and b"max_steps=-1" in err()
    ptrs = {k: 64 for k in ("t", "y0", "dosage", "theta", "w1", "h")}
    for k in ptrs:
        assert fwd(_desc(**dict(ptrs, **{k: None})), None) == E_NULL
    assert fwd(_desc(**ptrs), None) == E_WORKSPACE and b"workspace 0 B < required" in err()
    assert bwd(_desc(**ptrs), None) == E_NULL and b"grad_h / grad_y0 / grad_theta" in err()
    ptrs.update(grad_h=64, grad_y0=64, grad_theta=64)
    assert bwd(_desc(**ptrs), None) == E_UNSUPPORTED and b"grad_w1 is NULL" in err() and b"operand-tape" in err()
    ptrs.update(grad_w1=64)
    assert bwd(_desc(**ptrs), None) == E_WORKSPACE and b"workspace 0 B < required" in err()
    need = lib.hode_real_step_workspace_bytes(_desc(), L.WS_RK_BWD)
    assert bwd(_desc(workspace=64, workspace_bytes=need - 1, **ptrs), None) == E_WORKSPACE
    assert bwd(_desc(workspace=68, workspace_bytes=need, **ptrs), None) == E_ALIGN and b"16-byte aligned" in err()


def _rule(B, N, forced):
    """The launch rule restated: a forced C is clipped to N; otherwise the C that minimises rounds x (C + 2), rounds =
    ceil(waves / 1 024) with waves = ceil(B / 16) ceil(N / C), the shortest such run."""
    if forced > 0:
        return min(forced, N)
    blocks = -(-B // 16)
    return min(range(1, N + 1), key=lambda c: (-(-blocks * -(-N // c) // 1024) * (c + 2), c))


def test_workspace_sizes_and_the_launch_rule(lib):
    """[ per-wave weight-gradient blocks of (4 HT + 3) 256 + 16 floats | three floats per wave | sub-step states
    N (S - 1) B D floats | dose table 2 (Ta + 1) B floats ], each rounded up to 256 bytes, waves = ceil(B / 16) ceil(N / C);
    the forward holds the dose table alone."""
    from hode import _lib as L
    ws, cpw = lib.hode_real_step_workspace_bytes, lib.hode_real_step_intervals_per_wave

    def up(n):
        return -(-n // 256) * 256
    for D in (5, 12, 20):
        for H in (1, 17, 43, 64):
            for B in (1, 16, 17, 37, 2097, 8192):
                for N, S, forced in ((1, 1, 0), (7, 2, 0), (7, 3, 3), (7, 1, 9), (119, 1, 0), (119, 8, 5)):
                    d = _desc(D, hidden_dim=H, batch=B, n_times=N, n_dose=S, max_steps=forced, n_action_times=30)
                    C = _rule(B, N, forced)
                    assert cpw(d) == C, (B, N, forced)
                    waves, dose = -(-B // 16) * -(-N // C), up(2 * 31 * B * 4)
                    assert ws(d, L.WS_RK_FWD) == dose
                    assert ws(d, L.WS_RK_BWD) == (up(waves * ((4 * cases.ht(H) + 3) * 256 + 16) * 4) + up(waves * 12)
                                                  + up(N * (S - 1) * B * D * 4) + dose), (D, H, B, N, S, forced)
    assert _rule(8192, 119, 0) == 60 and _rule(2097, 119, 0) == 17 and _rule(33, 119, 0) == 1   # config 5's shapes
    for which in (L.WS_DOPRI5_FWD, L.WS_DOPRI5_BWD):
        assert ws(_desc(), which) == 0
    for bad in (_desc(4), _desc(21), _desc(hidden_dim=65), _desc(lanes_per_patient=1), _desc(batch=0), _desc(n_dose=9),
                _desc(rhs_kind=L.RHS_ROCHE), _desc(max_steps=-2)):
        assert ws(bad, L.WS_RK_FWD) == 0 and ws(bad, L.WS_RK_BWD) == 0 and cpw(bad) == 0


def test_the_adapter_presents_the_library_under_libhode_names(lib):
    """One adapter per call: it writes the interval count, the solver steps and the forced run length into the descriptor
    fields the header names, reports this library's own error text, and hode.real recognises it for the on-chip path."""
    from hode import HodeConfigError, _lib as L, _real_dims_lib as RD, _real_step_lib as RS
    side = RS.step_library(6, 2, 3)
    assert RS.is_step_library(side) and not RD.is_side_library(side) and not RS.is_step_library(RD.side_library())
    for name, _, _ in RS.SOLVER_ENTRIES:
        assert callable(getattr(side, "hode_" + name))
    d = _desc(n_times=21, n_dose=0)   # what hode.real._desc leaves there: t.numel() and nothing
    assert side.hode_workspace_bytes(d, L.WS_RK_BWD) == lib.hode_real_step_workspace_bytes(_desc(n_times=6, n_dose=2, max_steps=3), L.WS_RK_BWD)
    assert (d.n_times, d.n_dose, d.max_steps) == (6, 2, 3) and side.chosen_intervals_per_wave(d) == 3
    with pytest.raises(HodeConfigError, match=r"hode_real_step_rk_fwd failed \(code -3\): real step: lanes_per_patient 1 "):
        side.hode_rk_fwd(_desc(lanes_per_patient=1), None)
    src = open(os.path.join(ROOT, build_hip.PKG, "hode", "real.py")).read()
    assert "RD.is_side_library(lib) or RS.is_step_library(lib)" in src


# -------------------------------------------------------------------------------------------------- 3. the grid table
@pytest.mark.parametrize("t0", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_grid_table_is_fixed_grid_per_interval(S, t0):
    """Row i of the table is substep.fixed_grid(t[i : i + 2], 1 / S), bit for bit, on the decoder's own grid -- with the
    offset start t[0] = -1 of t0 = 0 -- and for a float64 grid in float64."""
    from hode import real_step, substep
    for dtype in (torch.float32, torch.float64):
        t = torch.arange(t0 - 1, 8, 1, dtype=dtype)
        table = real_step.interval_grids(t, 1.0 / S)
        assert table.shape == (t.numel() - 1, S + 1) and table.dtype == dtype
        for i in range(t.numel() - 1):
            want = substep.fixed_grid(t[i:i + 2], 1.0 / S)
            assert torch.equal(table[i], want), (i, table[i], want)
            assert table[i, 0] == t[i] and table[i, -1] == t[i + 1] and bool((table[i, 1:] > table[i, :-1]).all())
    plain = real_step.interval_grids(torch.arange(-1.0, 8.0), None)
    assert torch.equal(plain, torch.stack([torch.arange(-1.0, 7.0), torch.arange(0.0, 8.0)], dim=1))


def test_grid_table_refuses_unequal_and_too_many_steps():
    from hode import HodeConfigError, real_step
    with pytest.raises(HodeConfigError, match="same number of solver steps in every interval.*1 and 2"):
        real_step.interval_grids(torch.tensor([0.0, 1.0, 3.0]), 1.0)
    with pytest.raises(HodeConfigError, match="no kernel for 9 solver steps per interval"):
        real_step.interval_grids(torch.arange(0.0, 4.0), 1.0 / 9)
    assert real_step.interval_grids(torch.arange(0.0, 4.0), 1.0 / 8).shape == (3, 9)


def test_grid_table_is_cached_per_grid_tensor(monkeypatch):
    """One read-back per grid tensor: the second call with the same tensor and step size builds nothing."""
    from hode import real_step
    t = torch.arange(0.0, 6.0)
    first = real_step._grid_table(t, 0.5)
    monkeypatch.setattr(real_step, "interval_grids", lambda *a: pytest.fail("rebuilt"))
    assert real_step._grid_table(t, 0.5) is first
    monkeypatch.undo()
    assert real_step._grid_table(t, 1.0).shape == (5, 2) and real_step._grid_table(t.clone(), 0.5) is not first
    t.add_(1.0)   # a new version of the same tensor
    assert torch.equal(real_step._grid_table(t, 0.5)[0], torch.tensor([1.0, 1.5, 2.0]))
