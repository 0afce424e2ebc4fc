"""CPU checks of the all-steps LSTM's side library (no GPU): libhode_lstm_seq.so's C ABI and refusals, its row of the
build table, the kernels its objects contain against the GPU case table (tests/lstm_seq_cases.py), the adapter that offers
it under libhode.so's entry names, how ``hode.lstm`` is wired to it, and what stays as it was: libhode.so keeps its own
kernels."""
import glob
import inspect
import os
import sys

import pytest
import torch

import abi_checks
import build_hip
import kernel_variants as kv
import lstm_seq_cases as cases

ROOT = build_hip.ROOT
LIB = "libhode_lstm_seq.so"
FUNCTIONS = {"hode_lstm_seq_" + n for n in ("version", "last_error_string", "workspace_bytes", "fwd", "bwd", "fill_operand")}
E_NULL, E_SIZE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from hode import _lstm_seq_lib as SL
    return abi_checks.built(SL.LIBRARY)


# ------------------------------------------------------------------------------------------------------ 1. ABI, build
def test_header_functions_are_exported_and_bound(lib):
    from hode import _lstm_seq_lib as SL
    declared = abi_checks.declared_functions("hode_lstm_seq.h", "hode_lstm_seq_")
    assert declared == {name for name, _, _ in SL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_lstm_seq.h")
    assert "#define HODE_LSTM_SEQ_ABI_VERSION %d\n" % SL.HODE_LSTM_SEQ_ABI_VERSION in src
    assert lib.hode_lstm_seq_version() == SL.HODE_LSTM_SEQ_ABI_VERSION
    assert '#include "hode.h"' in src and "struct" not in src   # the descriptor is hode.h's: included, not restated
    raw = open(os.path.join(ROOT, "include", "hode_lstm_seq.h")).read()
    assert "h_out       [T][B][H]" in raw and "grad_h_out  [T][B][H]" in raw   # the two fields that are read differently


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    hashed = build_hip.digest_files(LIB)
    assert row.header == "include/hode_lstm_seq.h" and "include/hode.h" in hashed
    assert row.src_dir == build_hip.PKG + "/csrc/lstm_seq"
    units = {n: (os.path.relpath(s, build_hip.CSRC), e) for n, s, e in row.units()}
    assert sorted(units) == sorted(["hode_lstm_seq", "hode_lstm_seq_host"] + ["hode_lstm_seq_tpw%d" % n for n in cases.TPWS])
    # libhode.so's own units compiled a second time under the unit macro: no copy of the host code
    assert units["hode_lstm_seq_host"] == ("hode_lstm.hip", ["-DHODE_LSTM_SEQ_UNIT"])
    for n in cases.TPWS:
        assert units["hode_lstm_seq_tpw%d" % n] == ("hode_lstm_tpw.hip", ["-DHODE_LSTM_SEQ_UNIT", "-DHODE_LSTM_TPW=%d" % n])
    assert [f for f in os.listdir(os.path.join(build_hip.CSRC, "lstm_seq")) if f != "build"] == ["hode_lstm_seq.hip"]
    assert build_hip.LSTM_TPWS == cases.TPWS
    for f in ("hode_lstm.hip", "hode_lstm_tpw.hip", "hode_lstm_kernels.hpp", "hode_lstm_fwd_body.hpp", "hode_lstm_bwd_body.hpp"):
        assert build_hip.PKG + "/csrc/" + f in hashed, f


def test_the_kernel_bodies_are_shared_not_copied():
    """One text per kernel body, included by the final-state kernel and by the all-steps kernel; the all-steps kernels exist
    only under the unit macro of this library."""
    csrc = build_hip.CSRC
    kernels = open(os.path.join(csrc, "hode_lstm_kernels.hpp")).read()
    for body in ("hode_lstm_fwd_body.hpp", "hode_lstm_bwd_body.hpp"):
        assert kernels.count('#include "%s"' % body) == 2, body
        assert "__global__" not in open(os.path.join(csrc, body)).read()
    assert kernels.count("using POLICY = LstmFinalState;") == 2 and kernels.count("using POLICY = LstmSequence;") == 2
    before, _, after = kernels.partition("#ifdef HODE_LSTM_SEQ_UNIT")
    assert "lstm_seq_fwd_kernel" not in before and "lstm_seq_fwd_kernel(LstmArgs p)" in after
    for name in ("void lstm_fwd_kernel(LstmArgs p)", "void lstm_bwd_kernel(LstmBwdArgs p)", "void lstm_seq_fwd_kernel(LstmArgs p)",
                 "void lstm_seq_bwd_kernel(LstmBwdArgs p)"):
        assert kernels.count(name) == 1, name
    assert "int lstm_geom(" not in open(os.path.join(csrc, "lstm_seq", "hode_lstm_seq.hip")).read()


def _compiled(obj_dir):
    objs = sorted(o for o in glob.glob(os.path.join(obj_dir, "*.o")) if "__" not in os.path.basename(o))
    if not objs:
        build_hip.build(verbose=False)
        objs = sorted(o for o in glob.glob(os.path.join(obj_dir, "*.o")) if "__" not in os.path.basename(o))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    return {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    """The kernel symbols of csrc/lstm_seq/build/*.o are the instantiations the case table states, every one is reached by a
    case, and every case names a compiled one.  libhode.so holds none of the all-steps kernels and this library none of the
    final-state ones."""
    compiled = _compiled(build_hip.LIBRARIES[LIB].obj)
    want = cases.expected_kernels()
    assert len(want) == 4 + len(cases.TPWS) * 2 * (2 * 4 + 3) == 180   # forward: NT x VEC4 x PAD; backward: NT x FLAT
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    assert cases.kernels_reached() == compiled
    for group in (cases.DIFF_CASES, cases.MIDDLE_CASES, [cases.AUTOGRAD_CASE], [cases.SENTINEL_CASE]):
        assert cases.kernels_reached(group) <= compiled
    assert not any(n.startswith(("hode::lstm_fwd_kernel", "hode::lstm_bwd_kernel")) for n in compiled)
    main = _compiled(build_hip.LIBRARIES["libhode.so"].obj)
    assert not any("lstm_seq" in n for n in main)
    assert {n.replace("lstm_seq_", "lstm_") for n in compiled} == {n for n in main if n.startswith("hode::lstm_")}


def test_the_case_table_holds_what_it_promises():
    F, B = cases.FWD_CASES, cases.BWD_CASES
    assert len(F) == 64 and len(B) == 48
    P = cases.PAD_FWD_CASES   # the forward cases again with the other hidden size of each: padded units on / off
    assert [(c["H"] % 16 == 0, c["obs"], c["nt"], c["reverse"]) for c in P] == [(c["H"] % 16 != 0, c["obs"], c["nt"], c["reverse"]) for c in F]
    assert {c["T"] for c in P} == {1, 3, 5} and not any(c["tape"] for c in P)
    assert not {cases.case_id(c) for c in P} & {cases.case_id(c) for c in F + B}
    for c in F + B:
        assert c["B"] == 32 * c["nt"] + 5 and c["obs"] in (20, 23) and c["H"] <= cases.MAX_HIDDEN
    assert all(not c["tape"] and c["T"] in (1, 3, 4) for c in F) and all(c["tape"] and c["T"] == 4 for c in B)
    for tpw in cases.TPWS:
        fs = [c for c in F if -(-c["H"] // 16) == tpw]
        assert {c["nt"] for c in fs} == {1, 2, 3, 4} and {c["T"] for c in fs} == {1, 3, 4}
        assert {(c["H"] == 16 * tpw, c["obs"]) for c in fs} == {(f, o) for f in (True, False) for o in (20, 23)}
        assert {c["H"] for c in fs} == {16 * tpw, 16 * tpw - 3}
        assert {c["a"] for c in fs} == {c["mask"] for c in fs} == {True, False} and {c["reverse"] for c in fs} == {0, 1}
        bs = [c for c in B if -(-c["H"] // 16) == tpw]
        assert {(c["nt"], c["H"] == 16 * tpw) for c in bs} == {(n, f) for n in (1, 2, 3) for f in (True, False)}
    assert {(c["reverse"], c["H"] % 16 == 0) for c in B} == {(r, f) for r in (0, 1) for f in (True, False)}
    assert {c["a"] for c in B} == {c["mask"] for c in B} == {True, False}
    assert {c["reverse"] for c in cases.DIFF_CASES} == {0, 1} and len(cases.DIFF_CASES) >= 8
    assert [(c["T"], c["row"], c["reverse"]) for c in cases.MIDDLE_CASES] == [(5, 2, 0), (5, 2, 1)]
    assert (cases.SENTINEL_CASE["B"], cases.SENTINEL_CASE["H"]) == (21, 13)
    assert cases.MODEL_SHAPE == dict(T=7, B=21, obs=24, action=1, statics=11, H=44) and cases.GRAD_TOL == 1e-4
    assert len({cases.case_id(c) for c in F}) == len(F) and len({cases.case_id(c) for c in B}) == len(B)


# ------------------------------------------------------------------------------------------- 2. the adapter, the wiring
def test_the_adapter_maps_names_as_claimed(lib):
    import hode
    from hode import _lstm_seq_lib as SL
    side = SL.side_library()
    assert side is SL.side_library() and SL.is_side_library(side) and not SL.is_side_library(hode.lib())
    assert SL.lstm_library(True) is side and SL.lstm_library(False) is hode.lib()
    assert [n for n, _, _ in SL.LSTM_ENTRIES] == ["workspace_bytes", "fwd", "bwd", "fill_operand"]
    for name, _, _ in SL.LSTM_ENTRIES:
        assert callable(getattr(side, "hode_lstm_" + name)) and hasattr(hode.lib(), "hode_lstm_" + name)
    assert side.hode_lstm_workspace_bytes is lib.hode_lstm_seq_workspace_bytes
    # a failing entry raises with THIS library's text (libhode.so has no message for it)
    d = _desc(hidden_dim=161)
    with pytest.raises(hode.HodeConfigError, match=r"hode_lstm_seq_fwd failed \(code -3\): lstm: hidden_dim 161 exceeds"):
        side.hode_lstm_fwd(d, None)
    assert side.hode_lstm_workspace_bytes(d) == 0


def test_the_binding_adds_no_function_and_takes_the_library_from_its_last_argument():
    from hode import lstm
    assert list(inspect.signature(lstm._LstmEncode.forward).parameters)[-3:] == ["reverse", "patient_tiles", "all_steps"]
    assert inspect.signature(lstm._LstmEncode.forward).parameters["all_steps"].default is False
    classes = [n for n, c in vars(lstm).items() if inspect.isclass(c) and issubclass(c, torch.autograd.Function)]
    assert classes == ["_LstmEncode"]
    sig = inspect.signature(lstm.lstm_sequence)
    assert list(sig.parameters) == ["x", "a", "mask", "w_ih", "w_hh", "b_ih", "b_hh", "reverse", "patient_tiles"]
    assert sig.parameters["reverse"].default is False and sig.parameters["patient_tiles"].default == 0
    src = inspect.getsource(lstm.lstm_sequence)
    assert "_LstmEncode.apply(" in src and "hode_lstm" not in src and "data_ptr" not in src


def test_lstm_sequence_refuses_cpu_tensors():
    import hode
    from hode.lstm import lstm_sequence
    T, B, obs, H = 3, 4, 5, 6
    w = (torch.zeros(4 * H, obs + 1), torch.zeros(4 * H, H), torch.zeros(4 * H), torch.zeros(4 * H))
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        lstm_sequence(torch.zeros(T, B, obs), torch.zeros(T, B, 1), torch.ones(T, B, obs), *w)
    with torch.no_grad(), pytest.raises(hode.HodeConfigError, match="HIP device"):
        lstm_sequence(torch.zeros(T, B, obs), None, None, torch.zeros(4 * H, obs), *w[1:])


# ----------------------------------------------------------------------------------------------- 3. the library's checks
def _desc(**over):
    from hode import _lib as L
    d = L.new_lstm_desc()
    d.seq_len, d.batch, d.input_dim, d.hidden_dim, d.obs_dim, d.save_tape = 4, 21, 24, 13, 23, 1
    for k in ("x", "a", "w_ih", "w_hh", "b_ih", "b_hh", "h_out", "c_out"):
        setattr(d, k, 64)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_argument_errors_do_not_launch(lib):
    err = lib.hode_lstm_seq_last_error_string
    fwd, bwd, fill, ws = lib.hode_lstm_seq_fwd, lib.hode_lstm_seq_bwd, lib.hode_lstm_seq_fill_operand, lib.hode_lstm_seq_workspace_bytes
    for fn in (fwd, bwd, fill):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        assert fn(_desc(seq_len=0), None) == E_SIZE and b"T=0" in err()
        assert fn(_desc(a=None), None) == E_NULL and b"a is required" in err()
    for fn in (fwd, bwd):
        for H in (161, 200):   # the library's own refusal (check_lstm / lstm_geom): the sizes are libhode.so's
            assert fn(_desc(hidden_dim=H, grad_h_out=64, grad_gates=64, h_prev=64), None) == E_UNSUPPORTED
            assert b"hidden_dim %d exceeds the largest compiled kernel (160)" % H in err()
            assert ws(_desc(hidden_dim=H)) == 0
    need = ws(_desc())
    assert need > 0 and need == ws(_desc(save_tape=1)) > ws(_desc(save_tape=0)) > 0
    assert fwd(_desc(), None) == E_WORKSPACE and b"workspace 0 B < required %d B" % need in err()
    assert fwd(_desc(workspace=256, workspace_bytes=need - 1), None) == E_WORKSPACE and b"workspace %d B < required" % (need - 1) in err()
    assert bwd(_desc(save_tape=0), None) == E_UNSUPPORTED and b"hode_lstm_seq_bwd needs the tape" in err()
    assert bwd(_desc(grad_gates=64, h_prev=64), None) == E_NULL and b"grad_h_out / grad_gates / h_prev" in err()   # NULL grad_h_out
    full = dict(grad_h_out=64, grad_gates=64, h_prev=64)
    assert bwd(_desc(workspace=256, workspace_bytes=need - 1, **full), None) == E_WORKSPACE
    assert fill(_desc(), None) == E_NULL and b"h_prev must be non-NULL" in err()


def test_the_workspace_is_libhode_s_for_the_same_descriptor(lib):
    """The same host code sizes both: packed weights, and with a tape the packed W_hh^T and the tape."""
    import hode
    for H in (13, 16, 44, 160):
        for B in (21, 101, 8193):
            for tape in (0, 1):
                for nt in (0, 1, 2, 3, 4):
                    d = _desc(hidden_dim=H, batch=B, save_tape=tape, patient_tiles=nt)
                    assert lib.hode_lstm_seq_workspace_bytes(d) == hode.lib().hode_lstm_workspace_bytes(d) > 0
                    assert lib.hode_lstm_seq_workspace_bytes(d) == kv.lstm_workspace_bytes(4, B, 24, H, 23, bool(tape), nt)


# ----------------------------------------------------------------------------------------------- 4. what stays as it was
def test_libhode_keeps_its_entries_and_its_error_text():
    import hode
    assert hode.lib().hode_lstm_bwd(_desc(save_tape=0), None) == E_UNSUPPORTED
    assert b"hode_lstm_bwd needs the tape" in hode.lib().hode_last_error_string()
