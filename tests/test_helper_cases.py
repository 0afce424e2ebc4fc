"""CPU checks of tests/helper_cases.py, the tables tests/test_hip_helpers.py runs on the GPU:
(a) the numpy float32 restatement of every helper, its primitives rounded correctly and then moved by +-PRIM_ULP ulp,
    stays within bound(x) on the whole input set -- the bounds are proved here, not fitted to the device;
(b) restated mutants exceed the bound somewhere -- the bounds have teeth;
(c) every HODE_DEV function of hode_common.hpp and hode_lanes.hpp has a row in the probe table or a named exemption."""
import os
import re

import numpy as np
import pytest

import device_probe
import helper_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc")
UNARY = ("exp", "exp_full", "log", "tanh", "tanh_precise", "sigmoid", "sigmoid_gate", "tanh_scaled")
#: perfect primitives; +-k ulp with seeded signs; all up; all down
PERTURBATIONS = (dict(), dict(ulp=hc.PRIM_ULP, seed=1), dict(ulp=hc.PRIM_ULP, sign=1.0), dict(ulp=hc.PRIM_ULP, sign=-1.0))


def test_input_set():
    x = hc.unary_inputs()
    assert 2_000_000 < x.size < 3_000_000
    u = x.view(np.uint32)
    for b in (0, 0x80000000, 0x7f800000, 0xff800000, 1, 0x7fffff, 0x80000001, 0x807fffff, 0x00800000, 0x7f7fffff):
        assert (u == b).any(), hex(b)
    assert np.isnan(x).any()
    for e in range(1, 255):
        assert ((u >> 23) == e).sum() >= 4096 and ((u >> 23) == (e | 0x100)).sum() >= 4096
    for c in (0.625, -0.625, 88.72, -88.72, -87.34, -103.97, 1.0):
        assert np.isin(hc.around(c), x).all()
    a, b = hc.div_inputs()
    with np.errstate(all="ignore"):
        q, r = np.abs(a.astype(np.float64) / b), np.abs(1.0 / b.astype(np.float64))
    for cls in (q < hc.FLUSH, q > hc.FLT_MAX, r < hc.FLUSH, r > hc.FLT_MAX, hc.div_main(a, b)):
        assert cls.sum() > 1000


@pytest.mark.parametrize("name", UNARY)
def test_restatement_stays_within_the_bound(name):
    x = hc.unary_inputs()
    for kw in PERTURBATIONS:
        got = hc.RESTATE[name](x, hc.Prims(**kw))
        res = hc.check_unary(name, x, got)
        assert res["ratio"].size > 1_000_000 or name == "log"
        i = int(np.argmax(res["ratio"]))
        assert res["ratio"][i] <= 1.0, (name, kw, float(res["x"][i]), float(res["ratio"][i]), float(res["abs"][i]))


def test_div_restatement_stays_within_the_bound():
    a, b = hc.div_inputs()
    m = hc.div_main(a, b)
    assert m.sum() > 500_000
    for kw in PERTURBATIONS:
        got = hc.r_div(a[m], b[m], hc.Prims(**kw)).astype(np.float64)
        err = np.abs(got - a[m].astype(np.float64) / b[m].astype(np.float64))
        assert (err <= hc.bound_div(a[m], b[m])).all(), kw


def test_dpow_dp_restatement_stays_within_the_bound():
    x, p, xp = hc.dpow_inputs()
    m = x > 0
    for kw in PERTURBATIONS:
        got = hc.r_dpow_dp(x, p, xp, hc.Prims(**kw))
        assert (got[~m] == 0).all()
        err = np.abs(got[m].astype(np.float64) - xp[m].astype(np.float64) * np.log(x[m].astype(np.float64)))
        assert (err <= hc.bound_dpow_dp(x[m], p[m], xp[m])).all(), kw


@pytest.mark.parametrize("name", sorted(hc.EDGES))
def test_edge_table_is_the_mathematical_function(name):
    """The stated edge values are the float64 function's (NaN, +-inf, or within the bound), and the restated formula
    gives exactly them."""
    x = np.array([e[0] for e in hc.EDGES[name]], np.float32)
    want = np.array([e[1] for e in hc.EDGES[name]], np.float32)
    res = hc.check_unary(name, x, want)
    assert (res["ratio"] <= 1.0).all(), (name, res["x"][res["ratio"] > 1.0])
    got = hc.RESTATE[name](x, hc.Prims())
    assert hc.same_value(got, want).all(), [(float(a), float(g), float(w)) for a, g, w in zip(x, got, want)]


def test_div_edge_table_is_the_documented_one():
    a = np.array([e[0][0] for e in hc.DIV_EDGES], np.float32)
    b = np.array([e[0][1] for e in hc.DIV_EDGES], np.float32)
    want = np.array([e[1] for e in hc.DIV_EDGES], np.float32)
    hc.check_div(a, b, want)
    got = hc.r_div(a, b, hc.Prims())
    assert hc.same_value(got, want).all(), [(float(p), float(q), float(g), float(w)) for p, q, g, w in zip(a, b, got, want)]
    assert not hc.div_main(a, b)[np.isnan(want)].any()


def test_div_restatement_classes_everywhere():
    a, b = hc.div_inputs()
    for kw in PERTURBATIONS:
        err, bound = hc.check_div(a, b, hc.r_div(a, b, hc.Prims(**kw)))
        assert (err <= bound).all(), kw


def test_nextafter_restatement_is_numpy_nextafter():
    x = hc.unary_inputs()
    fin = np.isfinite(x)
    up, down = hc.r_nextafter_up(x), hc.r_nextafter_down(x)
    with np.errstate(all="ignore"):
        assert hc.same_value(up[fin], np.nextafter(x[fin], np.float32(np.inf))).all()
        assert hc.same_value(down[fin], np.nextafter(x[fin], np.float32(-np.inf))).all()


def test_unfused_and_fused_references_differ():
    a, b, c = hc.rn_inputs()
    unfused, fused = hc.rn_reference(a, b, c)
    assert (unfused != fused).mean() > 0.5


# ----------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("mutant", sorted(hc.MUTANTS))
def test_bound_catches_the_mutant(mutant):
    name, fn = hc.MUTANTS[mutant]
    x = hc.unary_inputs()
    x = x[hc.DOMAIN[name](x)]
    got = fn(x, hc.Prims()).astype(np.float64)
    ref = hc.REF[name](x)
    with np.errstate(all="ignore"):
        over = np.abs(got - ref) > hc.BOUND[name](x.astype(np.float64))
    assert (over & np.isfinite(ref) & np.isfinite(got)).sum() > 100, mutant


def test_bound_catches_div_without_the_newton_step():
    a, b = hc.div_inputs()
    m = hc.div_main(a, b)
    got = hc.r_div(a[m], b[m], hc.Prims(ulp=hc.PRIM_ULP, seed=2), newton=False).astype(np.float64)
    err = np.abs(got - a[m].astype(np.float64) / b[m].astype(np.float64))
    assert (err > hc.bound_div(a[m], b[m])).sum() > 100


def test_reference_catches_nextafter_up_ignoring_the_sign():
    x = hc.unary_inputs()
    x = x[np.isfinite(x)]
    bad = hc.r_nextafter_up(x, sign_aware=False)
    with np.errstate(all="ignore"):
        assert (~hc.same_value(bad, np.nextafter(x, np.float32(np.inf)))).sum() > 1_000_000


def test_lanemap_restatement_properties():
    """Every patient below B is live in exactly one slot (lpp lanes of it), idle lanes shadow a patient below B."""
    for lpp in (1, 4):
        for B in hc.LANEMAP_B:
            for ppw in hc.LANEMAP_PPW[lpp]:
                for block in hc.BLOCKS:
                    m = hc.lanemap(lpp, B, ppw, block, hc.grid_blocks(B, ppw, block))
                    live = m[m[:, 2] == 1]
                    assert np.array_equal(np.bincount(live[:, 0], minlength=B), np.full(B, lpp)), (lpp, B, ppw, block)
                    assert (m[:, 0] >= 0).all() and (m[:, 0] < B).all()


# -------------------------------------------------------------------------------------------------- coverage guard
def _hode_dev_functions(path):
    src = open(path).read()
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\bHODE_DEV\s+(?:[\w:<>\*&]+\s+)*?(\w+)\s*(?:<[^<>()]*>\s*)?\(", src))


def test_every_shared_device_helper_is_probed_or_exempt():
    found = _hode_dev_functions(os.path.join(CSRC, "hode_common.hpp")) | _hode_dev_functions(os.path.join(CSRC, "hode_lanes.hpp"))
    assert {"exp_f32", "vfma", "vsplat", "LaneMap", "store_vec", "wave_sum_patients", "quad_bcast", "add_rn"} <= found, sorted(found)
    assert not set(hc.PROBED) & set(hc.EXEMPT)
    missing = sorted(found - set(hc.PROBED) - set(hc.EXEMPT))
    assert not missing, "HODE_DEV functions without a probe row or an exemption: %s" % missing
    gone = sorted((set(hc.PROBED) | set(hc.EXEMPT)) - found)
    assert not gone, "rows for functions that no longer exist: %s" % gone
    assert all(len(reason) > 20 for reason in hc.EXEMPT.values())
    probe_src = open(os.path.join(CSRC, "probe", "hode_probe.hip")).read()
    for fn, ops in hc.PROBED.items():
        assert re.search(r"\b%s\b" % fn, probe_src), "the probe does not call %s" % fn
        for op in ops:
            assert op in device_probe.OPS or op in hc.ENTRY_POINTS, (fn, op)
            assert op in hc.ENTRY_POINTS or ("HODE_PROBE_OP_" + op.upper()) in probe_src, op
    # every op of the header is reached by the GPU test's tables
    tested = {op for ops in hc.PROBED.values() for op in ops} | {"prim_exp2", "prim_log2", "prim_rcp", "prim_sqrt", "sigmoid_gate"} \
        | {"tanh_scaled%d" % i for i in range(4)}
    unary_table = {"exp", "exp_full", "log", "tanh", "tanh_precise", "sigmoid", "sigmoid_gate", "tanh_scaled0"}
    for op, base in hc.SAME_BITS.items():     # a copy is held to its original's bits, the original to float64
        assert op in device_probe.OPS and base in unary_table, (op, base)
    assert {"tanh_scaled", "tanh_scaled4", "sigmoid2", "sigmoid4", "tanh4"} <= found
    assert set(device_probe.OPS) == tested - set(hc.ENTRY_POINTS), sorted(set(device_probe.OPS) ^ (tested - set(hc.ENTRY_POINTS)))


def test_probe_library_is_a_test_library_only():
    """A row of the build table like any other, with the product flags; nothing under hode/ names it."""
    import build_hip
    row = build_hip.LIBRARIES[device_probe.FILE_NAME]
    assert row.header == "include/hode_probe.h" and row.src_dir == build_hip.PKG + "/csrc/probe"
    assert [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()] == \
        [("hode_probe", row.src_dir + "/hode_probe.hip", [])]
    hode_dir = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "hode")
    for fn in os.listdir(hode_dir):
        if fn.endswith(".py"):
            assert "hode_probe" not in open(os.path.join(hode_dir, fn)).read(), fn
    # the digest follows every header the unit includes
    src = open(os.path.join(ROOT, row.src_dir, "hode_probe.hip")).read()
    hashed = set(build_hip.digest_files(device_probe.FILE_NAME))
    assert {build_hip.PKG + "/csrc/hode_common.hpp", build_hip.PKG + "/csrc/hode_lanes.hpp"} <= hashed   # the helpers it probes
    for inc in re.findall(r'#include "([^"]+)"', src):
        rel = os.path.normpath(os.path.join(row.src_dir, inc)).replace(os.sep, "/")
        assert rel in hashed, rel
