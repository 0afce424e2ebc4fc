"""Guard (no GPU) for the metric kernels' case tables (tests/metric_cases.py): the restated CRPS host rules are pinned to
csrc/hode_crps.hip, no shape the host accepts needs more LDS than a CU has (dynamic, as the host computes it, plus the
static LDS in the kernel's descriptor), and the tables reach every regime and edge they are meant to."""
import glob
import os
import re
import struct
import sys

import pytest

import metric_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc")
BUILD = os.path.join(CSRC, "build")
sys.path.insert(0, os.path.join(ROOT, "tools"))

CU_LDS = 160 * 1024  # gfx950: 160 KiB of LDS per CU, the most one workgroup can hold


def _norm(x):
    return " ".join(x.split())


def _crps_source():
    src = open(os.path.join(CSRC, "hode_crps.hip")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return _norm(re.sub(r"//[^\n]*", "", src))


def _host_lds_rule(src):
    """The host's LDS expression and refusal bound, read out of the source and evaluated as Python:
    (M, Dv, weighted) -> bytes, and the bound in bytes."""
    m = re.search(r"const size_t lds = (.*?);", src)
    expr = m.group(1)
    expr = expr.replace("sizeof(float)", "4").replace("(size_t)", "").replace("hode::kCrpsThreads", "128")
    expr = re.sub(r"\(a\.w \? (.*?) : 0\)", r"((\1) if w else 0)", expr)
    expr = expr.replace("a.M", "M").replace("a.Dv", "Dv").replace("/", "//")
    fn = eval("lambda M, Dv, w: " + expr)  # noqa: S307  (the repository's own source)
    bound = re.search(r"if \(lds > (\d+) \* 1024\) return hode::fail\(HODE_E_UNSUPPORTED", src)
    return fn, int(bound.group(1)) * 1024


def test_crps_source_pins_the_restated_rules():
    """The lines mc.crps_lds_bytes / crps_accepts / crps_regime restate, as they read in the source."""
    s = _crps_source()
    assert "constexpr int kCrpsThreads = 128;" in s
    assert ("if (d->obs_dim > hode::kCrpsThreads || d->n_members > 128 || d->latent_dim > 128) "
            "return hode::fail(HODE_E_UNSUPPORTED,") in s
    assert "if (!d->w && d->latent_dim < d->obs_dim) return hode::fail(HODE_E_SIZE," in s
    assert ("const size_t lds = sizeof(float) * ((size_t)a.M * a.Dv + (a.w ? (size_t)a.Dv * hode::kCrpsThreads : 0) + "
            "(size_t)a.M * hode::kCrpsThreads + hode::kCrpsThreads / 64);") in s
    assert 'if (lds > 160 * 1024) return hode::fail(HODE_E_UNSUPPORTED, "needs %zu B of LDS", lds);' in s
    assert "if (lds > 64 * 1024) if (int e = hode::hip_fail(hipFuncSetAttribute(" in s
    fn, bound = _host_lds_rule(s)
    assert bound == mc.CRPS_LDS_LIMIT
    for M in range(1, 129):
        for Dv in range(1, 129):
            for ro in ("identity", "affine"):
                assert fn(M, Dv, ro != "identity") == mc.crps_lds_bytes(M, Dv, ro), (M, Dv, ro)


def test_crps_restated_acceptance_at_the_boundary():
    for M, Dv in mc.CRPS_LARGEST:
        assert mc.crps_accepts(M, Dv, 128 if Dv >= 128 else Dv, "affine")
        assert mc.crps_accepts(M, Dv, 8, "linear")
    for M, Dv in mc.CRPS_REFUSED:
        assert not mc.crps_accepts(M, Dv, 8, "affine") and not mc.crps_accepts(M, Dv, 8, "linear")
    # each of the three is maximal: one more member or one more latent component is refused
    for M, Dv in mc.CRPS_LARGEST:
        assert M == 128 or not mc.crps_accepts(M + 1, Dv, 8, "affine")
        assert Dv == 128 or not mc.crps_accepts(M, Dv + 1, 8, "affine")
    assert mc.crps_accepts(128, 128, 128, "identity")


@pytest.fixture(scope="module")
def crps_static_lds():
    """group_segment_fixed_size (the first dword of the kernel descriptor) of hode::crps_kernel, read from the object that
    build_hip.py compiled (like the kernel-variant guard, this relies on a current build: an object older than its source
    fails here rather than being read)."""
    obj = os.path.join(BUILD, "hode_crps.o")
    if not glob.glob(obj):
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    src = os.path.join(CSRC, "hode_crps.hip")
    assert os.path.getmtime(obj) >= os.path.getmtime(src), "hode_crps.o is older than hode_crps.hip: run build_hip.py"
    from kernel_descriptor import kernel_descriptors
    import kernel_variants as kv
    kds = [kd for dem, kd in kernel_descriptors(obj) if kv.kernel_name(dem) == "hode::crps_kernel"]
    assert kds and all(kd == kds[0] for kd in kds)  # a symbol may be listed by more than one symbol table
    return struct.unpack_from("<I", kds[0], 0)[0]


def test_no_accepted_crps_shape_needs_more_lds_than_a_cu_has(crps_static_lds):
    """Dynamic LDS as the host computes it (its own expression, read from the source) plus the kernel's static LDS, over
    every shape the host lets through: at most 160 KiB."""
    fn, bound = _host_lds_rule(_crps_source())
    worst = max((fn(M, Dv, w), M, Dv, w) for M in range(1, 129) for Dv in range(1, 129) for w in (False, True)
                if fn(M, Dv, w) <= bound)
    assert worst[0] + crps_static_lds <= CU_LDS, (
        "(M, Dv, readout) = %r is accepted with %d B dynamic + %d B static LDS > %d" % (
            worst[1:], worst[0], crps_static_lds, CU_LDS))


# --------------------------------------------------------------------------------------------------------- reach
def _substantive(c):
    return c["Tn"] > 1 and c["B"] > 1


def test_crps_table_is_well_formed():
    ids = [mc.crps_id(c) for c in mc.CRPS_CASES]
    assert len(ids) == len(set(ids))
    for c in mc.CRPS_CASES:
        assert mc.crps_accepts(c["M"], c["Dv"], c["obs"], c["readout"]), mc.crps_id(c)
        assert c["readout"] in mc.READOUTS and c["out"] in mc.OUTPUTS and c["layout"] in mc.LAYOUTS
        assert c["values"] in mc.VALUES
        if c["values"] in ("truth_member", "zero_spread", "offset"):
            assert c["readout"] == "identity", mc.crps_id(c)  # exact fp32 member values
        if c["values"] == "truth_member":
            assert c["M"] >= 3


def test_crps_table_reaches_every_regime_and_edge():
    cs = mc.CRPS_CASES
    sub = [c for c in cs if _substantive(c)]
    assert {mc.crps_regime(c) for c in sub} == {"small", "attr"}
    for M, Dv in mc.CRPS_LARGEST:
        assert any((c["M"], c["Dv"]) == (M, Dv) and c["readout"] != "identity" for c in sub), (M, Dv)
    assert {1, 63, 64, 65, 127, 128} <= {c["obs"] for c in cs}
    # crps_sum: a partial first wave, exactly one wave, and the second wave's partial (red[1])
    summing = [c for c in sub if c["out"] in ("sum", "both")]
    assert any(c["obs"] < 64 for c in summing) and any(c["obs"] == 64 for c in summing)
    assert any(64 < c["obs"] < 128 for c in summing) and any(c["obs"] == 128 for c in summing)
    assert any(c["readout"] == "identity" and c["obs"] == c["Dv"] for c in sub)
    assert {1, 2, 50, 64, 127, 128} <= {c["M"] for c in cs}
    assert {1, 128} <= {c["Dv"] for c in cs}
    assert any(c["Tn"] * c["B"] > 65535 and c["B"] % 2 == 1 and c["B"] % 3 and c["B"] % 5 for c in cs)
    assert set(mc.READOUTS) == {c["readout"] for c in sub}
    assert set(mc.OUTPUTS) == {c["out"] for c in sub}
    assert set(mc.LAYOUTS) == {c["layout"] for c in sub}
    assert set(mc.VALUES) == {c["values"] for c in sub}
    # the bias path under both outputs; every layout at more than 64 KiB or one of the largest shapes somewhere
    assert any(c["readout"] == "affine" and c["out"] == "both" and c["obs"] > 64 for c in sub)
    # the calls the product makes: evaluate (M = 50) / evaluate_horizon (M = 10) per sim config, and crps_z0
    for obs, D in mc.SIM_SHAPES:
        for M in mc.SIM_MEMBERS:
            assert any((c["obs"], c["Dv"], c["M"], c["readout"], c["out"], c["layout"]) ==
                       (obs, D, M, "affine", "sum", "member") and _substantive(c) for c in cs), (obs, D, M)
        assert any(c["Tn"] == 1 and c["readout"] == "identity" and c["obs"] == mc.EXPERT_DIM and c["Dv"] == D and
                   c["M"] in mc.SIM_MEMBERS and c["B"] > 1 for c in cs), D


def test_mckl_table_reaches_every_regime_and_edge():
    cs = mc.MCKL_CASES
    ids = [mc.mckl_id(c) for c in cs]
    assert len(ids) == len(set(ids))
    rows = {c["rows"] for c in cs}
    assert {1, 255, 256, 257} <= rows
    assert any(r > (1 << 20) and r % 256 for r in rows)
    assert {1, 2, 17, 100, 1000} <= {c["S"] for c in cs}
    assert {100.0, 1.0, 0.5} <= {c["rate"] for c in cs}
    assert set(mc.CLAMPS) == {c["clamp"] for c in cs}
    assert mc.CLAMPS["eps"] == 2.0 ** -23
    assert min(c["lv"][0] for c in cs) <= -20 and max(c["lv"][1] for c in cs) >= 4
    assert {"positive", "clamped", "mix", "zero"} == {c["mu"] for c in cs}
    assert {"both", "mu", "lv", "none"} == {c["grads"] for c in cs}
    # z = 0 exactly, with the gradient that tells the branches apart asked for, at a clamp value != rate
    assert any(c["mu"] == "zero" and c["grads"] in ("both", "mu") for c in cs)
    # the clamped branch's d/dlog_var asked for on all-clamped draws; the forward-only path at the large size
    assert any(c["mu"] == "clamped" and c["grads"] in ("both", "lv") for c in cs)
    assert any(c["rows"] > (1 << 20) and c["grads"] == "none" for c in cs)
    assert any(c["rows"] > (1 << 20) and c["grads"] == "both" for c in cs)
