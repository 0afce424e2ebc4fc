"""The shared device helpers of csrc/hode_common.hpp and csrc/hode_lanes.hpp (and sigmoid_gate, NeuralMf::tanh_scaled,
dpow_dp), each run on its own through the test-only libhode_probe.so and compared with float64 on the input sets, bounds
and edge tables of tests/helper_cases.py; the bit-exact helpers against their float32 restatements.

Every accuracy test prints, per sub-domain, the largest err / bound, absolute error and ulp error before it asserts (run
with -s to see them; DESIGN.md section 10 records the values)."""
import numpy as np
import pytest

import helper_cases as hc

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def probe():
    import device_probe
    return device_probe.Probe()


# ------------------------------------------------------------------------------------------------------ primitives
def _prim_domain(name, x, ref):
    """Normal operand and normal result (PRIM_ULP's domain)."""
    ok = np.isfinite(x) & (np.abs(x) >= f32(hc.FLUSH)) & np.isfinite(ref) & (np.abs(ref) >= hc.FLUSH) & (np.abs(ref) <= hc.FLT_MAX)
    if name in ("log2", "sqrt"):
        ok &= x > 0
    if name == "log2":
        ok |= x == 1      # log2(1) = 0 exactly
    if name == "exp2":
        ok |= (np.abs(x) < f32(hc.FLUSH))   # 2^x = 1 for a tiny operand
    return ok


@pytest.mark.parametrize("name", ("exp2", "log2", "rcp", "sqrt"))
def test_primitive_stays_within_its_measured_constant(probe, name):
    x = hc.unary_inputs()
    got = probe.map("prim_" + name, x)
    with np.errstate(all="ignore"):
        ref = hc.REF["prim_" + name](x)
        m = _prim_domain(name, x, ref)
        err = np.abs(got[m].astype(f64) - ref[m]) / hc.ulp32(ref[m])
    i = int(np.argmax(err))
    print("\nprim %-5s n = %d  max ulp = %.4f at x = %.9g (constant %.1f)" % (name, m.sum(), err[i], x[m][i], hc.PRIM_ULP[name]))
    assert np.isfinite(got[m]).all()
    # outside the domain: what HW_FLUSH and the edge rows state
    sub_in = np.isfinite(x) & (x != 0) & (np.abs(x) < f32(hc.FLUSH))
    with np.errstate(all="ignore"):
        sub_out = np.isfinite(ref) & (ref != 0) & (np.abs(ref) < hc.FLUSH) & ~sub_in
    for label, mm in (("subnormal operand", sub_in), ("subnormal result", sub_out)):
        if mm.any():
            g = got[mm]
            print("prim %-5s %-18s n = %d: zeros %d, infs %d, nans %d, max |got - ref| = %.3e" % (
                name, label, mm.sum(), (g == 0).sum(), np.isinf(g).sum(), np.isnan(g).sum(),
                np.nanmax(np.where(np.isfinite(g), np.abs(g.astype(f64) - ref[mm]), 0.0))))
    assert err[i] <= hc.PRIM_ULP[name]
    if name == "exp2":
        if hc.HW_FLUSH["exp2_out"]:
            assert (got[sub_out] == 0).all()
        assert (np.abs(got[sub_out].astype(f64) - ref[sub_out]) <= hc.FLUSH).all()
        assert (got[x >= 128] == np.inf).all() and (got[x <= -150] == 0).all() and np.isnan(got[np.isnan(x)]).all()
    if name == "log2":
        if hc.HW_FLUSH["log2_in"]:
            assert (got[sub_in & (x > 0)] == -np.inf).all()
        assert (got[x == 0] == -np.inf).all() and np.isnan(got[x < -f32(hc.FLUSH)]).all() and (got[x == np.inf] == np.inf).all()
    if name == "rcp":
        if hc.HW_FLUSH["rcp_in"]:
            assert np.array_equal(got[sub_in], np.copysign(f32(np.inf), x[sub_in]))
        if hc.HW_FLUSH["rcp_out"]:
            assert (got[sub_out] == 0).all()
        assert (np.abs(got[sub_out].astype(f64) - ref[sub_out]) <= hc.FLUSH).all()
        assert np.array_equal(got[x == 0], np.copysign(f32(np.inf), x[x == 0])) and (got[np.isinf(x)] == 0).all()
    if name == "sqrt":
        s = sub_in & (x > 0)
        assert (np.abs(got[s].astype(f64) - ref[s]) <= hc.PRIM_ULP[name] * hc.ulp32(ref[s])).all()
        assert np.isnan(got[x <= -f32(hc.FLUSH)]).all() and (got[x == 0] == 0).all() and (got[x == np.inf] == np.inf).all()


# --------------------------------------------------------------------------------------------------- unary helpers
UNARY = (("exp", "exp", "exp"), ("exp_full", "exp_full", "exp_full"), ("log", "log", "log"), ("tanh", "tanh", "tanh"), ("tanh_precise", "tanh_precise", "tanh_precise"),
         ("sigmoid", "sigmoid", "sigmoid"), ("sigmoid_gate", "sigmoid_gate", "sigmoid_gate"),
         ("tanh_scaled0", "tanh_scaled", "tanh_scaled"))


@pytest.mark.parametrize("op,name,ref", UNARY, ids=[u[0] for u in UNARY])
def test_unary_helper_against_fp64(probe, op, name, ref):
    x = hc.unary_inputs()
    got = probe.map(op, x)
    res = hc.check_unary(name, x, got, ref)
    print()
    for line in hc.report(name, res):
        print(line)
    i = int(np.argmax(res["ratio"]))
    assert res["ratio"][i] <= 1.0, (name, float(res["x"][i]), float(res["ratio"][i]), float(res["abs"][i]))
    ex = np.array([e[0] for e in hc.EDGES[name]], f32)
    want = np.array([e[1] for e in hc.EDGES[name]], f32)
    edge = probe.map(op, ex)
    assert hc.same_value(edge, want).all(), [(float(a), float(g), float(w)) for a, g, w in zip(ex, edge, want)]


@pytest.mark.parametrize("op", sorted(hc.SAME_BITS))
def test_copy_of_a_formula_has_the_bits_of_its_original(probe, op):
    """The packed tanh_f32, tanh4, every scaled tanh (tanh_scaled on float and f2, tanh_scaled4, the slots of
    NeuralMf::tanh_scaled) and sigmoid2 / sigmoid4 equal, bit for bit on the whole input set, the scalar helper that the
    float64 tests hold to its bound."""
    x = hc.unary_inputs()
    assert hc.same_value(probe.map(op, x), probe.map(hc.SAME_BITS[op], x)).all(), op


def test_exp_full_is_exp_inside_its_domain(probe):
    """exp_full_f32 is bit for bit exp_f32 wherever |x log2(e)| < 128: the two differ only in the factor chosen beyond it."""
    x = hc.unary_inputs()
    x = x[~hc.RESTRICTED["exp"](x)]
    assert x.size > 1_500_000 and hc.same_value(probe.map("exp_full", x), probe.map("exp", x)).all()


def test_scaled_tanh_is_tanh_f32_at_the_scaled_argument(probe):
    """tanh_f32(x) == tanh_scaled(fl(x * 2 log2 e)): the scaled form is tanh_f32's own exp2 / rcp / fma chain."""
    z = hc.unary_inputs()
    x = z[np.isfinite(z) & (np.abs(z) < 64)]
    zz = (x * hc.C2).astype(f32)
    assert hc.same_value(probe.map("tanh", x), probe.map("tanh_scaled0", zz)).all()


@pytest.mark.parametrize("op,restate,target", (("nextafter_up", hc.r_nextafter_up, np.inf), ("nextafter_down", hc.r_nextafter_down, -np.inf)))
def test_nextafter_is_numpy_nextafter(probe, op, restate, target):
    x = hc.unary_inputs()
    got = probe.map(op, x)
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        assert hc.same_value(got[fin], np.nextafter(x[fin], f32(target))).all()
    # outside "finite x": the bit arithmetic, as restated (nextafter_up(+inf) is a NaN, nextafter_up(-inf) = -FLT_MAX)
    assert np.array_equal(got[~fin].view(np.uint32), restate(x[~fin]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ binary / ternary
def test_div_against_fp64(probe):
    """The derived bound inside the main domain; everywhere else the documented classes (hc.check_div)."""
    a, b = hc.div_inputs()
    got = probe.map("div", a, b)
    m = hc.div_main(a, b)
    err, bound = hc.check_div(a, b, got)
    i = int(np.argmax(err / bound))
    with np.errstate(all="ignore"):
        q = a[m].astype(f64) / b[m].astype(f64)
    print("\ndiv            main domain        n = %8d  max err/bound = %.3f (a = %.9g, b = %.9g)  max ulp = %.3f" % (
        m.sum(), err[i] / bound[i], a[m][i], b[m][i], (err / hc.ulp32(q)).max()))
    print("div            outside            n = %8d  NaN %d, inf %d, zero %d" % (
        (~m).sum(), np.isnan(got[~m]).sum(), np.isinf(got[~m]).sum(), (got[~m] == 0).sum()))
    assert err[i] <= bound[i]
    ea = np.array([e[0][0] for e in hc.DIV_EDGES], f32)
    eb = np.array([e[0][1] for e in hc.DIV_EDGES], f32)
    want = np.array([e[1] for e in hc.DIV_EDGES], f32)
    edge = probe.map("div", ea, eb)
    assert hc.same_value(edge, want).all(), [(float(p), float(r), float(g), float(w)) for p, r, g, w in zip(ea, eb, edge, want)]


def test_mul_rn_add_rn_resist_contraction(probe):
    a, b, c = hc.rn_inputs()
    unfused, fused = hc.rn_reference(a, b, c)
    assert (unfused != fused).mean() > 0.5
    got = probe.map("mul_add_rn", a, b, c)
    assert np.array_equal(got.view(np.uint32), unfused.view(np.uint32))


def test_dpow_dp_against_fp64(probe):
    x, p, xp = hc.dpow_inputs()
    got = probe.map("dpow_dp", x, p, xp)
    m = x > 0
    assert (x[~m] == 0).all() and (p[~m] >= 0).all() and (got[~m] == 0).all()   # torch: zero where x == 0 and p >= 0
    ref = xp[m].astype(f64) * np.log(x[m].astype(f64))
    err = np.abs(got[m].astype(f64) - ref)
    bound = hc.bound_dpow_dp(x[m], p[m], xp[m])
    print("\ndpow_dp        n = %d  max err/bound = %.3f  max ulp = %.3f" % (m.sum(), (err / bound).max(), (err / hc.ulp32(ref)).max()))
    assert (err <= bound).all()
    neg = probe.map("dpow_dp", np.zeros(64, f32), np.full(64, -1.5, f32), np.full(64, np.inf, f32))
    assert (neg == -np.inf).all()    # x == 0, p < 0: inf * log(0)


# ------------------------------------------------------------------------------------------------- cross-lane ops
@pytest.mark.parametrize("block", hc.BLOCKS)
@pytest.mark.parametrize("op", sorted(hc.WAVE_OPS))
def test_cross_lane_op_bit_for_bit(probe, op, block):
    """Every lane against its own restated order.  3 waves at block 64; 4 at block 256 (one block)."""
    v = hc.wave_inputs(3 if block == 64 else 4)
    got = probe.wave(op, v, block)
    want = hc.WAVE_OPS[op](v)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:16]
    # the summation order matters on these values: the float64 sum differs from the float32 chain somewhere
    if "sum" in op:
        exact = hc.WAVE_OPS[op](v.astype(f64))
        assert (exact.astype(f32) != want).any()
    # lanes the comments promise one common value to
    g = got.view(np.uint32)
    if op in ("quad_sum",) or op.startswith("quad_bcast"):
        assert (g.reshape(-1, 4) == g.reshape(-1, 4)[:, :1]).all()
    if op in ("wave_sum", "wave_sum_patients1"):
        assert (g.reshape(-1, 64) == g.reshape(-1, 64)[:, :1]).all()
    if op in ("wave_sum_stride4", "wave_sum_patients4"):
        w = g.reshape(-1, 16, 4)
        assert (w == w[:, :1, :]).all()


def test_row_sums_differ_between_lanes_only_in_rounding(probe):
    """row_sum and row_sum_stride4 add in a rotated order per lane: each lane holds the sum of its group, but not
    bit-identical across lanes.  No caller may branch on the value (hode_common.hpp says so)."""
    v = hc.wave_inputs(3)
    for op, restate, group in (("row_sum", hc.w_row_sum, 16), ("row_sum_stride4", hc.w_row_sum_stride4, 4)):
        got = probe.wave(op, v, 64).astype(f64)
        exact = restate(v.astype(f64))
        scale = restate(np.abs(v).astype(f64))
        assert (np.abs(got - exact) <= (group - 1) * hc.U * scale).all(), op


# ---------------------------------------------------------------------------------------- lane map and round trip
def _geometries():
    for lpp in (4, 1):
        for B in hc.LANEMAP_B:
            for ppw in hc.LANEMAP_PPW[lpp]:
                for block in hc.BLOCKS:
                    yield lpp, B, ppw, block


@pytest.mark.parametrize("lpp", (4, 1))
def test_lanemap_against_restatement(probe, lpp):
    for l, B, ppw, block in _geometries():
        if l != lpp:
            continue
        nb = hc.grid_blocks(B, ppw, block) + 1     # one block past the grid: all idle
        got = probe.lanemap(lpp, B, ppw, block, nb)
        want = hc.lanemap(lpp, B, ppw, block, nb)
        assert np.array_equal(got, want), (lpp, B, ppw, block, np.flatnonzero((got != want).any(axis=1))[:8])
        live = got[got[:, 2] == 1]
        assert np.array_equal(np.bincount(live[:, 0], minlength=B), np.full(B, lpp)), (lpp, B, ppw, block)
        assert sorted(set(live[:, 1])) == list(range(lpp))
        assert (got[:, 0] >= 0).all() and (got[:, 0] < B).all()     # idle lanes shadow a patient below B


@pytest.mark.parametrize("D", hc.ROUNDTRIP_D)
@pytest.mark.parametrize("lpp", (4, 1))
def test_load_store_round_trip(probe, D, lpp):
    """store_vec writes every row exactly as load_vec read it and nothing else, tail waves with idle quads included.  In the
    probe every lane that must not store (an idle lane, which shadows a live patient's row; a lane with q != 0 when
    D % 4 != 0) holds values no source row has, so a store without the `live` or `q == 0` gate lands in dst and fails the
    comparison; the guard bands catch a store outside [B][D].  With a gate removed a poisoned lane and a live lane of one
    wave store to the same address in one instruction, and the detection rests on the poisoned store being the one that
    stays (in practice the higher lane, which the idle lanes are); a side buffer counting writes would not depend on that."""
    sentinel = -12345.0
    for B, ppw, block in ((1, 1, 64), (5, 3, 64), (65, hc.LANEMAP_PPW[lpp][2], 256), (161, hc.LANEMAP_PPW[lpp][3], 64), (161, 10, 256)):
        src = (np.arange(B * D, dtype=f32) + 1.0).reshape(B, D)
        buf = probe.roundtrip(D, lpp, B, ppw, block, src, sentinel)
        guard = (len(buf) - B * D) // 2
        assert (buf[:guard] == sentinel).all() and (buf[guard + B * D:] == sentinel).all(), (D, lpp, B, ppw, block)
        assert np.array_equal(buf[guard:guard + B * D].reshape(B, D), src), (D, lpp, B, ppw, block)
