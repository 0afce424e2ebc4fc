"""The tables behind tests/test_hip_helpers.py (GPU) and tests/test_helper_cases.py (CPU): for every shared device helper of
csrc/hode_common.hpp and csrc/hode_lanes.hpp (and sigmoid_gate, NeuralMf::tanh_scaled, dpow_dp, which are built on them)

  * the deterministic input set (unary_inputs, div_inputs, ...),
  * the float64 reference of the mathematical function (REF),
  * a numpy float32 restatement of the helper's formula over replaceable hardware primitives (RESTATE, Prims),
  * a pointwise error bound evaluated in float64 (BOUND), derived to first order from PRIM_ULP and half an ulp per float32
    rounding, with a commented allowance for the dropped higher-order terms and no free multiplier,
  * the value the helper must return on every non-finite or out-of-range class (EDGES), and
  * the restated mutants that the bounds must catch (MUTANTS).

numpy's float64 functions are good to about 1e-16 relative, 1e-9 of the float32 errors measured here.

PRIM_ULP holds the measured maxima of the four hardware primitives on the unary input set, in ulp of the float64 result,
each rounded up to the next half ulp (DESIGN.md section 10 names the run).  The GPU test asserts that they still hold."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24            # unit roundoff: a float32 rounding moves a normal value by at most U |value| (half an ulp)
FLUSH = 2.0 ** -126       # smallest normal: what flushing one subnormal primitive operand or result to zero can cost
FLT_MAX = float(np.finfo(f32).max)
OVERFLOW = 2.0 ** 128 * (1 - 2.0 ** -25)   # values of at least this magnitude round to +-inf

#: measured on an MI355X (see the module docstring), rounded up to the next half ulp; domain: normal operand AND normal result
PRIM_ULP = {"exp2": 1.0, "log2": 1.0, "rcp": 1.0, "sqrt": 0.5}
#: what the primitives do outside that domain, as measured in the same run and asserted by the GPU test
#:   exp2: a result below 2^-126 is flushed to 0                     log2: a subnormal operand is read as 0 (-> -inf)
#:   rcp:  a subnormal operand is read as 0 (-> +-inf), and a result below 2^-126 is flushed to +-0
HW_FLUSH = {"exp2_out": True, "log2_in": True, "rcp_in": True, "rcp_out": True}

L2E = f32(1.4426950408889634)
LN2F = f32(0.6931471805599453)
C2 = f32(2.885390081777927)
LOG2E = 1.0 / np.log(2.0)
LN2 = float(np.log(2.0))
PRECISE_BRANCH = f32(0.625)
PRECISE_COEF = tuple(f32(c) for c in (-0.005508354399353266, 0.020461998879909515, -0.05368518456816673,
                                      0.13330785930156708, -0.3333325684070587))


def quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return wrapped


def ulp32(v):
    """The float32 spacing at the float64 magnitude |v| (2^-149 below the smallest normal)."""
    _, e = np.frexp(np.abs(np.asarray(v, f64)))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def with_final_rounding(ref, b):
    """b plus the final float32 rounding: half an ulp at the largest magnitude the unrounded result can have, |ref| + b."""
    return b + 0.5 * ulp32(np.abs(ref) + b)


def bits(u):
    return np.asarray(u, np.uint32).view(f32)


# ------------------------------------------------------------------------------------------------------------ inputs
def around(x, k=2000):
    """The 2k + 1 consecutive floats centred on float32(x); around 0: the k smallest magnitudes of both signs and +-0."""
    c = int(np.asarray(x, f32).view(np.uint32))
    if c & 0x7fffffff == 0:
        m = np.arange(0, k + 1, dtype=np.uint32)
        return bits(np.concatenate([m, m | np.uint32(0x80000000)]))
    return bits((np.int64(c) + np.arange(-k, k + 1)).astype(np.uint32))


def _binade_crossings():
    """Where exp(2x) + 1 (tanh), exp(-x) + 1 (sigmoid_gate) and 2^z + 1 (tanh_scaled) reach a power of two."""
    k = np.arange(2, 25, dtype=f64)
    p = np.log(2.0 ** k - 1.0)
    pts = np.concatenate([0.5 * p, p, p * LOG2E])
    return np.concatenate([pts, -pts])


@functools.lru_cache(maxsize=None)
def unary_inputs():
    """About 2.7 million floats: per sign and normal exponent both ends of the binade and 4094 seeded mantissas; every
    subnormal power of two, the smallest and largest subnormal, +-0, +-inf, NaN; +-2000 ulp around every point where a
    formula changes behaviour."""
    rng = np.random.default_rng(20211206)
    mant = rng.integers(0, 1 << 23, size=(2, 254, 4094), dtype=np.uint32)
    ends = np.broadcast_to(np.array([0, 0x7fffff], np.uint32), (2, 254, 2))
    mant = np.concatenate([ends, mant], axis=2)
    sign = (np.arange(2, dtype=np.uint32) << 31)[:, None, None]
    expo = (np.arange(1, 255, dtype=np.uint32) << 23)[None, :, None]
    parts = [bits((sign | expo | mant).ravel())]
    sub = np.concatenate([np.uint32(1) << np.arange(23, dtype=np.uint32), np.array([1, 0x7fffff, 0, 0x7f800000], np.uint32)])
    parts.append(bits(np.concatenate([sub, sub | np.uint32(0x80000000), np.array([0x7fc00000], np.uint32)])))
    for x in (0.0, 0.625, -0.625, 88.72, -88.72, -87.34, -103.97, 1.0):
        parts.append(around(x))
    for x in _binade_crossings():
        parts.append(around(x))
    out = np.concatenate(parts)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def div_inputs():
    """(a, b): exponents of both spread over the whole range (seeded), plus the classes where 1/b or a/b is subnormal or
    overflows, and the non-finite and zero divisors."""
    rng = np.random.default_rng(7)
    n = 1 << 20
    a = bits(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    b = bits(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    # the main domain, dense: moderate exponents
    m = 1 << 19
    a2 = (rng.standard_normal(m) * 2.0 ** rng.integers(-40, 40, m)).astype(f32)
    b2 = (rng.standard_normal(m) * 2.0 ** rng.integers(-40, 40, m)).astype(f32)
    mag = f32(2.0) ** np.arange(-149, 128, dtype=f32)
    ea, eb = np.meshgrid(mag, mag)
    ea, eb = (ea.ravel() * f32(1.2345)).astype(f32), (eb.ravel() * f32(-1.7654)).astype(f32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -3.0, FLT_MAX, 2.0 ** -126, 2.0 ** -149], f32)
    sa, sb = np.meshgrid(sp, sp)
    a = np.concatenate([a, a2, ea, sa.ravel()])
    b = np.concatenate([b, b2, eb, sb.ravel()])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def rn_inputs():
    """(a, b, c) with c close to -a b, so that the unfused fl(fl(a b) + c) differs from fma(a, b, c): the fused form keeps
    the low half of the product that the rounded product drops."""
    rng = np.random.default_rng(11)
    n = 1 << 16
    a = (1.0 + rng.random(n)).astype(f32) * f32(2.0) ** rng.integers(-20, 20, n).astype(f32)
    b = (1.0 + rng.random(n)).astype(f32) * f32(2.0) ** rng.integers(-20, 20, n).astype(f32)
    p = (a.astype(f64) * b.astype(f64)).astype(f32)
    c = -np.nextafter(p, np.where(rng.random(n) < 0.5, f32(0), f32(np.inf))).astype(f32)
    c[::4] = -p[::4]
    return a, b, c


def rn_reference(a, b, c):
    """(fl(fl(a b) + c), fma(a, b, c)), both exact: a b is exact in float64, and c is within an ulp of -a b, so the sums are."""
    p = a.astype(f64) * b.astype(f64)
    return (p.astype(f32).astype(f64) + c.astype(f64)).astype(f32), (p + c.astype(f64)).astype(f32)


@functools.lru_cache(maxsize=None)
def dpow_inputs():
    rng = np.random.default_rng(13)
    n = 1 << 16
    x = np.exp(rng.uniform(-20, 20, n)).astype(f32)
    p = rng.uniform(-3, 3, n).astype(f32)
    xp = np.power(x.astype(f64), p.astype(f64)).astype(f32)
    x[:8] = 0.0
    p[:8] = (0.0, 1.0, 2.5, -0.0, 3.0, 2.0, 0.5, 1e-3)
    xp[:8] = np.power(0.0, p[:8].astype(f64)).astype(f32)
    return x, p, xp


def wave_inputs(n_waves=3):
    """n_waves * 64 values whose exponents span 40 binades, signs mixed: the summation order shows in the last bits."""
    rng = np.random.default_rng(3)
    n = 64 * n_waves
    return ((1.0 + rng.random(n)) * 2.0 ** rng.integers(-20, 21, n) * rng.choice([-1.0, 1.0], n)).astype(f32)


# ----------------------------------------------------------------------------------------- the hardware primitives
class Prims:
    """Stand-ins for v_exp_f32, v_log_f32, v_rcp_f32: the correctly rounded float64 result, optionally moved by +-k ulp
    (`ulp`: {name: k}, signs seeded or all `sign`) while staying within k ulp of the exact value; outside the normal range
    they flush as HW_FLUSH says."""

    def __init__(self, ulp=None, seed=0, sign=None):
        self.ulp, self.rng, self.sign = ulp or {}, np.random.default_rng(seed), sign

    @quiet
    def _round(self, name, exact):
        r = exact.astype(f32)
        k = self.ulp.get(name, 0)
        if not k:
            return r
        s = self.rng.choice([-1.0, 1.0], exact.shape) if self.sign is None else self.sign
        u = ulp32(exact)
        c = (exact + s * k * u).astype(f32)
        over = np.abs(c.astype(f64) - exact) > k * u
        c = np.where(over, np.nextafter(c, r), c)
        ok = np.isfinite(exact) & np.isfinite(r) & (exact != 0) & np.isfinite(c)
        return np.where(ok, c, r).astype(f32)

    @quiet
    def exp2(self, t):
        exact = np.exp2(t.astype(f64))
        r = self._round("exp2", exact)
        return np.where(exact < FLUSH, f32(0), r).astype(f32) if HW_FLUSH["exp2_out"] else r

    @quiet
    def log2(self, x):
        x = np.where(np.abs(x) < FLUSH, np.copysign(f32(0), x), x) if HW_FLUSH["log2_in"] else x
        return self._round("log2", np.log2(x.astype(f64)))

    @quiet
    def rcp(self, x):
        x = np.where(np.abs(x) < FLUSH, np.copysign(f32(0), x), x).astype(f32) if HW_FLUSH["rcp_in"] else x
        exact = 1.0 / x.astype(f64)
        r = self._round("rcp", exact)
        return np.where(np.abs(exact) < FLUSH, np.copysign(f32(0), r), r).astype(f32) if HW_FLUSH["rcp_out"] else r


@quiet
def fma(a, b, c):
    """One rounding of a b + c (the product is exact in float64; the rare double rounding of the sum does not matter to a
    bound test, and the bit-exact checks do not go through here)."""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


# ---------------------------------------------------------------------------- float32 restatements of the helpers
@quiet
def r_exp(x, P, residual=True):
    t = x * L2E
    lo = fma(x, L2E, -t)
    e = P.exp2(t)
    return fma(e, lo * LN2F, e) if residual else e


@quiet
def r_exp_full(x, P):
    t = x * L2E
    lo = fma(x, L2E, -t)
    e = P.exp2(t)
    return fma(e, np.where(np.abs(t) < f32(128), lo * LN2F, f32(1)).astype(f32), e)


@quiet
def r_log(x, P):
    return P.log2(x) * LN2F


@quiet
def r_tanh(x, P, scale=C2):
    e = P.exp2(x * f32(scale))
    return fma(P.rcp(e + f32(1)), f32(-2), f32(1))


@quiet
def r_tanh_scaled(z, P):
    return fma(P.rcp(P.exp2(z) + f32(1)), f32(-2), f32(1))


@quiet
def r_tanh_precise(x, P, branch=PRECISE_BRANCH, lead=PRECISE_COEF[4]):
    ax = np.abs(x)
    u = x * x
    p = np.full_like(x, PRECISE_COEF[0])
    for c in PRECISE_COEF[1:4] + (f32(lead),):
        p = fma(p, u, c)
    small = fma(ax * u, p, ax)
    e = P.exp2(ax * C2)
    big = fma(P.rcp(e + f32(1)), f32(-2), f32(1))
    return np.copysign(np.where(ax < f32(branch), small, big), x).astype(f32)   # a NaN compares false: `big`, which is NaN


@quiet
def r_sigmoid(x, P):
    return fma(r_tanh(f32(0.5) * x, P), f32(0.5), f32(0.5))


@quiet
def r_sigmoid_gate(x, P, scale=-1.4426950408889634):
    return P.rcp(f32(1) + P.exp2(f32(scale) * x))


@quiet
def r_div(a, b, P, newton=True):
    r = P.rcp(b)
    q = a * r
    return fma(fma(-b, q, a), r, q) if newton else q


@quiet
def r_dpow_dp(x, p, xp, P):
    return np.where((x == 0) & (p >= 0), f32(0), xp * r_log(x, P)).astype(f32)


def r_nextafter_up(x, P=None, sign_aware=True):
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    up = (x > 0) if sign_aware else np.ones(x.shape, bool)
    return np.where(x == 0, bits(np.uint32(1)), bits(np.where(up, u + np.uint32(1), u - np.uint32(1))))


def r_nextafter_down(x, P=None):
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    return np.where(x == 0, bits(np.uint32(0x80000001)), bits(np.where(x > 0, u - np.uint32(1), u + np.uint32(1))))


# --------------------------------------------------------------------------------------------- float64 references
@quiet
def ref_sigmoid(x):
    x = np.asarray(x, f64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


@quiet
def ref_tanh_scaled(z):
    return np.tanh(np.asarray(z, f64) * (0.5 * LN2))


REF = {
    "prim_exp2": quiet(lambda x: np.exp2(x.astype(f64))), "prim_log2": quiet(lambda x: np.log2(x.astype(f64))),
    "prim_rcp": quiet(lambda x: 1.0 / x.astype(f64)), "prim_sqrt": quiet(lambda x: np.sqrt(x.astype(f64))),
    "exp": quiet(lambda x: np.exp(x.astype(f64))), "exp_full": quiet(lambda x: np.exp(x.astype(f64))), "log": quiet(lambda x: np.log(x.astype(f64))),
    "tanh": quiet(lambda x: np.tanh(x.astype(f64))), "tanh_precise": quiet(lambda x: np.tanh(x.astype(f64))),
    "sigmoid": ref_sigmoid, "sigmoid_gate": ref_sigmoid, "tanh_scaled": ref_tanh_scaled,
}
RESTATE = {"exp": r_exp, "exp_full": r_exp_full, "log": r_log, "tanh": r_tanh, "tanh_precise": r_tanh_precise, "sigmoid": r_sigmoid,
           "sigmoid_gate": r_sigmoid_gate, "tanh_scaled": r_tanh_scaled}


# ---------------------------------------------------------------------------------------------------------- bounds
# Every bound is an ABSOLUTE error bound at the point x, evaluated in float64:
#   * a primitive contributes its PRIM_ULP k as a relative error 2 U k (an ulp is at most 2 U of the value);
#   * every float32 rounding contributes U relative, the final one half an ulp of the reference;
#   * the terms go through the formula to first order; HO_* is the allowance for what first order drops: the squares and
#     cross products of the relative terms, 2 S^2 for their sum S (|(1 + a)(1 + b) - 1 - a - b| <= S^2 / 4 and the
#     remainders of 1 / (1 + S) and exp(S) are below S^2 for S < 0.5; S is below 1e-4 wherever a bound is asserted);
#   * FLUSH is added where a primitive's operand or result can be subnormal at that x (HW_FLUSH), and only there.
def _tanh_bound(x, arg_rel, arg_const):
    """1 - 2 rcp(exp2(t) + 1) with t = x * c rounded (arg_rel = U) from a constant c off by arg_const relative."""
    k = PRIM_ULP
    T = np.tanh(x)
    om, w = 1.0 - T, 0.5 * (1.0 + T)           # 2 / (E + 1) and E / (E + 1), E = exp(2 x)
    # beyond |x| = 32, E and any perturbed E are outside [2^-92, 2^92]: the result is +-1 to 2^-90 whatever the exponent error
    ee = 2 * U * k["exp2"] + 2.0 * np.minimum(np.abs(x), 32.0) * (arg_rel + arg_const)   # d ln E = 2 |x| (relative error of t)
    S = w * ee + U + 2 * U * k["rcp"]           # exp2, the rounding of e + 1, rcp
    return with_final_rounding(T, om * (S + 2 * (ee + 2 * U + 2 * U * k["rcp"]) ** 2) + 2.0 ** -90 + 2 * FLUSH)


@quiet
def bound_tanh(x):
    x = np.asarray(x, f64)
    return _tanh_bound(x, U, abs(float(C2) - 2 * LOG2E) / (2 * LOG2E))


@quiet
def bound_tanh_scaled(z):
    return _tanh_bound(np.asarray(z, f64) * (0.5 * LN2), 0.0, 0.0)


@quiet
def bound_sigmoid(x):
    x = np.asarray(x, f64)
    return with_final_rounding(ref_sigmoid(x), 0.5 * bound_tanh(0.5 * x))   # 0.5 x is exact; one fma rounding


@quiet
def bound_sigmoid_gate(x):
    x = np.asarray(x, f64)
    k = PRIM_ULP
    s = ref_sigmoid(x)
    # beyond |x| = 128 the exponential is 0 or inf whatever its error
    ee = 2 * U * k["exp2"] + np.minimum(np.abs(x), 128.0) * (U + abs(float(L2E) - LOG2E) / LOG2E)
    S = (1.0 - s) * ee + U + 2 * U * k["rcp"]
    # v_rcp flushes a subnormal result (sigma below 2^-126); a flushed exp2 moves 1 + e by at most FLUSH, sigma by s FLUSH
    return s * (S + 2 * (ee + 2 * U + 2 * U * k["rcp"]) ** 2) + np.where(s < 2 * FLUSH, FLUSH, 0.0) + s * FLUSH


@quiet
def bound_exp(x):
    x = np.asarray(x, f64)
    ref = np.exp(x)
    t = np.abs(x) * LOG2E
    const = LN2 * np.abs(x) * abs(float(L2E) - LOG2E)      # the float32 log2(e): NOT corrected by the residual, linear in |x|
    lo = LN2 * U * t                                       # |ln2 lo|, lo the exact rounding residual of t
    resid = lo * (2 * U + abs(float(LN2F) - LN2) / LN2)     # the rounding of lo * ln2 and the float32 ln2
    S = 2 * U * PRIM_ULP["exp2"] + const + resid
    ho = lo ** 2 + 2 * (S + U) ** 2                        # exp(ln2 lo) beyond its linear term; cross products
    return with_final_rounding(ref, ref * (S + ho) + np.where(ref < 2 * FLUSH, FLUSH, 0.0))   # v_exp flushes a subnormal 2^t


@quiet
def bound_log(x):
    x = np.asarray(x, f64)
    ref = np.log(x)
    S = 2 * U * PRIM_ULP["log2"] + abs(float(LN2F) - LN2) / LN2
    return with_final_rounding(ref, np.abs(ref) * (S + 2 * (S + U) ** 2))


def _precise_poly(u):
    c = [float(v) for v in PRECISE_COEF]
    ps = [np.full_like(u, c[0])]
    for v in c[1:]:
        ps.append(ps[-1] * u + v)
    return ps


@quiet
def bound_tanh_precise(x):
    ax = np.abs(np.asarray(x, f64))
    u = ax * ax
    ps = _precise_poly(u)
    p = ps[-1]
    T = np.tanh(ax)
    approx = np.abs(ax + ax * u * p - T)                   # what the polynomial itself is off by, in float64
    dp = sum(U * np.abs(ps[k]) * u ** (4 - k) for k in range(1, 5))   # the four fma roundings of the Horner chain
    du = u * 1e-6
    dp = dp + np.abs(_precise_poly(u + du)[-1] - p) / 1e-6 * U        # fl(x x): u p'(u) U
    small = with_final_rounding(T, approx + ax * u * (np.abs(p) * 2 * U + dp) + ax * u * np.abs(p) * 2 * (4 * U) ** 2)
    return np.where(ax < float(PRECISE_BRANCH), small, bound_tanh(ax))


def div_main(a, b):
    """Where div_f32's bound is asserted: a, b, 1 / b and a / b normal with the residual a - b q (about 3 U |a|) normal too."""
    with np.errstate(all="ignore"):
        a, b = np.abs(np.asarray(a, f64)), np.abs(np.asarray(b, f64))
        q = a / b
        return (a >= 2.0 ** -100) & (a < np.inf) & (b >= 2.0 ** -125) & (b <= 2.0 ** 125) & (q >= 2.0 ** -125) & (q < 2.0 ** 127)


@quiet
def bound_div(a, b):
    """q' = q (1 + s), s = rcp's error + one rounding; the Newton step returns q (1 - s (d + delta)) rounded once: the
    first-order terms cancel, which is the point of the step."""
    q = np.asarray(a, f64) / np.asarray(b, f64)
    s = 2 * U * PRIM_ULP["rcp"] + U
    return with_final_rounding(q, np.abs(q) * (s * s + 2 * s ** 3))


@quiet
def bound_dpow_dp(x, p, xp):
    ref = xp.astype(f64) * np.log(x.astype(f64))
    return with_final_rounding(ref, np.abs(xp.astype(f64)) * bound_log(x) + np.abs(ref) * 2 * U ** 2)


BOUND = {"exp": bound_exp, "exp_full": bound_exp, "log": bound_log, "tanh": bound_tanh, "tanh_precise": bound_tanh_precise,
         "sigmoid": bound_sigmoid, "sigmoid_gate": bound_sigmoid_gate, "tanh_scaled": bound_tanh_scaled}

#: where the pointwise bound of a unary helper is asserted; elsewhere EDGES and the class check apply
DOMAIN = {
    "exp": lambda x: np.isfinite(x), "exp_full": lambda x: np.isfinite(x),
    "log": lambda x: (x >= f32(FLUSH)) & np.isfinite(x),
    "tanh": lambda x: ~np.isnan(x), "tanh_precise": lambda x: ~np.isnan(x), "sigmoid": lambda x: ~np.isnan(x),
    "sigmoid_gate": lambda x: ~np.isnan(x), "tanh_scaled": lambda x: ~np.isnan(x),
}

#: sub-domains the GPU test reports maxima for
SUBDOMAINS = (("|x| < 2^-10", 0.0, 2.0 ** -10), ("2^-10 <= |x| < 1", 2.0 ** -10, 1.0), ("1 <= |x| < 8", 1.0, 8.0),
              ("8 <= |x| < 89", 8.0, 89.0), ("|x| >= 89", 89.0, np.inf))


# ----------------------------------------------------------------------------------------------------------- edges
NAN, INF = float("nan"), float("inf")
#: helper -> ((input, value it must return), ...).  A NaN stands for any NaN; zeros are compared with their sign.  Every
#: value is the mathematical one (the limit at +-inf, +-inf past the overflow threshold) to within the bound, with the
#: primitives' flush-to-zero of subnormals: tests/test_helper_cases.py holds the table to the float64 function.
EDGES = {
    # exp_f32 inside its domain, then the DOCUMENTED RESTRICTION (finite x, |x log2(e)| < 128): NaN where the limit is not
    "exp": ((0.0, 1.0), (-0.0, 1.0), (NAN, NAN), (-88.0, 0.0), (-88.7, 0.0),
            (-104.0, 0.0), (-200.0, 0.0), (-2e38, 0.0), (-FLT_MAX, NAN), (-INF, NAN), (INF, NAN), (FLT_MAX, NAN), (89.0, INF), (128.0, NAN)),
    "exp_full": ((0.0, 1.0), (-0.0, 1.0), (NAN, NAN), (-104.0, 0.0), (-200.0, 0.0), (-2e38, 0.0), (-FLT_MAX, 0.0),
                 (-INF, 0.0), (INF, INF), (FLT_MAX, INF), (2.4e38, INF), (89.0, INF), (128.0, INF)),
    "log": ((1.0, 0.0), (0.0, -INF), (-0.0, -INF), (INF, INF), (-1.0, NAN), (-INF, NAN), (NAN, NAN), (2.0 ** -149, -INF),
            (2.0 ** -127, -INF)),
    "tanh": ((0.0, 0.0), (-0.0, 0.0), (INF, 1.0), (-INF, -1.0), (NAN, NAN), (FLT_MAX, 1.0), (-FLT_MAX, -1.0), (45.0, 1.0), (-45.0, -1.0)),
    "tanh_scaled": ((0.0, 0.0), (-0.0, 0.0), (INF, 1.0), (-INF, -1.0), (NAN, NAN), (FLT_MAX, 1.0), (-FLT_MAX, -1.0), (130.0, 1.0), (-130.0, -1.0)),
    "tanh_precise": ((0.0, 0.0), (-0.0, -0.0), (INF, 1.0), (-INF, -1.0), (NAN, NAN), (FLT_MAX, 1.0), (-FLT_MAX, -1.0),
                     (2.0 ** -149, 2.0 ** -149), (-(2.0 ** -126), -(2.0 ** -126))),
    "sigmoid": ((0.0, 0.5), (-0.0, 0.5), (INF, 1.0), (-INF, 0.0), (NAN, NAN), (FLT_MAX, 1.0), (-FLT_MAX, 0.0), (-90.0, 0.0)),
    "sigmoid_gate": ((0.0, 0.5), (-0.0, 0.5), (INF, 1.0), (-INF, 0.0), (NAN, NAN), (FLT_MAX, 1.0), (-FLT_MAX, 0.0), (-90.0, 0.0), (90.0, 1.0)),
}
#: where a helper's comment restricts its domain and the call sites are shown to stay inside it (hode_common.hpp): there,
#: and only there, the class of the result is the formula's own (the restatement with perfect primitives), not the function's
RESTRICTED = {"exp": lambda x: ~np.isfinite(x) | (np.abs(x.astype(f64) * float(L2E)) >= 127.999)}
#: a subnormal operand of v_log_f32 is read as 0: the reference is taken at the flushed argument
ARG = {"log": lambda x: np.where(np.abs(x) < f32(FLUSH), np.copysign(f32(0), x), x).astype(f32)}
#: div_f32(a, b) outside div_main: ((a, b), value).  DOCUMENTED DOMAIN RESTRICTION, not the IEEE quotient: the Newton step
#: forms 0 * inf or inf - inf for a zero, infinite or subnormal divisor, an infinite dividend and an overflowing quotient, so
#: these rows pin NaN where IEEE division gives +-inf or +-0 (hode_common.hpp says why the select that would mend it was
#: not taken).  A reciprocal below 2^-126 is flushed: +-0.
DIV_EDGES = (((1.0, INF), NAN), ((1.0, -INF), NAN), ((0.0, INF), NAN), ((1.0, 0.0), NAN), ((0.0, 0.0), NAN), ((-1.0, -0.0), NAN),
             ((FLT_MAX, 0.25), NAN), ((1.0, 2.0 ** -149), NAN), ((1.0, 2.0 ** -127), NAN), ((NAN, 1.0), NAN), ((1.0, NAN), NAN),
             ((INF, 2.0), NAN), ((INF, INF), NAN), ((0.0, 3.0), 0.0), ((-0.0, 3.0), 0.0), ((6.0, 3.0), 2.0), ((1.0, 2.0 ** 127), 0.0))


def same_value(got, want):
    """Element-wise: NaN matches NaN, everything else bit for bit except the NaN payload."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return (np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))


# --------------------------------------------------------------------------------------------------- the check itself
@quiet
def check_unary(name, x, got, ref_name=None):
    """Compare `got` = helper(x) with the float64 reference of the mathematical function (at ARG's flushed argument).
    Where the function is NaN the helper must be NaN and nowhere else; where it is +-inf or rounds to +-inf by more than
    the bound the helper must be that inf; within the bound of the overflow threshold either that inf or a finite value
    within the bound is right; elsewhere the helper is finite and |got - ref| <= bound(x).
    Returns arrays over the finite points: their inputs "x", "abs", "ratio" = err / bound, "ulp", "normal"."""
    xe = ARG[name](x) if name in ARG else x
    ref = REF[ref_name or name](xe)
    b = BOUND[name](xe.astype(f64))
    g64 = got.astype(f64)
    out = RESTRICTED[name](x) if name in RESTRICTED else np.zeros(x.shape, bool)
    ideal = RESTATE[name](x[out], Prims())
    assert (np.isnan(got[out]) == np.isnan(ideal)).all() and np.array_equal(got[out][np.isinf(ideal)], ideal[np.isinf(ideal)]), name
    full, x, got, xe, ref, b, g64 = x, x[~out], got[~out], xe[~out], ref[~out], b[~out], g64[~out]
    nan_want = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan_want), "%s: NaN where none is due (or the reverse) at x = %r" % (
        name, x[np.isnan(got) != nan_want][:8])
    bb = np.where(np.isfinite(b), b, 0.0)
    must_inf = ~nan_want & (np.isinf(ref) | (np.abs(ref) - bb >= OVERFLOW))
    may_inf = ~nan_want & (np.isinf(ref) | (np.abs(ref) + bb >= OVERFLOW))
    want_inf = np.copysign(f32(np.inf), ref).astype(f32)
    assert np.array_equal(got[must_inf], want_inf[must_inf]), "%s: inf is due at x = %r" % (name, x[must_inf & (got != want_inf)][:8])
    wrong = np.isinf(got) & ~(may_inf & (got == want_inf))
    assert not wrong.any(), "%s: inf where none is due at x = %r" % (name, x[wrong][:8])
    fin = np.isfinite(got) & np.isfinite(ref) & DOMAIN[name](x)
    err = np.abs(g64[fin] - ref[fin])
    assert np.isfinite(b[fin]).all(), name
    return {"x": x[fin], "abs": err, "ratio": err / b[fin], "ulp": err / ulp32(ref[fin]), "normal": np.abs(ref[fin]) >= FLUSH}


@quiet
def check_div(a, b, got):
    """div_f32 everywhere.  Inside div_main the derived bound.  Outside, the documented classes, stated from the operands and
    the float64 quotient q = a * (1 / b) with v_rcp's flushes (a subnormal b is 0, a reciprocal below 2^-126 is 0), not from
    the formula: NaN where IEEE division is NaN and on the documented restriction (b zero, subnormal or infinite, a infinite,
    a quotient that overflows by more than 1e-6 relative); within 1e-6 of the overflow threshold NaN or a value within the
    bound; everywhere else a finite value, which is 0 where the reciprocal is flushed.  Returns (err, bound) over div_main."""
    a64 = a.astype(f64)
    bz = np.where(np.abs(b) < f32(FLUSH), np.copysign(f32(0), b), b).astype(f64)
    rr = 1.0 / bz
    rr = np.where(np.abs(rr) < FLUSH, np.copysign(0.0, rr), rr)
    qm = a64 * rr
    must_nan = np.isnan(qm) | (bz == 0) | np.isinf(bz) | np.isinf(a64) | (np.abs(qm) >= OVERFLOW * (1 + 1e-6))
    edge = ~must_nan & (np.abs(qm) > OVERFLOW * (1 - 1e-6))
    assert np.isnan(got[must_nan]).all(), "NaN is the documented result on the restriction"
    rest = ~must_nan & ~edge
    bad = rest & ~np.isfinite(got)
    assert not bad.any(), [(float(p), float(q), float(g)) for p, q, g in zip(a[bad][:8], b[bad][:8], got[bad][:8])]
    zero = rest & (rr == 0)
    assert (got[zero] == 0).all(), "a / b with a flushed reciprocal is 0"
    ok = np.isnan(got[edge]) | (np.abs(got[edge].astype(f64) - qm[edge]) <= bound_div(a[edge], b[edge]))
    assert ok.all()
    m = div_main(a, b)
    q = a64[m] / b[m].astype(f64)
    return np.abs(got[m].astype(f64) - q), bound_div(a[m], b[m])


def report(name, res):
    """One line per sub-domain: the largest err / bound, abs error and ulp error (ulp over the normal references)."""
    lines = []
    ax = np.abs(res["x"].astype(f64))
    for label, lo, hi in SUBDOMAINS + (("all", 0.0, np.inf),):
        m = (ax >= lo) & (ax < hi) if label != "all" else np.ones(ax.shape, bool)
        if m.any():
            i = np.argmax(np.where(m, res["ratio"], -1.0))
            lines.append("%-14s %-18s n = %8d  max err/bound = %.3f (x = %.9g)  max abs = %.3e  max ulp = %.2f" % (
                name, label, m.sum(), res["ratio"][i], res["x"][i], res["abs"][m].max(), np.max(res["ulp"][m & res["normal"]], initial=0.0)))
    return lines


# -------------------------------------------------------------------------------------------------------- mutants
#: name -> (helper whose bound must catch it, restatement).  Each must exceed BOUND somewhere on the input set.
MUTANTS = {
    "exp_without_residual": ("exp", lambda x, P: r_exp(x, P, residual=False)),
    "tanh_scale_5_digits": ("tanh", lambda x, P: r_tanh(x, P, scale=2.8854)),
    "sigmoid_gate_scale_5_digits": ("sigmoid_gate", lambda x, P: r_sigmoid_gate(x, P, scale=-1.4427)),
    "tanh_precise_branch_at_1": ("tanh_precise", lambda x, P: r_tanh_precise(x, P, branch=1.0)),
    "tanh_precise_lead_5_digits": ("tanh_precise", lambda x, P: r_tanh_precise(x, P, lead=-0.33333)),
}


# ------------------------------------------------------------------------------- bit-exact cross-lane restatements
def _ror(v, n):
    """DPP row_ror:n on [waves, 4 rows, 16 lanes]: lane i of a row reads lane (i - n) mod 16."""
    return np.roll(v, n, axis=-1)


def w_quad_bcast(v, src):
    q = v.reshape(-1, 4)
    return np.repeat(q[:, src], 4)


def w_quad_sum(v):
    q = v.reshape(-1, 4)
    a = q + q[:, [1, 0, 3, 2]]
    return (a + a[:, [2, 3, 0, 1]]).ravel()


def w_row_sum_stride4(v):
    r = v.reshape(-1, 16).copy()
    r = r + _ror(r, 4)
    r = r + _ror(r, 8)
    return r.ravel()


def w_row_sum(v):
    r = v.reshape(-1, 16).copy()
    for n in (1, 2, 4, 8):
        r = r + _ror(r, n)
    return r.ravel()


def w_wave_sum_stride4(v):
    w = v.reshape(-1, 64).copy()
    lane = np.arange(64)
    for m in (4, 8, 16, 32):
        w = w + w[:, lane ^ m]
    return w.ravel()


def w_wave_sum(v):
    r = w_row_sum(v).reshape(-1, 64)
    s = (r[:, 0] + r[:, 16]) + (r[:, 32] + r[:, 48])
    return np.repeat(s, 64)


#: op -> (restatement, lanes that must agree bit for bit: None, or the group size of consecutive/strided lanes)
WAVE_OPS = {
    "quad_bcast0": lambda v: w_quad_bcast(v, 0), "quad_bcast1": lambda v: w_quad_bcast(v, 1),
    "quad_bcast2": lambda v: w_quad_bcast(v, 2), "quad_bcast3": lambda v: w_quad_bcast(v, 3),
    "quad_sum": w_quad_sum, "row_sum_stride4": w_row_sum_stride4, "row_sum": w_row_sum,
    "wave_sum_stride4": w_wave_sum_stride4, "wave_sum": w_wave_sum,
    "wave_sum_patients1": w_wave_sum, "wave_sum_patients4": w_wave_sum_stride4,
}


def lanemap(lpp, B, ppw, block, n_blocks):
    """numpy restatement of LaneMap<lpp>(B, ppw) for every thread of the grid: [threads, 3] = (p, q, live)."""
    tid = np.arange(n_blocks * block)
    lane, wave = (tid % block) & 63, tid >> 6
    slot, q = lane // lpp, lane % lpp
    pp = wave * ppw + slot
    live = (slot < ppw) & (pp < B)
    p = np.where(live, pp, np.minimum(pp, B - 1))
    p = np.where(slot >= ppw, np.minimum(wave * ppw, B - 1), p)
    return np.stack([p, q, live.astype(np.int64)], axis=1)


LANEMAP_B = (1, 5, 63, 64, 65, 161)
LANEMAP_PPW = {4: (1, 3, 10, 16), 1: (1, 10, 37, 64)}
BLOCKS = (64, 256)
ROUNDTRIP_D = (4, 6, 8, 12, 20)


def grid_blocks(B, ppw, block):
    waves = -(-B // ppw)
    return -(-waves // (block // 64))


# ------------------------------------------------------------------------------------------------- coverage table
#: HODE_DEV function of hode_common.hpp / hode_lanes.hpp -> the probe ops (include/hode_probe.h) that run it
PROBED = {
    "exp_f32": ("exp",), "exp_full_f32": ("exp_full",), "log_f32": ("log", "dpow_dp"), "tanh_f32": ("tanh", "tanh_pk0", "tanh_pk1"),
    "tanh_precise_f32": ("tanh_precise",), "sigmoid_f32": ("sigmoid",), "div_f32": ("div",),
    "quad_bcast": ("quad_bcast0", "quad_bcast1", "quad_bcast2", "quad_bcast3"), "quad_sum": ("quad_sum",),
    "row_sum_stride4": ("row_sum_stride4",), "row_sum": ("row_sum",), "wave_sum_stride4": ("wave_sum_stride4",),
    "wave_sum": ("wave_sum",), "nextafter_up": ("nextafter_up",), "nextafter_down": ("nextafter_down",),
    "mul_rn": ("mul_add_rn",), "add_rn": ("mul_add_rn",),
    "wave_sum_patients": ("wave_sum_patients1", "wave_sum_patients4"),
    "tanh_scaled": ("tanh_scaled_f", "tanh_scaled_pk0", "tanh_scaled_pk1"),
    "tanh_scaled4": ("tanh_scaled4_0", "tanh_scaled4_1", "tanh_scaled4_2", "tanh_scaled4_3"),
    "sigmoid2": ("sigmoid2_0", "sigmoid2_1", "sigmoid4_0", "sigmoid4_3"), "sigmoid4": ("sigmoid4_0", "sigmoid4_3"),
    "tanh4": ("tanh4_1", "tanh4_2"),
    "load_vec": ("roundtrip",), "store_vec": ("roundtrip",), "LaneMap": ("lanemap", "roundtrip"),
}
#: not probed on their own, with the reason
EXEMPT = {
    "splat2": "pure spelling of one instruction (a register pair)",
    "pair2": "pure spelling of one instruction (a register pair)",
    "vfma": "pure spelling of one instruction (v_fma_f32 / v_pk_fma_f32)",
    "vsplat": "pure spelling of one instruction (identity / splat2)",
    "hsum": "pure spelling of one instruction (v_add_f32 of the two halves)",
    "lo2": "pure spelling of one instruction (a register pair); runs inside sigmoid4 and tanh4, which are probed",
    "hi2": "pure spelling of one instruction (a register pair); runs inside sigmoid4 and tanh4, which are probed",
    "cat4": "pure spelling of one instruction (two register pairs); runs inside sigmoid4 and tanh4, which are probed",
    "vfinite": "pure spelling of one instruction (v_cmp_class); a wrong answer would show as a wrong status in the solver tests",
    "dpp_f32": "pure spelling of one instruction (v_mov_dpp); runs inside row_sum and row_sum_stride4, which are probed",
}
#: op -> the op it must equal bit for bit on the whole unary input set (the copies of one formula)
SAME_BITS = {
    "tanh_pk0": "tanh", "tanh_pk1": "tanh", "tanh4_1": "tanh", "tanh4_2": "tanh",
    "tanh_scaled1": "tanh_scaled0", "tanh_scaled2": "tanh_scaled0", "tanh_scaled3": "tanh_scaled0",
    "tanh_scaled_f": "tanh_scaled0", "tanh_scaled_pk0": "tanh_scaled0", "tanh_scaled_pk1": "tanh_scaled0",
    "tanh_scaled4_0": "tanh_scaled0", "tanh_scaled4_1": "tanh_scaled0", "tanh_scaled4_2": "tanh_scaled0", "tanh_scaled4_3": "tanh_scaled0",
    "sigmoid2_0": "sigmoid", "sigmoid2_1": "sigmoid", "sigmoid4_0": "sigmoid", "sigmoid4_3": "sigmoid",
}
#: probe entry points that are not ops of hode_probe_map / hode_probe_wave
ENTRY_POINTS = ("lanemap", "roundtrip")
