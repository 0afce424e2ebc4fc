"""The GPU case table of libhode_roche_dims.so (tests/test_hip_roche_dims.py) and the kernels each case launches: the
hybrid Roche rhs at the latent sizes libhode.so does not hold.  Restates, independently of the library, which kernel
csrc/roche_dims/ launches for a call: fixed grid -- dispatch_lpp_ragged (csrc/hode_rk_kernels.hpp): LPP 4 (a patient per
quad, ragged where (D - 4) % 4 != 0) or 1 at every size; dopri5 -- dp_dispatch as it is: LPP 4 at 16 only.  The rhs
bodies, theta vectors and dose counts are tests/kernel_variants.py's."""
import kernel_variants as kv

DIMS = (5, 7, 9, 10, 11, 13, 14, 15, 16)
LANES = (1, 4)            # lanes_per_patient of the fixed-grid cases: both layouts at every size
METHODS = ("euler", "midpoint", "rk4")
N, T = kv.ROCHE_N, kv.ROCHE_T     # 77 patients: the host gives a batch this small one patient per wave; 8 grid points
MANY_N = 2 * 1024 + N         # 2125 patients: three per wave, one on the last wave


def patients_per_wave(B, lpp):
    """csrc/hode_rk_host.hpp patients_per_wave for B < 1024 * 64 / lpp: about one wave per SIMD."""
    assert B < 1024 * (64 // lpp)
    return max(1, min(64 // lpp, -(-B // 1024)))


def n_waves(B, lpp):
    return -(-B // patients_per_wave(B, lpp))


def ragged(D):
    return (D - 4) % 4 != 0


def rk_lpp(D, lanes, B=N):
    """csrc/roche_dims/hode_roche_dims.hip rk_lpp: by default the quad layout below 131 072 patients, at every size but 5
    (the layout measured faster at 10 000 patients, profiles/roche_dims_probe.txt)."""
    if lanes in (1, 4):
        return lanes
    return 1 if (D == 5 or B >= 131072) else 4


def dp_lpp(D, lanes, B=kv.DOPRI5_N):
    return kv.choose_lpp(D, lanes, B)


def fixed_kernels(D, lanes, method, ablate, need_theta):
    lpp, a = rk_lpp(D, lanes), kv._b(ablate)
    m = kv.METHODS[method]
    return ["hode::rk_fwd_kernel<%d, %d, %d, %s>" % (D, lpp, m, a),
            "hode::rk_bwd_kernel<%d, %d, %d, %s, %s>" % (D, lpp, m, a, kv._b(need_theta)), "hode::fold_partials_kernel"]


def dopri5_kernels(D, lanes, ablate, need_theta, detach):
    return kv.dopri5_kernels(D, lanes, ablate, need_theta, detach) + ["hode::fold_partials_kernel"]


def _fixed_cases():
    base = [dict(family="roche", D=D, lanes=lanes, method=method, ablate=ablate, need_theta=nt)
            for D in DIMS for lanes in LANES for method in METHODS for ablate in (False, True) for nt in (False, True)]
    return kv._with_bodies(base)


def _dopri5_cases():
    """Every instantiation with every body it holds (first step attached: dp_initbwd runs too), and one call per
    (size, layout, rhs) with the first step detached.

    The detached calls run WITHOUT doses, as kernel_variants' hill_ulp dopri5 cases do: their bound (rel-L2 1e-4) has no
    term for what float32 itself loses, so the problem must not have the one float32 event that is not rounding -- a stage
    time within an fp32 ulp of a dose time, which the fp32 stage time puts on the other side of the jump.  With one dose
    per patient that happens on the D = 10 problem: the oracle's own fp32 replay of the kernel's tape is 1.68e-4 from fp64
    in grad_theta (d / d kel 2.4e-4; the kernel 1.64e-4 / 2.4e-4, every other gradient 1e-6 .. 8e-6), and 6e-9 .. 7e-6 at
    the other sizes.  The jump is covered by the attached cases, whose bound carries twice the fp32 replay's own distance;
    the sweep kernel is the same in both, detaching only skips the two passes of the first step's backward."""
    out, i = [], 0
    for D in DIMS:
        for lanes in ((1, 4) if not ragged(D) else (1,)):
            for ablate in (False, True):
                for nt in (False, True):
                    c = dict(family="dopri5", D=D, lanes=lanes, ablate=ablate, need_theta=nt)
                    out.append(dict(c, detach=False, theta="default", n_dose=1))
                    out.append(dict(c, detach=False, theta="default", n_dose=(0, 2, 3)[i % 3]))
                    if not ablate:
                        out.append(dict(c, detach=False, theta="general", hill=kv.GENERAL_HILL[i % 3], n_dose=(2, 3, 0)[(i // 3) % 3]))
                    i += 1
                out.append(dict(family="dopri5", D=D, lanes=lanes, ablate=ablate, need_theta=bool(i % 2), detach=True,
                                theta="default", n_dose=0))
    return out


FIXED_CASES = _fixed_cases()
DOPRI5_CASES = _dopri5_cases()
CASES = FIXED_CASES + DOPRI5_CASES

#: the fixed-grid cases that aim at one property each (tests/test_hip_roche_dims.py): at the two sizes with the most padding
#: (5: three of four lanes own only padding; 15: the last lane owns two rows and one padding slot) and the regular 16
TARGETED_DIMS = (5, 10, 15, 16)
#: (B, T) beside (N, T): one patient, T = 1 (the backward returns grad_h[0]) and T = 2 (one step)
EDGE_SHAPES = ((1, T), (N, 1), (N, 2), (1, 1))


def kernels(case):
    if case["family"] == "roche":
        return fixed_kernels(case["D"], case["lanes"], case["method"], case["ablate"], case["need_theta"])
    return dopri5_kernels(case["D"], case["lanes"], case["ablate"], case["need_theta"], case["detach"])


def case_id(case):
    return kv.case_id(case)


def expected_kernels():
    """What the objects of csrc/roche_dims/build hold."""
    out = {"hode::fold_partials_kernel"}
    for D in DIMS:
        for a in ("false", "true"):
            for lpp in (1, 4):
                for m in (0, 1, 2):
                    out.add("hode::rk_fwd_kernel<%d, %d, %d, %s>" % (D, lpp, m, a))
                    out.update("hode::rk_bwd_kernel<%d, %d, %d, %s, %s>" % (D, lpp, m, a, nt) for nt in ("false", "true"))
            for lpp in ((1,) if ragged(D) else (1, 4)):
                out.update("hode::dp_fwd_kernel<%d, %d, %s, %d>" % (D, lpp, a, ph) for ph in (0, 1, 2))
                out.update("hode::dp_bwd_kernel<%d, %d, %s, %s>" % (D, lpp, a, nt) for nt in ("false", "true"))
                out.add("hode::dp_initbwd_kernel<%d, %d, %s, false, 1>" % (D, lpp, a))
                out.update("hode::dp_initbwd_kernel<%d, %d, %s, %s, 2>" % (D, lpp, a, nt) for nt in ("false", "true"))
            if not ragged(D):
                out.add("hode::dp_persist_kernel<%d, %s>" % (D, a))
    return out


#: compiled, never launched by the product build (tests/kernel_variants.py _NO_PERSIST says why)
UNREACHABLE = {"hode::dp_persist_kernel<16, %s>" % a for a in ("false", "true")}


def kernels_reached():
    return {k for c in CASES for k in kernels(c)}


def bodies_reached():
    """{(kernel, body)} over the table."""
    return {(k, kv.body(c)) for c in CASES for k in kernels(c) if kv.family(k) in kv.ROCHE_FAMILIES}
