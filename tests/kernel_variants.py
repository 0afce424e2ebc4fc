"""Which compiled kernel instantiation a call launches: the host dispatch rules of the solver and decoder families restated
in Python, and the table of calls (CASES) that reaches every instantiation.  A plain helper module, not a conftest.

* tests/test_kernel_variant_coverage.py (CPU) checks the table against the `.kd` symbols of the built code objects (every
  instantiation of a covered family is produced by a CASES entry or listed in UNREACHABLE) and the restated tile rules
  against the workspace sizes libhode reports.
* tests/test_hip_kernel_variants.py (GPU) runs every CASES entry against a float64 reference.

Kernel names are the demangled symbols with `(anonymous namespace)::`, the return type and the argument list dropped:
`hode::split_bwd_kernel<12, 2, false, false, true>`; enums appear as integers (HODE_METHOD_EULER / MIDPOINT / RK4_38 =
0 / 1 / 2, HODE_SEQDEC_TLSTM / GRUODE = 0 / 1, HODE_RHS_NEURAL_REAL / _2ND = 4 / 5).  rocprofv3 prints the same names
with those decorations; `kernel_name()` strips them.
"""
import re

EULER, MIDPOINT, RK4 = 0, 1, 2
METHODS = {"euler": EULER, "midpoint": MIDPOINT, "rk4": RK4}
METHOD_NAMES = {v: k for k, v in METHODS.items()}
SEQDEC_KIND = {"tlstm": 0, "gruode": 1}
NR_KIND = {"neural": 4, "2nd": 5}
SPLIT_MAX_T = 8192  # kSplitMaxT, csrc/hode_rk_split.hip:105

# kernel-name prefixes of the covered families (the guard reads every symbol that starts with one of them)
FAMILIES = ("tlstm_fwd_kernel", "tlstm_bwd_kernel", "gruode_fwd_kernel", "gruode_bwd_kernel", "seqdec_fold_kernel",
            "neural_real_fwd_kernel", "neural_real_bwd_kernel", "neural_real_fold_kernel",
            "real_mf_kernel", "real_grad_fold_kernel", "real_kernel",
            "rk_fwd_kernel", "rk_bwd_kernel", "split_fwd_kernel", "split_bwd_kernel", "split_fold_kernel",
            "mf_fwd_kernel", "mf_bwd_kernel", "mf_fold_kernel", "dp_bwd_kernel")


def kernel_name(demangled):
    """`void hode::(anonymous namespace)::f<1, 2>(hode::Args)` -> `hode::f<1, 2>`."""
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"^void ", "", s.strip())
    depth = 0
    for i, c in enumerate(s):  # cut at the argument list (the first '(' outside the template brackets)
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return s[:i]
    return s


def family(name):
    base = name.split("<")[0]
    base = base[len("hode::"):] if base.startswith("hode::") else base
    return base if base in FAMILIES else None


def _b(x):
    return "true" if x else "false"


# ------------------------------------------------------------------------------------------------------ dispatch rules
def seqdec_tiles(D):
    """csrc/hode_seqdec.hip:564 tile_config: D <= 13 -> <1,1>, 14..16 -> <1,2>, 17..29 -> <2,2> (HT = ceil(D/16),
    KT = ceil((D+3)/16))."""
    return (1, 1) if D <= 13 else ((1, 2) if D <= 16 else (2, 2))


def seqdec_kernels(kind, D):
    """csrc/hode_seqdec.hip:575-594 launch<HT, KT>: the kind's forward, backward and the fold of its partials."""
    ht, kt = seqdec_tiles(D)
    return ["hode::%s_fwd_kernel<%d, %d>" % (kind, ht, kt), "hode::%s_bwd_kernel<%d, %d>" % (kind, ht, kt),
            "hode::seqdec_fold_kernel<%d, %d, %d>" % (SEQDEC_KIND[kind], ht, kt)]


def neural_real_shape(kind, D, H):
    """csrc/hode_neural_real_mf.hip:50-62 NrLayout + :572-580 nr_shape -> (ST, IT, HT).  neural: ST = ceil(D/16),
    IT = ceil((D+2)/16); 2nd: the state is two halves of D/2, each padded to whole tiles (off2 = 16 ceil(D/32)),
    ST = 2 off2/16, IT = ceil((off2 + D/2 + 2)/16); HT = ceil(H/16)."""
    if kind == "2nd":
        n1 = D // 2
        off2 = 16 * ((n1 + 15) // 16)
        st, pdose = 2 * (off2 // 16), off2 + n1
    else:
        st, pdose = (D + 15) // 16, D
    return st, (pdose + 2 + 15) // 16, (H + 15) // 16


def neural_real_kernels(kind, D, H, method):
    """csrc/hode_neural_real_mf.hip:584-605 nr_launch / nr_launch_ht, :646-656 the (ST, IT) switch, :659 the fold."""
    st, it, ht = neural_real_shape(kind, D, H)
    args = "%d, %d, %d, %d, %d" % (NR_KIND[kind], st, it, ht, method)
    return ["hode::neural_real_fwd_kernel<%s>" % args, "hode::neural_real_bwd_kernel<%s>" % args,
            "hode::neural_real_fold_kernel"]


def real_mf_ht(H):
    """csrc/hode_real_mf.hip:551-553 launch_real_mf: HT = ceil(H/16)."""
    return (H + 15) // 16


def real_kernels(D, H, method, onchip=True):
    """HODE_RHS_ROCHE_REAL.  csrc/hode_real_mf.hip:518 real_mf_supported (D == 20, H <= 64) selects the matrix-core
    kernels (csrc/hode_real.hip:405); their backward folds the weight gradients on chip when the caller hands grad_w1
    (csrc/hode_real_mf.hip:525 `onchip`, :534 real_grad_fold_kernel), else it writes the operand tape.  Everything else
    (D = 4, D = 20 with H > 64) runs csrc/hode_real.hip:374-382 real_kernel<D, METHOD, BWD>."""
    if D == 20 and 1 <= H <= 64:
        ht = real_mf_ht(H)
        out = ["hode::real_mf_kernel<%d, %d, false, false>" % (ht, method),
               "hode::real_mf_kernel<%d, %d, true, %s>" % (ht, method, _b(onchip))]
        return out + (["hode::real_grad_fold_kernel<%d>" % ht] if onchip else [])
    return ["hode::real_kernel<%d, %d, false>" % (D, method), "hode::real_kernel<%d, %d, true>" % (D, method)]


def choose_lpp(D, lanes, B):
    """csrc/hode_api.hip:70 choose_lpp."""
    can4 = D > 4 and (D - 4) % 4 == 0
    if lanes == 1:
        return 1
    if lanes == 4:
        return 4 if can4 else 1
    if not can4:
        return 1
    return 1 if B >= 131072 else 4


def roche_layout(D, lanes, T):
    """csrc/hode_api.hip:126 use_split (D 8 / 12, T <= kSplitMaxT, lanes 48 or 0; the backward needs T >= 2), :113 use_mf
    (D 8 / 12 / 16 and lanes 16), else the per-dimension lane kernels (:138 dispatch_dim)."""
    if D in (8, 12) and T <= SPLIT_MAX_T and T >= 2 and lanes in (0, 48):
        return "split"
    if D in (8, 12, 16) and lanes == 16:
        return "mf"
    return "lane"


def roche_fixed(D, lanes, method, ablate, need_theta, tape=True, T=8, B=77):
    """Fixed-grid Roche forward + backward as hode.plan.RocheRKPlan launches them (tape = HODE_FLAG_TAPE).
    split: csrc/hode_rk_split.hip:1133-1168 split_method / split_bwd_method (the tape pointer selects TAPE, need_theta_grad
    NEED_TH) and the fold :1228.  mf: csrc/hode_rk_mf.hip:554-575 mf_launch / mf_dim and the fold :597.  lane kernels:
    csrc/hode_rk_kernels.hpp:344 dispatch_lpp (LPP 4 only where (D-4) % 4 == 0), :327 dispatch_method, :320 launch_bwd."""
    lay = roche_layout(D, lanes, T)
    a, nt = _b(ablate), _b(need_theta)
    if lay == "split":
        # csrc/hode_rk_split.hip:1189-1201 split_etape_bytes / split_ltape_bytes: euler has no intermediate stage to tape,
        # so split_tape() is NULL and the TAPE=false kernels run whatever the flag says
        tp = _b(tape and method != EULER)
        return ["hode::split_fwd_kernel<%d, %d, %s, %s>" % (D, method, a, tp),
                "hode::split_bwd_kernel<%d, %d, %s, %s, %s>" % (D, method, a, nt, tp), "hode::split_fold_kernel"]
    if lay == "mf":
        return ["hode::mf_fwd_kernel<%d, %d, %s>" % (D, method, a), "hode::mf_bwd_kernel<%d, %d, %s, %s>" % (D, method, a, nt),
                "hode::mf_fold_kernel"]
    lpp = choose_lpp(D, lanes, B)
    return ["hode::rk_fwd_kernel<%d, %d, %d, %s>" % (D, lpp, method, a),
            "hode::rk_bwd_kernel<%d, %d, %d, %s, %s>" % (D, lpp, method, a, nt)]


def dopri5_bwd(D, lanes, ablate, need_theta, B=21):
    """csrc/hode_dopri5.hip:258-262 (LPP = choose_lpp) -> csrc/hode_dopri5_kernels.hpp:1581 dp_dispatch (LPP 4 only where
    (D-4) % 4 == 0) -> :1561 phase 3, dp_bwd_kernel<D, LPP, ABLATE, NEED_TH>."""
    return ["hode::dp_bwd_kernel<%d, %d, %s, %s>" % (D, choose_lpp(D, lanes, B), _b(ablate), _b(need_theta))]


# ---------------------------------------------------------------------------------------------------------- the table
def _seqdec_cases():
    out = []
    for kind in ("tlstm", "gruode"):
        for D in (1, 13, 14, 16, 17, 29):
            for B in (1, 37, 100):
                out.append(dict(family="seqdec", kind=kind, D=D, B=B, t0=8))
        out.append(dict(family="seqdec", kind=kind, D=15, B=19, t0=29))  # T' = 1 in the <1,2> class
    return out


def _neural_real_cases():
    """Every (ST, IT) tile class of both kinds x every HT x every method; D alternates between the two edges of its class,
    H between the two edges of its hidden-tile class; B, perturb and ode_step_div cycle."""
    classes = (("neural", (1, 14)), ("neural", (15, 16)), ("neural", (17, 30)),
               ("2nd", (2, 28)), ("2nd", (30, 32)), ("2nd", (34, 60)))
    hs = ((1, 16), (17, 32), (33, 48), (49, 64))
    out, i = [], 0
    for kind, ds in classes:
        for hi, hpair in enumerate(hs):
            for method in ("euler", "midpoint", "rk4"):
                out.append(dict(family="neural_real", kind=kind, D=ds[i % 2], H=hpair[(i // 2) % 2], method=method,
                                B=(1, 37, 100)[i % 3], perturb=bool((i // 3) % 2), div=1 + (i // 5) % 2))
                i += 1
    return out


def _real_cases():
    out = []
    for method in ("euler", "midpoint", "rk4"):
        for H in (1, 16, 17, 32, 48, 64):
            out.append(dict(family="real", D=20, H=H, method=method, onchip=True))
        for H in (16, 17, 33, 49):  # the tape-writing matrix-core backward (C ABI with grad_w1 = NULL)
            out.append(dict(family="real", D=20, H=H, method=method, onchip=False))
        out.append(dict(family="real", D=20, H=65, method=method, onchip=True))  # past the matrix-core range: hode_real.hip
        out.append(dict(family="real", D=4, H=9, method=method, onchip=True))
    return out


def _roche_cases():
    out = []
    # lane kernels: every dimension x LPP x method x rhs x need_theta
    for D in (4, 6, 8, 12, 20):
        for lanes in ((1, 4) if (D - 4) % 4 == 0 and D > 4 else (1,)):
            for method in ("euler", "midpoint", "rk4"):
                for ablate in (False, True):
                    for nt in (False, True):
                        out.append(dict(family="roche", D=D, lanes=lanes, method=method, ablate=ablate, need_theta=nt,
                                        tape=True))
    # the library's choice (lanes 0) where it is a lane kernel: D 4 (LPP 1) and 20 (LPP 4)
    for D in (4, 20):
        out.append(dict(family="roche", D=D, lanes=0, method="rk4", ablate=False, need_theta=False, tape=True))
    # split layout: lanes 48 and the default (0) alternate; tape on and off
    i = 0
    for D in (8, 12):
        for method in ("euler", "midpoint", "rk4"):
            for ablate in (False, True):
                for nt in (False, True):
                    for tape in (False, True):
                        out.append(dict(family="roche", D=D, lanes=(48, 0)[i % 2], method=method, ablate=ablate,
                                        need_theta=nt, tape=tape))
                        i += 1
    # MFMA opt-in
    for D in (8, 12, 16):
        for method in ("euler", "midpoint", "rk4"):
            for ablate in (False, True):
                for nt in (False, True):
                    out.append(dict(family="roche", D=D, lanes=16, method=method, ablate=ablate, need_theta=nt, tape=True))
    return out


def _dopri5_cases():
    out = []
    for D in (4, 6, 8, 12):
        for lanes in ((1, 4) if D in (8, 12) else (1,)):
            for ablate in (False, True):
                for nt in (False, True):
                    out.append(dict(family="dopri5", D=D, lanes=lanes, ablate=ablate, need_theta=nt))
    return out


ROCHE_N, ROCHE_T = 77, 8   # ragged batch (not a multiple of 16, 48 or 64), short grid
DOPRI5_N, DOPRI5_T = 21, 10

CASES = _seqdec_cases() + _neural_real_cases() + _real_cases() + _roche_cases() + _dopri5_cases()


def kernels(case):
    """Kernel names the CASES entry launches."""
    f = case["family"]
    if f == "seqdec":
        return seqdec_kernels(case["kind"], case["D"])
    if f == "neural_real":
        return neural_real_kernels(case["kind"], case["D"], case["H"], METHODS[case["method"]])
    if f == "real":
        return real_kernels(case["D"], case["H"], METHODS[case["method"]], case["onchip"])
    if f == "roche":
        return roche_fixed(case["D"], case["lanes"], METHODS[case["method"]], case["ablate"], case["need_theta"],
                           case["tape"], ROCHE_T, ROCHE_N)
    if f == "dopri5":
        return dopri5_bwd(case["D"], case["lanes"], case["ablate"], case["need_theta"], DOPRI5_N)
    raise ValueError(f)


def case_id(case):
    return "-".join("%s=%s" % (k, v) for k, v in case.items())


# compiled instantiations no dispatch of the library reaches (name -> reason)
_NO_EULER_TAPE = ("euler has no intermediate stage to tape: the tape pointer is NULL (csrc/hode_rk_split.hip:1189-1201), "
                  "so HODE_FLAG_TAPE launches the TAPE=false kernel")
UNREACHABLE = {}
for _D in (8, 12):
    for _a in ("false", "true"):
        UNREACHABLE["hode::split_fwd_kernel<%d, 0, %s, true>" % (_D, _a)] = _NO_EULER_TAPE
        for _nt in ("false", "true"):
            UNREACHABLE["hode::split_bwd_kernel<%d, 0, %s, %s, true>" % (_D, _a, _nt)] = _NO_EULER_TAPE
