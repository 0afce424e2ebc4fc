"""Which compiled kernel instantiation a call launches: the host dispatch rules of the solver and decoder families restated
in Python, and the table of calls (CASES) that reaches every instantiation.  A plain helper module, not a conftest.

* tests/test_kernel_variant_coverage.py (CPU) checks the table against the `.kd` symbols of the built code objects (every
  instantiation of a covered family is produced by a CASES entry or listed in UNREACHABLE) and the restated tile rules
  against the workspace sizes libhode reports.
* tests/test_hip_kernel_variants.py (GPU) runs every CASES entry against a float64 reference.

Every Roche kernel also picks one of up to three inlined rhs bodies per launch, at run time (roche_body): a `.kd` symbol
holds all of them, so the guard checks (instantiation, body) pairs (bodies(), body(case)) and reads the branch itself out
of the kernel source.

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
            "mf_fwd_kernel", "mf_bwd_kernel", "mf_fold_kernel", "dp_fwd_kernel", "dp_bwd_kernel", "dp_initbwd_kernel",
            "dp_persist_kernel")
# the families whose kernels branch between the Roche rhs bodies (roche_body)
ROCHE_FAMILIES = ("rk_fwd_kernel", "rk_bwd_kernel", "split_fwd_kernel", "split_bwd_kernel", "mf_fwd_kernel", "mf_bwd_kernel",
                  "dp_fwd_kernel", "dp_bwd_kernel", "dp_initbwd_kernel", "dp_persist_kernel")


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


def dopri5_kernels(D, lanes, ablate, need_theta, detach_first_step=True, B=21):
    """One adaptive solve + its backward.  LPP = choose_lpp (csrc/hode_dopri5.hip:162, :258) -> csrc/hode_dopri5_kernels.hpp
    dp_dispatch (LPP 4 only where (D-4) % 4 == 0) -> dp_launch: the forward's phases 0 / 1 (initial step) and 2 (attempts),
    dp_fwd_kernel<D, LPP, ABLATE, PHASE>; the backward sweep, dp_bwd_kernel<D, LPP, ABLATE, NEED_TH>; and unless the first
    step size is detached (csrc/hode_dopri5.hip:267) the two passes of its backward, dp_initbwd_kernel<D, LPP, ABLATE,
    false, 1> (pass 1 forms a scalar: always NEED_TH = false) and dp_initbwd_kernel<D, LPP, ABLATE, NEED_TH, 2>."""
    lpp, a = choose_lpp(D, lanes, B), _b(ablate)
    out = ["hode::dp_fwd_kernel<%d, %d, %s, %d>" % (D, lpp, a, ph) for ph in (0, 1, 2)]
    out.append("hode::dp_bwd_kernel<%d, %d, %s, %s>" % (D, lpp, a, _b(need_theta)))
    if not detach_first_step:
        out += ["hode::dp_initbwd_kernel<%d, %d, %s, false, 1>" % (D, lpp, a),
                "hode::dp_initbwd_kernel<%d, %d, %s, %s, 2>" % (D, lpp, a, _b(need_theta))]
    return out


# ---------------------------------------------------------------------------------------------- Roche rhs bodies
# body -> (HILL2, K1) template arguments of the *_body / *_body_own call that runs it
BODY_ARGS = {"hill2_k1": (True, True), "hill2_kn": (True, False), "general": (False, False)}


def roche_body(ablate, theta0, theta1, K):
    """The runtime branch of every Roche kernel (K = dose times per patient, theta0 / theta1 = HillCure / HillPatho as the
    fp32 values the kernel reads):
        const bool hill2 = ABLATE || (a.theta[0] == 2.0f && a.theta[1] == 2.0f);
        if (hill2 && a.K == 1) body<..., HILL2 = true, K1 = true>     "hill2_k1"  x * x, one dose time in a register
        else if (hill2)        body<..., HILL2 = true, K1 = false>    "hill2_kn"  x * x, loop over K dose times
        else                   body<..., HILL2 = false, K1 = false>   "general"   powf / log_f32, loop over K dose times
    csrc/hode_rk_kernels.hpp:122-126 (rk_fwd_kernel), :299-302 (rk_bwd_kernel); csrc/hode_rk_split.hip:1115-1118
    (split_bwd_kernel), :1123-1126 (split_fwd_kernel); csrc/hode_rk_mf.hip:245-248 (mf_fwd_kernel), :498-501
    (mf_bwd_kernel); csrc/hode_dopri5_kernels.hpp:886-889 (dp_persist_kernel), :896-906 (dp_fwd_kernel; its attempt
    launches take hill2 from the host's read-back of the same comparison, csrc/hode_dopri5.hip:178-184), :1395-1403
    (dp_bwd_kernel), :1536-1539 (dp_initbwd_kernel).  ABLATE forces hill2: the ablate rhs has no Hill terms."""
    hill2 = bool(ablate) or (theta0 == 2.0 and theta1 == 2.0)
    if hill2:
        return "hill2_k1" if K == 1 else "hill2_kn"
    return "general"


def _ablate_arg(name):
    """ABLATE template argument of a Roche kernel name (rk_*: 4th, split_* / mf_*: 3rd, dp_*: 3rd, dp_persist: 2nd)."""
    fam = family(name)
    args = [x.strip() for x in name[name.index("<") + 1:name.rindex(">")].split(",")]
    pos = {"rk_fwd_kernel": 3, "rk_bwd_kernel": 3, "dp_persist_kernel": 1}.get(fam, 2)
    assert args[pos] in ("true", "false"), name
    return args[pos] == "true"


def bodies(name):
    """The rhs bodies a compiled Roche instantiation holds: all three, or hill2_k1 / hill2_kn for ABLATE = true."""
    if family(name) not in ROCHE_FAMILIES:
        return ()
    return ("hill2_k1", "hill2_kn") if _ablate_arg(name) else ("hill2_k1", "hill2_kn", "general")


# ------------------------------------------------------------------------------------------------------- theta vectors
THETA_DEFAULT = (2.0, 2.0) + (1.0,) * 11  # oracle.rhs.THETA_DEFAULT: the reference's configuration
# the 11 rate constants of the general cases (tests/test_hip_rk.py's random theta; ec50 != 1, so ln(ec50) != 0)
THETA_RATES = (0.8, 1.3, 0.7, 0.9, 1.1, 0.6, 1.2, 0.5, 1.4, 0.75, 0.65)
# Hill exponent pairs of theta = "general": both non-integer, or exactly one equal to 2.0 (still the general body)
GENERAL_HILL = ("2.5,1.5", "2.0,1.5", "1.5,2.0")
NEG_BASE_HILL = "3.0,1.0"  # integer exponents: with a negative Immunity, torch.pow is finite and its log is NaN
HILL_ULP = 2.0000002384185791  # nextafter(2.0f, 3.0f) = 2 + 2^-22


def theta_of(case):
    """The 13 expert parameters of a Roche / dopri5 case (theta key "default" / "general" / "hill_ulp")."""
    th = case.get("theta", "default")
    if th == "default":
        return THETA_DEFAULT
    if th == "hill_ulp":
        return (HILL_ULP, 2.0) + THETA_RATES
    assert th == "general", th
    return tuple(float(x) for x in case["hill"].split(",")) + THETA_RATES


def body(case):
    """The rhs body the Roche / dopri5 CASES entry runs (roche_body), None for the other families."""
    if case["family"] not in ("roche", "dopri5"):
        return None
    th = theta_of(case)
    return roche_body(case["ablate"], th[0], th[1], case["n_dose"])


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
    return _with_bodies(out) + _roche_extra_cases()


def _with_bodies(base):
    """Each call above runs the hill2_k1 body (default theta, one dose); every one is repeated with the dose-list body and,
    for the full rhs, with the general body, so that every (instantiation, body) pair is reached.  K = n_dose cycles
    through 0, 2, 3 and the general Hill pair through GENERAL_HILL."""
    out, i = [], 0
    for c in base:
        out.append(dict(c, theta="default", n_dose=1))
        out.append(dict(c, theta="default", n_dose=(0, 2, 3)[i % 3]))
        if not c["ablate"]:
            out.append(dict(c, theta="general", hill=GENERAL_HILL[i % 3], n_dose=(2, 3, 0)[(i // 3) % 3]))
        i += 1
    return out


def _roche_extra_cases():
    """hill_ulp: HillCure one ulp above 2 takes the general body; the GPU test compares it with fp64 and with the same call
    at exactly 2 (the x * x body).  neg_imm: Hill 3 and 1 with a negative Immunity in y0 (torch.pow's negative-base rule).
    One of each per layout and dimension class."""
    out = []
    for D, lanes, method in ((4, 1, "rk4"), (12, 4, "midpoint"), (20, 0, "euler"), (8, 48, "rk4"), (12, 0, "euler"),
                             (8, 16, "rk4"), (16, 16, "midpoint")):
        out.append(dict(family="roche", D=D, lanes=lanes, method=method, ablate=False, need_theta=True, tape=True,
                        theta="hill_ulp", n_dose=1))
        out.append(dict(family="roche", D=D, lanes=lanes, method=method, ablate=False, need_theta=True, tape=True,
                        theta="general", hill=NEG_BASE_HILL, n_dose=2, neg_imm=True))
    return out


def _dopri5_cases():
    """First step size detached (the hill2_k1 body), then attached (dp_initbwd) with every body: K cycles through 0, 2, 3."""
    out, i = [], 0
    for D in (4, 6, 8, 12):
        for lanes in ((1, 4) if D in (8, 12) else (1,)):
            for ablate in (False, True):
                for nt in (False, True):
                    c = dict(family="dopri5", D=D, lanes=lanes, ablate=ablate, need_theta=nt)
                    out.append(dict(c, detach=True, theta="default", n_dose=1))
                    out.append(dict(c, detach=False, theta="default", n_dose=1))
                    out.append(dict(c, detach=False, theta="default", n_dose=(0, 2, 3)[i % 3]))
                    if not ablate:
                        out.append(dict(c, detach=False, theta="general", hill=GENERAL_HILL[i % 3],
                                        n_dose=(2, 3, 0)[(i // 3) % 3]))
                    i += 1
    # hill_ulp without doses: a smooth problem, so the exponent's ulp cannot flip an accept / reject decision at a jump
    out.append(dict(family="dopri5", D=8, lanes=4, ablate=False, need_theta=True, detach=False, theta="hill_ulp", n_dose=0))
    out.append(dict(family="dopri5", D=6, lanes=1, ablate=False, need_theta=True, detach=False, theta="hill_ulp", n_dose=0))
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
        return dopri5_kernels(case["D"], case["lanes"], case["ablate"], case["need_theta"], case["detach"], DOPRI5_N)
    raise ValueError(f)


# keys left out of a case id at these values: the calls the table held before it named rhs bodies (hill2_k1: default
# theta, one dose; dopri5 with the first step detached) keep their test ids
_ID_DEFAULTS = {"theta": "default", "n_dose": 1, "detach": True}


def case_id(case):
    return "-".join("%s=%s" % (k, v) for k, v in case.items() if not (k in _ID_DEFAULTS and v == _ID_DEFAULTS[k]))


# compiled instantiations no dispatch of the library reaches (name -> reason)
_NO_EULER_TAPE = ("euler has no intermediate stage to tape: the tape pointer is NULL (csrc/hode_rk_split.hip:1189-1201), "
                  "so HODE_FLAG_TAPE launches the TAPE=false kernel")
UNREACHABLE = {}
for _D in (8, 12):
    for _a in ("false", "true"):
        UNREACHABLE["hode::split_fwd_kernel<%d, 0, %s, true>" % (_D, _a)] = _NO_EULER_TAPE
        for _nt in ("false", "true"):
            UNREACHABLE["hode::split_bwd_kernel<%d, 0, %s, %s, true>" % (_D, _a, _nt)] = _NO_EULER_TAPE
_NO_PERSIST = ("the persistent attempt loop is launched only by builds with -DHODE_DP_EXPERIMENTS and HODE_DP_PERSIST=1 "
               "(csrc/hode_dopri5.hip:195-197); the product build compiles it but never launches it")
for _D in (8, 12):
    for _a in ("false", "true"):
        UNREACHABLE["hode::dp_persist_kernel<%d, %s>" % (_D, _a)] = _NO_PERSIST

# (instantiation, body) pairs of reachable instantiations that no dispatch of the library reaches ((name, body) -> reason).
# Empty: ablate instantiations hold no general body (bodies()), and every other pair has a call.
UNREACHABLE_BODIES = {}
