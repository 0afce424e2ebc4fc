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
            "dp_persist_kernel",
            # NeuralODE rhs: fixed grid (matrix-core and lane layouts), dopri5
            "neural_mf_fwd_kernel", "neural_mf_bwd_kernel", "neural_grad_fold_kernel", "neural_fwd_kernel",
            "neural_bwd_kernel", "transpose_w2_kernel", "ndp_fwd_kernel", "ndp_bwd_kernel", "ndp_initbwd_kernel",
            # LSTM encoder
            "lstm_fwd_kernel", "lstm_bwd_kernel", "lstm_fill_operand_kernel", "lstm_pack_kernel", "lstm_pack_hh_kernel",
            # readouts
            "readout_sse_kernel", "readout_mf_kernel", "readout_fold_kernel", "readout_mlp_kernel", "readout_mlp_fold_kernel")
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
    (D = 4, D = 20 with H > 64) runs csrc/hode_real.hip:377-385 real_kernel<D, METHOD, BWD>."""
    if D == 20 and 1 <= H <= 64:
        ht = real_mf_ht(H)
        out = ["hode::real_mf_kernel<%d, %d, false, false>" % (ht, method),
               "hode::real_mf_kernel<%d, %d, true, %s>" % (ht, method, _b(onchip))]
        return out + (["hode::real_grad_fold_kernel<%d>" % ht] if onchip else [])
    return ["hode::real_kernel<%d, %d, false>" % (D, method), "hode::real_kernel<%d, %d, true>" % (D, method)]


def choose_lpp(D, lanes, B):
    """csrc/hode_api.hip:66 choose_lpp."""
    can4 = D > 4 and (D - 4) % 4 == 0
    if lanes == 1:
        return 1
    if lanes == 4:
        return 4 if can4 else 1
    if not can4:
        return 1
    return 1 if B >= 131072 else 4


def roche_layout(D, lanes, T):
    """csrc/hode_api.hip:121 use_split (D 8 / 12, T <= kSplitMaxT, lanes 48 or 0; the backward needs T >= 2), :109 use_mf
    (D 8 / 12 / 16 and lanes 16), else the per-dimension lane kernels (:132 dispatch_dim)."""
    if D in (8, 12) and T <= SPLIT_MAX_T and T >= 2 and lanes in (0, 48):
        return "split"
    if D in (8, 12, 16) and lanes == 16:
        return "mf"
    return "lane"


def roche_fixed(D, lanes, method, ablate, need_theta, tape=True, T=8, B=77):
    """Fixed-grid Roche forward + backward as hode.plan.RocheRKPlan launches them (tape = HODE_FLAG_TAPE).
    split: csrc/hode_rk_split.hip:1133-1168 split_method / split_bwd_method (the tape pointer selects TAPE, need_theta_grad
    NEED_TH) and the fold :1228.  mf: csrc/hode_rk_mf.hip:554-575 mf_launch / mf_dim and the fold :597.  lane kernels:
    csrc/hode_rk_kernels.hpp:384 dispatch_lpp (LPP 4 only where (D-4) % 4 == 0), :368 dispatch_method, :360 launch_bwd."""
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
    """One adaptive solve + its backward.  LPP = choose_lpp (csrc/hode_dopri5.hip:158, :254) -> csrc/hode_dopri5_kernels.hpp
    dp_dispatch (LPP 4 only where (D-4) % 4 == 0) -> dp_launch: the forward's phases 0 / 1 (initial step) and 2 (attempts),
    dp_fwd_kernel<D, LPP, ABLATE, PHASE>; the backward sweep, dp_bwd_kernel<D, LPP, ABLATE, NEED_TH>; and unless the first
    step size is detached (csrc/hode_dopri5.hip:263) the two passes of its backward, dp_initbwd_kernel<D, LPP, ABLATE,
    false, 1> (pass 1 forms a scalar: always NEED_TH = false) and dp_initbwd_kernel<D, LPP, ABLATE, NEED_TH, 2>."""
    lpp, a = choose_lpp(D, lanes, B), _b(ablate)
    out = ["hode::dp_fwd_kernel<%d, %d, %s, %d>" % (D, lpp, a, ph) for ph in (0, 1, 2)]
    out.append("hode::dp_bwd_kernel<%d, %d, %s, %s>" % (D, lpp, a, _b(need_theta)))
    if not detach_first_step:
        out += ["hode::dp_initbwd_kernel<%d, %d, %s, false, 1>" % (D, lpp, a),
                "hode::dp_initbwd_kernel<%d, %d, %s, %s, 2>" % (D, lpp, a, _b(need_theta))]
    return out


def neural_layout(D, lanes=0):
    """csrc/hode_neural.hip:356-359 neural_rk: the one-patient-per-lane kernels when lanes_per_patient == 1 (:272
    neural_lanes; compiled for D = 6, 8, 12 only, anything else is a configuration error); the matrix-core kernels for
    0 and 16."""
    if lanes == 1:
        assert D in (6, 8, 12), D
        return "lane"
    return "mf"


def neural_fixed(D, method, lanes=0, onchip=True):
    """Fixed-grid NeuralODE forward + backward (onchip = the caller hands grad_w1, hode.neural's default).
    mf: csrc/hode_neural_mf_kernels.hpp launch_neural_mf_d: grid ceil(B/16); neural_mf_bwd_kernel<D, M, ONCHIP> with
    ONCHIP = bwd && grad_w1, and the on-chip backward folds its per-wave partials with neural_grad_fold_kernel<D>.
    lane: csrc/hode_neural.hip:320-330 launch_neural: grid ceil(B/64), after transpose_w2_kernel (:360, every
    call); its backward always writes the operand tapes (csrc/hode_neural.hip:276 neural_onchip)."""
    if neural_layout(D, lanes) == "lane":
        return ["hode::transpose_w2_kernel", "hode::neural_fwd_kernel<%d, %d>" % (D, method),
                "hode::neural_bwd_kernel<%d, %d>" % (D, method)]
    out = ["hode::neural_mf_fwd_kernel<%d, %d>" % (D, method),
           "hode::neural_mf_bwd_kernel<%d, %d, %s>" % (D, method, _b(onchip))]
    return out + (["hode::neural_grad_fold_kernel<%d>" % D] if onchip else [])


def neural_lanes(case):
    """lanes_per_patient that forces a neural case's layout: 1 for "lane"; "mf" is what the library chooses (0)."""
    return 1 if case["layout"] == "lane" else 0


def neural_grid(B, layout):
    """Workgroups of one launch: csrc/hode_neural_mf_kernels.hpp launch_neural_mf_d (16 patients per wave), csrc/hode_neural.hip:321 (64)."""
    return (B + 15) // 16 if layout == "mf" else (B + 63) // 64


NEURAL_DOPRI5_DIMS = (4, 6, 8, 10, 12, 14)  # csrc/hode_host.hpp HODE_NEURAL_DIMS


def neural_dopri5_kernels(D, n_acc, detach_first_step):
    """csrc/hode_neural_dopri5_kernels.hpp nd_fwd: phases 0 / 1 (initial step) and 2 (attempts) of ndp_fwd_kernel<D, PHASE>;
    nd_bwd (same header): ndp_bwd_kernel<D> and the fold of its partials, then, when a step was accepted (n_acc > 0) and the
    first step size is not detached (HODE_FLAG_DETACH_FIRST_STEP), ndp_initbwd_kernel<D, 1>, <D, 2> and the fold again."""
    out = ["hode::ndp_fwd_kernel<%d, %d>" % (D, ph) for ph in (0, 1, 2)]
    out += ["hode::ndp_bwd_kernel<%d>" % D, "hode::neural_grad_fold_kernel<%d>" % D]
    if n_acc > 0 and not detach_first_step:
        out += ["hode::ndp_initbwd_kernel<%d, 1>" % D, "hode::ndp_initbwd_kernel<%d, 2>" % D]
    return out


LSTM_SIZES = (16, 32, 48, 64, 80, 96, 128, 160)  # csrc/hode_lstm.hip:85 kSizes
LSTM_TPWS = tuple(h // 16 for h in LSTM_SIZES)   # build_hip.py LSTM_TPWS: one hode_lstm_tpw.hip unit per padded size


def choose_nt(B, save_tape):
    """csrc/hode_lstm.hip:71-80 choose_nt: NT <= 3 with a tape (the backward's limit), <= 4 without; the smallest
    ceil(ceil(B / 16 nt) / 256) * nt, ties to the larger NT."""
    best, best_cost = 1, None
    for nt in range(1, (3 if save_tape else 4) + 1):
        blocks = (B + 16 * nt - 1) // (16 * nt)
        cost = ((blocks + 255) // 256) * nt
        if best_cost is None or cost <= best_cost:
            best, best_cost = nt, cost
    return best


def lstm_geom(H, obs, B, save_tape, patient_tiles=0):
    """csrc/hode_lstm.hip:82-122 lstm_geom -> (Hp, TPW, fTPW, fNW, NT): Hp the next compiled size, TPW = Hp / 16; the
    forward runs fNW = 4 waves of TPW tiles for TPW <= 5, else 8 waves of TPW / 2 (csrc/hode_lstm_tpw.hip:18-19); NT from
    choose_nt, the patient_tiles override inside the same bound (:96-97), then the staging clamp 16 NT obs <= 5120 (:106)."""
    Hp = next(v for v in LSTM_SIZES if H <= v)
    tpw = Hp // 16
    fnw = 4 if tpw <= 5 else 8
    nt = choose_nt(B, save_tape)
    if 1 <= patient_tiles <= (3 if save_tape else 4):
        nt = patient_tiles
    while nt > 1 and 16 * nt * obs > 5120:
        nt -= 1
    return Hp, tpw, 4 * tpw // fnw, fnw, nt


def lstm_kernels(H, obs, B, save_tape, patient_tiles=0):
    """hode_lstm_fwd (csrc/hode_lstm.hip:169 lstm_pack_kernel, then csrc/hode_lstm_tpw.hip:33-35
    lstm_fwd_kernel<NT, fTPW, fNW, VEC4 = obs % 4 == 0, PAD = H != 16 TPW>, csrc/hode_lstm_tpw.hip launch_fwd_pad); with the tape (hode.lstm.lstm_encode) also hode_lstm_bwd
    (csrc/hode_lstm.hip:217 lstm_pack_hh_kernel, csrc/hode_lstm_tpw.hip:47-49 lstm_bwd_kernel<NT, TPW, FLAT = H == 16 TPW>)
    and hode_lstm_fill_operand (csrc/hode_lstm.hip:268-274 lstm_fill_operand_kernel<VEC4>: obs % 4 == 0 and 16-byte
    aligned x / mask / h_prev, which fresh tensors are)."""
    _, tpw, ftpw, fnw, nt = lstm_geom(H, obs, B, save_tape, patient_tiles)
    vec4 = _b(obs % 4 == 0)
    out = ["hode::lstm_pack_kernel", "hode::lstm_fwd_kernel<%d, %d, %d, %s, %s>" % (nt, ftpw, fnw, vec4, _b(H != 16 * tpw))]
    if save_tape:
        out += ["hode::lstm_pack_hh_kernel", "hode::lstm_bwd_kernel<%d, %d, %s>" % (nt, tpw, _b(H == 16 * tpw)),
                "hode::lstm_fill_operand_kernel<%s>" % vec4]
    return out


def lstm_workspace_bytes(T, B, I, H, obs, save_tape, patient_tiles=0):
    """csrc/hode_lstm.hip:150-156 hode_lstm_workspace_bytes from the restated geometry: [packed W (4 KQ4 TPW 64 4 floats,
    Kq = ceil((I + Hp + 1) / 4), KQ4 = ceil(Kq / 4)) | packed W_hh^T | tape (T nblk 4 TPW NT 5 64 floats)], 256-aligned."""
    Hp, tpw, _, _, nt = lstm_geom(H, obs, B, save_tape, patient_tiles)
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    kq = (I + Hp + 1 + 3) // 4
    kq4 = (kq + 3) // 4
    # csrc/hode_lstm.hip:111-113: the LDS bound of the launched (clamped) tile, 0 = unsupported
    if 2 * 4 * kq * (16 * nt + (16 if (16 * nt) % 32 == 0 else 0)) * 4 > 160 * 1024:
        return 0
    n = al(4 * kq4 * tpw * 64 * 4 * 4)
    if save_tape:
        nblk = (B + 16 * nt - 1) // (16 * nt)
        n += al(4 * tpw * 4 * ((tpw + 3) // 4) * 64 * 4 * 4) + al(T * nblk * 4 * tpw * nt * 5 * 64 * 4)
    return n


READOUT_VARIANT_VALU = 1  # include/hode.h HODE_READOUT_VARIANT_VALU


def readout_mf(latent, obs, variant=0):
    """csrc/hode_readout.hip:292-295 readout_mf: the matrix-core kernel for (12, 48 < obs <= 80) and (8, 32 < obs <= 48),
    unless the descriptor's variant is HODE_READOUT_VARIANT_VALU."""
    if variant == READOUT_VARIANT_VALU:
        return False
    return (latent == 12 and 48 < obs <= 80) or (latent == 8 and 32 < obs <= 48)


def readout_kernels(latent, obs, grad, variant=0):
    """csrc/hode_readout.hip:330-353 hode_readout_sse: readout_mf_kernel<12, 5, GRAD> / <8, 3, GRAD> or
    readout_sse_kernel<D, GRAD> (GRAD = grad_h given), then readout_fold_kernel (grid P with the gradient, 1 without)."""
    g = _b(grad)
    if readout_mf(latent, obs, variant):
        k = "hode::readout_mf_kernel<%s, %s>" % ("12, 5" if latent == 12 else "8, 3", g)
    else:
        k = "hode::readout_sse_kernel<%d, %s>" % (latent, g)
    return [k, "hode::readout_fold_kernel"]


def readout_waves(rows, obs, latent, variant=0):
    """csrc/hode_readout.hip:297-301 readout_waves: 16 rows per wave-iteration on the matrix cores, 64 / (obs / 4) on the
    lanes; at most 2048 waves."""
    rpi = 16 if readout_mf(latent, obs, variant) else 64 // (obs // 4)
    return max(1, min((rows + rpi - 1) // rpi, 2048))


def readout_mlp_kernels(latent, grad):
    """csrc/hode_readout_mlp.hip:326-334: DL = 20 if latent == 20 else 4; readout_mlp_kernel<DL, 24, GRAD> and
    readout_mlp_fold_kernel<DL, 24>."""
    dl = 20 if latent == 20 else 4
    return ["hode::readout_mlp_kernel<%d, 24, %s>" % (dl, _b(grad)), "hode::readout_mlp_fold_kernel<%d, 24>" % dl]


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
    csrc/hode_rk_kernels.hpp:136-140 (rk_fwd_kernel), :339-342 (rk_bwd_kernel); csrc/hode_rk_split.hip:1115-1118
    (split_bwd_kernel), :1123-1126 (split_fwd_kernel); csrc/hode_rk_mf.hip:245-248 (mf_fwd_kernel), :498-501
    (mf_bwd_kernel); csrc/hode_dopri5_kernels.hpp:876-879 (dp_persist_kernel), :886-896 (dp_fwd_kernel; its attempt
    launches take hill2 from the host's read-back of the same comparison, csrc/hode_dopri5.hip:174-180), :1361-1369
    (dp_bwd_kernel), :1502-1505 (dp_initbwd_kernel).  ABLATE forces hill2: the ablate rhs has no Hill terms."""
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


NEURAL_STEP = 0.375  # fixed-grid step of the NeuralODE cases: 3/8, so t0 + dt/3 is a representable fp32 (and fp64) stage time


def substantive(case):
    """A case where the kernel's arithmetic really runs: T >= 3 (at least two steps / recurrences: the LSTM's W_hh product
    multiplies the zero initial state at the first one) and a batch of more than one full 16-patient tile with a ragged
    last one.  The guard requires every instantiation of the NeuralODE, LSTM and readout families to be reached by one;
    T = 1 and B = 1 entries come on top."""
    return case["T"] >= 3 and case["B"] > 16 and case["B"] % 16 != 0


def _neural_cases():
    """Every matrix-core (D, method) with the on-chip and the tape-writing backward, every lane-layout (D, method), each at
    T = 6 on a ragged batch (B in {65, 100, 37, 129}: ragged against 16 and 64; 65 is one past a lane wave); perturb and the
    dose list (n_dose 0, 1, 3 on the grid) cycle.  Extra: two equal dose times ("dup": the impulse counts twice), a dose time
    on the rk4 1/3 stage ("third"), and the degenerate B = 1 and T = 1 (no step) calls of each layout."""
    out, i = [], 0
    for D in (4, 6, 8, 10, 12, 14):
        for method in ("euler", "midpoint", "rk4"):
            for onchip in (True, False):
                out.append(dict(family="neural", D=D, method=method, layout="mf", onchip=onchip, B=(65, 100, 37, 129)[i % 4],
                                T=6, perturb=bool((i // 2) % 2), n_dose=(0, 1, 3)[(i + i // 3) % 3], dose="grid"))
                i += 1
    for D in (6, 8, 12):
        for method in ("euler", "midpoint", "rk4"):
            out.append(dict(family="neural", D=D, method=method, layout="lane", onchip=False, B=(65, 130, 37)[i % 3],
                            T=6, perturb=bool(i % 2), n_dose=(0, 1, 3)[i % 3], dose="grid"))
            i += 1
    for D, layout, onchip, method in ((14, "mf", True, "rk4"), (14, "mf", False, "rk4"), (12, "lane", False, "rk4"),
                                      (10, "mf", True, "midpoint"), (8, "lane", False, "midpoint")):
        for dose in ("dup", "third"):
            if dose == "third" and method != "rk4":
                continue
            out.append(dict(family="neural", D=D, method=method, layout=layout, onchip=onchip, B=37, T=5, perturb=False,
                            n_dose=2, dose=dose))
    for D, layout, onchip, method in ((4, "mf", True, "midpoint"), (14, "mf", False, "rk4"), (6, "lane", False, "euler")):
        for B, T in ((1, 6), (37, 1), (1, 1)):
            out.append(dict(family="neural", D=D, method=method, layout=layout, onchip=onchip, B=B, T=T, perturb=True,
                            n_dose=1, dose="grid"))
    return out


def _neural_dopri5_cases():
    """Every compiled D with the first step size detached and attached on ragged batches (17 is one past a wave); then
    B = 1, and one output time (no accepted step: the attached backward has nothing to do and is not launched)."""
    out = []
    for i, D in enumerate(NEURAL_DOPRI5_DIMS):
        for detach in (True, False):
            out.append(dict(family="neural_dopri5", D=D, detach=detach, B=(17, 70, 33, 65, 45)[(2 * i + detach) % 5], T=14))
    out.append(dict(family="neural_dopri5", D=12, detach=False, B=1, T=14))
    out.append(dict(family="neural_dopri5", D=8, detach=False, B=5, T=1))
    return out


LSTM_OBS_VEC4, LSTM_OBS_ODD = 20, 23


def _lstm_cases():
    """Per padded hidden size (TPW): the tape path (lstm_encode) at NT 1, 2, 3 once with H = 16 TPW and obs % 4 != 0,
    once with H = 16 TPW - 3 and obs % 4 == 0 -- every (NT, FLAT) backward -- and the no-tape path (lstm_final_state) at
    NT = 4 with both obs; NT forced by patient_tiles on a batch ragged against 16 NT, T = 3 or 4.  Then the no-tape path at
    every NT with the other obs of each, so that every (NT, VEC4, PAD) forward runs (PAD = padded hidden units).
    Then NT chosen by choose_nt from the batch size alone (1: B = 100; 2: 4097; 3: 8193; 4: 12289 without a tape), the
    staging clamp (obs = 100 lowers a forced NT = 4 to 3, at the largest hidden size too), and B = 1 / T = 1 calls."""
    out = []
    for j, tpw in enumerate(LSTM_TPWS):
        for nt in (1, 2, 3, 4):
            for flat in (True, False):
                tape = nt <= 3
                H = 16 * tpw if flat else 16 * tpw - 3
                obs = (LSTM_OBS_ODD if flat else LSTM_OBS_VEC4) if tape else (LSTM_OBS_VEC4 if flat else LSTM_OBS_ODD)
                out.append(dict(family="lstm", H=H, obs=obs, B=32 * nt + 5 + j, T=3 + (j + nt + flat) % 2, tape=tape, nt=nt))
    # the forward's PAD (padded hidden units: H != 16 TPW) with the other obs, so that every (NT, VEC4, PAD) forward runs
    for j, tpw in enumerate(LSTM_TPWS):
        for nt in (1, 2, 3, 4):
            for flat in (True, False):
                tape = nt <= 3
                obs = (LSTM_OBS_VEC4 if flat else LSTM_OBS_ODD) if tape else (LSTM_OBS_ODD if flat else LSTM_OBS_VEC4)
                out.append(dict(family="lstm", H=16 * tpw if flat else 16 * tpw - 5, obs=obs, B=32 * nt + 3 + j, T=3 + (j + nt) % 2,
                                tape=False, nt=nt))
    for B, tape in ((100, True), (4097, True), (8193, True), (100, False), (4097, False), (8193, False), (12289, False)):
        out.append(dict(family="lstm", H=13, obs=LSTM_OBS_VEC4, B=B, T=3, tape=tape, nt=None))
    for H in (40, 150):
        out.append(dict(family="lstm", H=H, obs=100, B=150, T=3, tape=False, nt=4))
    for H, tape, nt in ((160, True, 3), (64, False, 4), (13, True, None)):
        for B, T in ((1, 3), (37, 1), (1, 1)):
            out.append(dict(family="lstm", H=H, obs=LSTM_OBS_ODD, B=B, T=T, tape=tape, nt=nt))
    return out


def _readout_cases():
    """Each latent dimension of the lane kernel, both sides of every readout_mf window edge (D 12: 48 | 52, 80 | 84; D 8:
    32 | 36, 48 | 52), the window with the lane kernel forced (variant), row counts at the 2048-wave cap; the MLP readout at both DL;
    then a single row.  Every case runs the call with and without the gradient (GRAD = true / false)."""
    out = []
    for D, obs, T, B in ((4, 20, 3, 21), (4, 128, 3, 33), (6, 20, 4, 17), (6, 92, 3, 21), (8, 32, 3, 19), (8, 36, 3, 23),
                         (8, 48, 4, 31), (8, 52, 3, 27), (12, 48, 3, 23), (12, 52, 3, 19), (12, 80, 3, 21), (12, 84, 3, 25),
                         (12, 80, 130, 257), (4, 20, 100, 257)):
        out.append(dict(family="readout", D=D, obs=obs, T=T, B=B, valu=False))
    out.append(dict(family="readout", D=12, obs=64, T=3, B=29, valu=True))
    out.append(dict(family="readout", D=8, obs=40, T=3, B=29, valu=True))
    out.append(dict(family="readout", D=8, obs=44, T=1, B=1, valu=False))
    for D, T, B in ((20, 7, 33), (4, 6, 17), (4, 96, 257), (20, 1, 1)):
        out.append(dict(family="readout_mlp", D=D, obs=24, T=T, B=B))
    return out


NEURAL_DIMS = (4, 6, 8, 10, 12, 14)  # csrc/hode_host.hpp HODE_NEURAL_DIMS (check_neural: even, 4..14)
NEURAL_LANE_DIMS = (6, 8, 12)        # csrc/hode_neural.hip:358-366
READOUT_LATENT = (4, 6, 8, 12)       # csrc/hode_readout.hip:342-347
NEW_FAMILIES = ("neural", "neural_dopri5", "lstm", "readout", "readout_mlp")  # CASES families of the kernels below


def instantiations():
    """Every name the NeuralODE, LSTM and readout rules above can produce, over the domains they restate (dimensions,
    methods, padded sizes, NT, flags): the guard compares it with the compiled symbols of these families."""
    out = set()
    for m in METHODS.values():
        for D in NEURAL_DIMS:
            out.update(neural_fixed(D, m, 0, True) + neural_fixed(D, m, 0, False))
        for D in NEURAL_LANE_DIMS:
            out.update(neural_fixed(D, m, 1))
    for D in NEURAL_DOPRI5_DIMS:
        out.update(neural_dopri5_kernels(D, 1, False))
    for tpw in LSTM_TPWS:
        fnw = 4 if tpw <= 5 else 8
        for nt in (1, 2, 3, 4):
            for v in (True, False):
                for pad in (True, False):
                    out.add("hode::lstm_fwd_kernel<%d, %d, %d, %s, %s>" % (nt, 4 * tpw // fnw, fnw, _b(v), _b(pad)))
                if nt <= 3:
                    out.add("hode::lstm_bwd_kernel<%d, %d, %s>" % (nt, tpw, _b(v)))
    out.update(["hode::lstm_pack_kernel", "hode::lstm_pack_hh_kernel", "hode::lstm_fill_operand_kernel<true>",
                "hode::lstm_fill_operand_kernel<false>"])
    for g in (True, False):
        for D in READOUT_LATENT:
            out.update(readout_kernels(D, 4, g))
        out.update(readout_kernels(12, 64, g) + readout_kernels(8, 40, g))
        out.update(readout_mlp_kernels(20, g) + readout_mlp_kernels(4, g))
    return out

ROCHE_N, ROCHE_T = 77, 8   # ragged batch (not a multiple of 16, 48 or 64), short grid
DOPRI5_N, DOPRI5_T = 21, 10

CASES = (_seqdec_cases() + _neural_real_cases() + _real_cases() + _roche_cases() + _dopri5_cases() + _neural_cases()
         + _neural_dopri5_cases() + _lstm_cases() + _readout_cases())


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
    if f == "neural":
        return neural_fixed(case["D"], METHODS[case["method"]], neural_lanes(case), case["onchip"])
    if f == "neural_dopri5":
        return neural_dopri5_kernels(case["D"], case["T"] - 1, case["detach"])
    if f == "lstm":
        return lstm_kernels(case["H"], case["obs"], case["B"], case["tape"], case["nt"] or 0)
    if f == "readout":
        v = int(case["valu"])  # valu=True: READOUT_VARIANT_VALU
        return readout_kernels(case["D"], case["obs"], True, v) + readout_kernels(case["D"], case["obs"], False, v)[:1]
    if f == "readout_mlp":
        return readout_mlp_kernels(case["D"], True) + readout_mlp_kernels(case["D"], False)[:1]
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
               "(csrc/hode_dopri5.hip:191-193); the product build compiles it but never launches it")
for _D in (8, 12):
    for _a in ("false", "true"):
        UNREACHABLE["hode::dp_persist_kernel<%d, %s>" % (_D, _a)] = _NO_PERSIST

# (instantiation, body) pairs of reachable instantiations that no dispatch of the library reaches ((name, body) -> reason).
# Empty: ablate instantiations hold no general body (bodies()), and every other pair has a call.
UNREACHABLE_BODIES = {}

# kernel symbols of the library outside FAMILIES -> the test that checks them against a float64 reference
# (tests/test_kernel_variant_coverage.py: every `.kd` symbol of the build is in FAMILIES or here)
OTHER_KERNELS = {
    # the metric kernels have a case table of their own (tests/metric_cases.py, guarded by tests/test_metric_case_coverage.py)
    "hode::crps_kernel": "tests/test_hip_metric_cases.py::test_crps_case",
    "hode::mc_kl_exp_kernel": "tests/test_hip_metric_cases.py::test_mckl_case",
    # the weight / theta gradient fold behind the Roche lane-kernel backward (csrc/hode_api.hip:249), the Roche dopri5
    # backward (csrc/hode_dopri5.hip:260, :270) and hode_real.hip (:412): every lane / dopri5 / real_kernel case runs it
    "hode::fold_partials_kernel": "tests/test_hip_kernel_variants.py::test_roche_fixed_grid",
}
