"""The GPU case table of libhode_lstm_seq.so (tests/test_hip_lstm_seq.py) and the kernels each case launches: the masked
LSTM window kernels under their all-steps policy (h of every step out, a cotangent on every step in).  Restates,
independently of the library, which kernel a call launches.  The geometry is the one csrc/hode_lstm.hip computes for
libhode.so too (the host code is compiled twice), restated in tests/kernel_variants.py lstm_geom: the padded hidden size
Hp = 16 TPW, the forward's fNW waves of fTPW tiles, NT forced by patient_tiles (1 .. 4 without a tape, 1 .. 3 with one).
    forward    lstm_pack_kernel, lstm_seq_fwd_kernel<NT, fTPW, fNW, VEC4 = obs % 4 == 0, PAD = H != 16 TPW>
    backward   lstm_pack_hh_kernel, lstm_seq_bwd_kernel<NT, TPW, FLAT = H == 16 TPW>, lstm_fill_operand_kernel<VEC4>

Not a cross product.  Every case has a batch ragged against its tile, B = 32 NT + 5 (more than one workgroup, the last one
partly filled).  FWD_CASES (forward only, no tape): every (TPW, NT 1 .. 4, VEC4); along the way T in 1 (no recurrence), 3
(the first shape with a middle step), 4; H = 16 TPW and 16 TPW - 3 (padded units); obs 20 / 23; with and without `a`, with
and without `mask`, both directions; PAD_FWD_CASES: the same calls with the other H of each, so that every forward runs with
and without padded hidden units.  BWD_CASES (forward with the tape + backward, T = 4): every (TPW, NT 1 .. 3, FLAT),
both directions, obs 20 / 23."""
import kernel_variants as kv

TPWS = kv.LSTM_TPWS                     # (1, 2, 3, 4, 5, 6, 8, 10)
MAX_HIDDEN = 160
OBS_VEC4, OBS_ODD = 20, 23
FWD_T = (1, 3, 4)
BWD_T = 4
#: parameter gradients against float64 autograd, rel-L2 (the bound of tests/test_hip_lstm.py)
GRAD_TOL = 1e-4


def batch(nt):
    return 32 * nt + 5


def _case(tpw, nt, flat, obs, T, a, mask, reverse, tape):
    return dict(H=16 * tpw - (0 if flat else 3), obs=obs, B=batch(nt), T=T, a=bool(a), mask=bool(mask), reverse=int(reverse),
                tape=bool(tape), nt=nt)


def _fwd_cases():
    out, k = [], 0
    for tpw in TPWS:
        for nt in (1, 2, 3, 4):
            for vec4 in (True, False):
                out.append(_case(tpw, nt, flat=(nt + int(vec4)) % 2 == 0, obs=OBS_VEC4 if vec4 else OBS_ODD, T=FWD_T[k % 3],
                                 a=(k // 2) % 2 == 0, mask=(k // 3) % 2 == 0, reverse=(k // 5) % 2, tape=False))
                k += 1
    return out


def _bwd_cases():
    out, k = [], 0
    for tpw in TPWS:
        for nt in (1, 2, 3):
            for flat in (True, False):
                out.append(_case(tpw, nt, flat, obs=OBS_VEC4 if (k // 2 + k) % 2 == 0 else OBS_ODD, T=BWD_T, a=k % 3 != 0,
                                 mask=(k // 2) % 2 == 0, reverse=(k + k // 6) % 2, tape=True))
                k += 1
    return out


def _pad_fwd_cases():
    """FWD_CASES pairs every (TPW, NT, VEC4) with one of H = 16 TPW and 16 TPW - 3; these are the other ones, so that every
    forward runs with and without padded hidden units (the kernels' PAD)."""
    return [_case(-(-c["H"] // 16), c["nt"], c["H"] % 16 != 0, c["obs"], 5 if c["T"] == 4 else c["T"], c["a"], c["mask"], c["reverse"], False)
            for c in _fwd_cases()]   # T = 5 for 4: BWD_CASES hold every T = 4 id


FWD_CASES = _fwd_cases()
PAD_FWD_CASES = _pad_fwd_cases()
BWD_CASES = _bwd_cases()
#: the bit-for-bit comparison with lstm_final_state / lstm_encode (libhode.so): a subset over the sizes, both directions
DIFF_CASES = [c for i, c in enumerate(BWD_CASES) if i % 5 == 0]
#: a cotangent that is nonzero on ONE middle row (catches a row added at the wrong step): T = 5, row 2
MIDDLE_CASES = [dict(_case(3, 2, False, OBS_VEC4, 5, True, True, r, True), row=2) for r in (0, 1)]
#: the cotangents autograd really produces: for h[:-1] a zero-padded contiguous tensor, for h.sum() an expanded one
AUTOGRAD_CASE = _case(3, 1, False, OBS_VEC4, 4, True, True, 0, True)
#: sentinels around h_all, grad_gates and h_prev
SENTINEL_CASE = dict(H=13, obs=OBS_ODD, B=21, T=3, a=True, mask=True, reverse=1, tape=True, nt=0)
#: the model-level test (DDW-shaped: obs 24, action 1, statics 11, hidden 44)
MODEL_SHAPE = dict(T=7, B=21, obs=24, action=1, statics=11, H=44)


def case_id(c):
    return "H%d-obs%d-B%d-T%d-nt%d-%s%s%s" % (c["H"], c["obs"], c["B"], c["T"], c["nt"], "a" if c["a"] else "",
                                               "m" if c["mask"] else "", "r" if c["reverse"] else "f")


def kernels(c):
    """The kernels of one call of the case: forward, and with a tape also the backward and the operand fill."""
    _, tpw, ftpw, fnw, nt = kv.lstm_geom(c["H"], c["obs"], c["B"], c["tape"], c["nt"])
    vec4 = kv._b(c["obs"] % 4 == 0)
    out = ["hode::lstm_pack_kernel", "hode::lstm_seq_fwd_kernel<%d, %d, %d, %s, %s>" % (nt, ftpw, fnw, vec4, kv._b(c["H"] != 16 * tpw))]
    if c["tape"]:
        out += ["hode::lstm_pack_hh_kernel", "hode::lstm_seq_bwd_kernel<%d, %d, %s>" % (nt, tpw, kv._b(c["H"] == 16 * tpw)),
                "hode::lstm_fill_operand_kernel<%s>" % vec4]
    return out


def expected_kernels():
    """Every kernel symbol of the library: the forward at NT 1 .. 4, the backward at NT 1 .. 3, the packers, the fill."""
    out = {"hode::lstm_pack_kernel", "hode::lstm_pack_hh_kernel", "hode::lstm_fill_operand_kernel<true>",
           "hode::lstm_fill_operand_kernel<false>"}
    for tpw in TPWS:
        fnw = 4 if tpw <= 5 else 8
        for v in ("true", "false"):
            out |= {"hode::lstm_seq_fwd_kernel<%d, %d, %d, %s, %s>" % (nt, 4 * tpw // fnw, fnw, v, pad) for nt in (1, 2, 3, 4)
                    for pad in ("true", "false")}
            out |= {"hode::lstm_seq_bwd_kernel<%d, %d, %s>" % (nt, tpw, v) for nt in (1, 2, 3)}
    return out


def kernels_reached(cases=None):
    return {k for c in (FWD_CASES + PAD_FWD_CASES + BWD_CASES if cases is None else cases) for k in kernels(c)}
