"""The calls that test libhode's two metric kernels, `hode::crps_kernel` (csrc/hode_crps.hip) and `hode::mc_kl_exp_kernel`
(csrc/hode_mckl.hip), and the host rules of the CRPS entry point restated in Python.  A plain helper module, not a
conftest, in the style of tests/kernel_variants.py.

* tests/test_metric_case_coverage.py (CPU) pins the restated rules to the source, reads the kernel's static LDS out of
  its descriptor, and checks that the tables reach every regime and edge listed below.
* tests/test_hip_metric_cases.py (GPU) runs every entry through the C ABI against float64.

CRPS entries: shape (Tn, B, M, Dv, obs), readout (identity: h_m[:obs]; affine: W h_m + b; linear: W h_m, no bias),
outputs (crps: the (Tn, B, obs) field; sum: the per-row sum; both in one call), the layout of h in memory, and the values:
  member   h[t][m * B + b][d]: what hode.crps.ensemble_crps passes
  patient  h[t][b][m][d]
  padded   member-major with patient_stride > Dv and a gap between members and between times (NaN in every gap)
  slice    member-major, starting at time 2 of a longer buffer: what evaluate() passes as h[t0:]
  normal        standard-normal members and truth
  tied          every member equal: CRPS = |x - y|
  truth_member  the truth equal to one member (exact, identity readout)
  zero_spread   every member equal to the truth: CRPS = 0 exactly (identity readout)
  offset        members and truth at 1e3 with a spread of 1e-2 (identity readout: exact fp32 inputs, so any cancellation
                in the kernel shows against a tolerance scaled to the spread)

MC-KL entries: rows (B * D elements), S draws, rate, clamp value, the log_var range, the mu regime (positive: every draw
z > 0; clamped: every z <= 0; mix; zero: a mix plus rows with mu = 0, log_var = 0 and noise = +0.0 / -0.0, so z = 0
exactly and both sides clamp), and which gradient buffers the call passes (both, mu, lv, none: the forward-only path).
"""

CRPS_THREADS = 128                   # kCrpsThreads, csrc/hode_crps.hip
CRPS_MAX_DIM = 128                   # obs_dim, n_members and latent_dim bound
CRPS_LDS_LIMIT = 160 * 1024          # the host's refusal bound, = the LDS of one gfx950 CU
CRPS_ATTR_ABOVE = 64 * 1024          # above this the host raises hipFuncAttributeMaxDynamicSharedMemorySize
READOUTS = ("identity", "affine", "linear")
OUTPUTS = ("crps", "sum", "both")
LAYOUTS = ("member", "patient", "padded", "slice")
VALUES = ("normal", "tied", "truth_member", "zero_spread", "offset")


def crps_lds_bytes(M, Dv, readout):
    """csrc/hode_crps.hip, hode_ensemble_crps: the kernel's whole LDS (all of it dynamic) --
    M * Dv member vectors, Dv * 128 transposed readout (with a weight), M * 128 ensemble values, 2 wave partials."""
    return 4 * (M * Dv + (Dv * CRPS_THREADS if readout != "identity" else 0) + M * CRPS_THREADS + CRPS_THREADS // 64)


def crps_accepts(M, Dv, obs, readout):
    """The host's checks in order: dimensions, identity width, LDS bound (True = launched)."""
    if min(M, Dv, obs) < 1 or obs > CRPS_THREADS or M > CRPS_MAX_DIM or Dv > CRPS_MAX_DIM:
        return False
    if readout == "identity" and Dv < obs:
        return False
    return crps_lds_bytes(M, Dv, readout) <= CRPS_LDS_LIMIT


def crps_regime(c):
    """'small' (no attribute call) or 'attr' (the host raises the dynamic-LDS limit first)."""
    return "attr" if crps_lds_bytes(c["M"], c["Dv"], c["readout"]) > CRPS_ATTR_ABOVE else "small"


# the three largest shapes with a weight the host accepts, and the smallest it refuses past them (M, Dv)
CRPS_LARGEST = ((95, 128), (127, 96), (128, 95))
CRPS_REFUSED = ((96, 128), (128, 96), (128, 128))

# sim configs (sim_config.py DataConfig / dim8_config / dim12_config): obs_dim / latent_dim, and the ensemble sizes of
# evaluate (mc_itr 50) and evaluate_horizon (mc_itr 10); expert_dim 4 is the width crps_z0 scores
SIM_SHAPES = ((20, 6), (40, 8), (80, 12))
SIM_MEMBERS = (50, 10)
EXPERT_DIM = 4
SIM_TN, SIM_B = 10, 50  # t_max 14, t0 5: 10 forecast steps; test batch 50


def _crps(Tn, B, M, Dv, obs, readout="affine", out="both", layout="member", values="normal", note=""):
    return {"kernel": "crps", "Tn": Tn, "B": B, "M": M, "Dv": Dv, "obs": obs, "readout": readout, "out": out,
            "layout": layout, "values": values, "note": note}


CRPS_CASES = []
# the product calls: evaluate / evaluate_horizon (affine readout of the latent trajectory, crps_sum) and crps_z0
for _obs, _D in SIM_SHAPES:
    for _M in SIM_MEMBERS:
        CRPS_CASES.append(_crps(SIM_TN, SIM_B, _M, _D, _obs, "affine", "sum", "member", note="eval"))
    CRPS_CASES.append(_crps(1, SIM_B, 50 if _D != 8 else 10, _D, EXPERT_DIM, "identity", "sum", "member", note="z0"))
CRPS_CASES += [
    # LDS regimes: above 64 KiB (attribute call), and the three largest accepted shapes
    _crps(3, 5, 64, 128, 65, "affine", "both", "patient"),
    _crps(2, 3, 95, 128, 128, "affine", "both", "member"),
    _crps(2, 3, 127, 96, 127, "linear", "crps", "padded"),
    _crps(2, 3, 128, 95, 64, "affine", "sum", "slice"),
    # identity at full width (obs = Dv = 128), 127 members, above 64 KiB
    _crps(2, 4, 127, 128, 128, "identity", "both", "patient"),
    # component counts around the wave: 1, 63 (sum of one partial wave), 64 (exactly one wave), 65
    _crps(3, 7, 2, 1, 1, "identity", "both", "member"),
    _crps(4, 9, 50, 16, 63, "affine", "sum", "padded"),
    _crps(4, 9, 17, 16, 64, "linear", "both", "slice"),
    _crps(3, 11, 64, 32, 65, "affine", "sum", "member"),
    # one member (plain absolute error) at the widest readout; 128 members of width 1
    _crps(3, 5, 1, 128, 100, "affine", "both", "padded"),
    _crps(3, 5, 128, 1, 1, "identity", "crps", "slice"),
    _crps(2, 6, 128, 24, 33, "linear", "sum", "patient"),
    # a grid of more than 65 535 rows, B prime
    _crps(93, 1009, 2, 3, 3, "affine", "both", "member"),
    # values
    _crps(3, 7, 50, 8, 40, "affine", "both", "patient", "tied"),
    _crps(3, 7, 33, 12, 12, "identity", "both", "padded", "tied"),
    _crps(3, 7, 17, 12, 10, "identity", "both", "slice", "truth_member"),
    _crps(3, 7, 50, 12, 12, "identity", "both", "member", "zero_spread"),
    _crps(3, 7, 64, 20, 20, "identity", "both", "patient", "offset"),
    _crps(2, 5, 128, 96, 96, "identity", "both", "member", "offset"),
]


def crps_id(c):
    return "crps-T%d-B%d-M%d-Dv%d-obs%d-%s-%s-%s-%s" % (c["Tn"], c["B"], c["M"], c["Dv"], c["obs"], c["readout"],
                                                       c["out"], c["layout"], c["values"])


def _mckl(rows, S, rate=100.0, clamp="eps", lv=(-9.0, -7.0), mu="mix", grads="both"):
    return {"kernel": "mckl", "rows": rows, "S": S, "rate": rate, "clamp": clamp, "lv": lv, "mu": mu, "grads": grads}


# clamp values: "eps" is torch.finfo(torch.float32).eps, the reference's
CLAMPS = {"eps": 1.1920928955078125e-07, "zero": 0.0, "1e-3": 1e-3}
BIG_ROWS = (1 << 20) + 77  # ragged against the 256-thread block

MCKL_CASES = [
    _mckl(1, 100, 100.0, "eps", (-8.0, -8.0), "mix", "both"),
    _mckl(255, 17, 100.0, "eps", (-20.0, -12.0), "clamped", "lv"),
    _mckl(256, 1000, 1.0, "1e-3", (-4.0, 4.0), "mix", "mu"),
    _mckl(257, 2, 0.5, "zero", (-2.0, 2.0), "positive", "none"),
    _mckl(257, 100, 100.0, "eps", (-9.0, -7.0), "zero", "both"),
    _mckl(256, 17, 1.0, "zero", (-1.0, 1.0), "zero", "mu"),
    _mckl(255, 1, 0.5, "1e-3", (-20.0, 4.0), "positive", "both"),
    _mckl(257, 1000, 100.0, "eps", (-20.0, -6.0), "positive", "lv"),
    _mckl(255, 2, 1.0, "eps", (0.0, 4.0), "clamped", "none"),
    _mckl(256, 100, 0.5, "zero", (-6.0, 0.0), "clamped", "mu"),
    _mckl(BIG_ROWS, 2, 100.0, "eps", (-20.0, 4.0), "mix", "both"),
    _mckl(BIG_ROWS, 1, 1.0, "1e-3", (-8.0, 2.0), "zero", "none"),
]


def mckl_id(c):
    return "mckl-rows%d-S%d-rate%g-clamp%s-lv%g..%g-%s-grad_%s" % (c["rows"], c["S"], c["rate"], c["clamp"], c["lv"][0],
                                                                  c["lv"][1], c["mu"], c["grads"])
