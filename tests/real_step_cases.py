"""The GPU case table of libhode_real_step.so (tests/test_hip_real_step.py) and the kernels each case launches: the one-step-
ahead solve of the real-data hybrid rhs (N independent intervals per patient, a start state each).  Restates, independently
of the library, which kernel csrc/real_step/ launches for a call: real_step_dose_kernel (the dose table, once per
direction), then real_step_kernel<HT, method, bwd> with HT = ceil(H / 16); every backward is followed by
real_step_fold_kernel<HT> (the flat weight gradient) and fold_partials_kernel (the three scalars).  The latent size, the
interval count N, the solver steps per interval S and the run length C are runtime arguments: they select no kernel.

Not a cross product.  Every case runs forward + backward.  The table holds every (HT, method) pair and the edge shapes
    D  5, 7, 8, 9, 12, 19, 20  M = D - 4 = 1, 3 (a partial quad), 4 (exactly one quad), 5, 8, 15, 16 (the full tile)
    H  1, 16, 17, 43, 64       the hidden-tile boundaries
    B  1, 15, 16, 17, 37       the wave boundary (16 patients per wave); more than one wave through the folds
    N  1, 2, 7                 intervals
    S  1, 2, 3                 solver steps per interval (step_size 1, 1/2, 1/3 on a unit grid)
    C  0 (the library's choice), 1, 2, 3, N, N + 2: runs that end inside N and exactly on it
Time axis of every case of this table: Ta = 12 action rows and the grid t = 4, 5, .., 4 + N, so that doses fall before and
inside the window; perturb is True for midpoint / rk4 and False for euler, as in tests/real_dims_cases.py.  On that unit
grid every row of the (N, S + 1) table is its neighbour shifted by 1 and all sub-steps are equal; intervals of different
lengths, a clipped last sub-step and the starts 0.0, 2.5 and -1.0 are tests/time_grids.py's real_step family
(tests/test_hip_time_grids.py)."""

METHODS = {"euler": 0, "midpoint": 1, "rk4": 2}
HTS = (1, 2, 3, 4)
MIN_LATENT, MAX_LATENT, MAX_HIDDEN, MAX_SUBSTEPS = 5, 20, 64, 8
TA, T_START = 12, 4               # t = arange(T_START, T_START + N + 1)

EDGE_D = (5, 7, 8, 9, 12, 19, 20)
EDGE_H = (1, 16, 17, 43, 64)
EDGE_B = (1, 15, 16, 17, 37)
EDGE_N = (1, 2, 7)
EDGE_S = (1, 2, 3)


def ht(H):
    """csrc/real_step/hode_real_step.hip hidden_tiles."""
    return (H + 15) // 16


def perturb(method):
    return method != "euler"


def _c(D, H, B, N, S, C, method):
    return dict(D=D, H=H, B=B, N=N, S=S, C=C, method=method, perturb=perturb(method))


#: (D, H, B, N, S, C, method)
CASES = [_c(*row) for row in (
    # one row per (HT, method)
    (5, 1, 17, 7, 1, 0, "euler"), (7, 16, 37, 7, 2, 2, "midpoint"), (8, 16, 15, 2, 1, 1, "rk4"),
    (9, 17, 16, 7, 3, 3, "euler"), (12, 17, 37, 1, 1, 0, "midpoint"), (19, 32, 1, 7, 2, 7, "rk4"),
    (20, 43, 37, 7, 1, 3, "euler"), (20, 43, 33, 7, 1, 0, "midpoint"), (7, 33, 17, 2, 3, 4, "rk4"),
    (12, 64, 15, 7, 2, 9, "euler"), (19, 49, 37, 2, 2, 1, "midpoint"), (5, 64, 16, 7, 1, 2, "rk4"),
    # the edge sizes again with other neighbours
    (8, 43, 1, 1, 3, 1, "midpoint"), (9, 1, 37, 7, 3, 2, "midpoint"), (20, 64, 17, 7, 3, 3, "rk4"), (19, 17, 15, 1, 2, 0, "euler"),
)]
#: the padding test: sentinels around h, grad_init, the flat weight gradient and the workspace
PADDING_CASES = [_c(5, 43, 17, 7, 2, 3, "midpoint"), _c(19, 43, 1, 2, 1, 1, "rk4"), _c(5, 17, 1, 7, 3, 0, "euler"),
                 _c(19, 16, 17, 7, 2, 2, "midpoint")]
#: S = 1 against the chained kernels, one real_solve per interval: libhode_real_dims.so (D <= 19) and libhode.so (D = 20)
COMPARE_CASES = [_c(7, 43, 17, 3, 1, 2, "midpoint"), _c(19, 16, 37, 2, 1, 0, "rk4"), _c(12, 64, 16, 3, 1, 1, "euler"),
                 _c(20, 43, 33, 3, 1, 0, "midpoint"), _c(20, 17, 17, 2, 1, 2, "rk4")]
#: the model-level test (DDW-shaped inputs: obs 24, statics 11, hidden 43, T 12, B 33)
MODEL_DIMS = (7, 20)
MODEL_STEP_DIVS = (1, 2)


def case_id(c):
    return "D%d-H%d-B%d-N%d-S%d-C%d-%s" % (c["D"], c["H"], c["B"], c["N"], c["S"], c["C"], c["method"])


def kernels(c):
    """Forward + backward of one call."""
    args = "%d, %d" % (ht(c["H"]), METHODS[c["method"]])
    return ["hode::real_step_dose_kernel", "hode::real_step_kernel<%s, false>" % args, "hode::real_step_kernel<%s, true>" % args,
            "hode::real_step_fold_kernel<%d>" % ht(c["H"]), "hode::fold_partials_kernel"]


def expected_kernels():
    """Every kernel symbol of the library: the dose prelude, HT x method x forward / backward, a fold per HT, the scalars' fold."""
    out = {"hode::fold_partials_kernel", "hode::real_step_dose_kernel"}
    for n in HTS:
        out.add("hode::real_step_fold_kernel<%d>" % n)
        out |= {"hode::real_step_kernel<%d, %d, %s>" % (n, m, b) for m in METHODS.values() for b in ("false", "true")}
    return out


def kernels_reached(cases=None):
    return {k for c in (CASES if cases is None else cases) for k in kernels(c)}


def wflat_len(D, H):
    return 9 * H + 2 + 3 * (D - 4) ** 2
