"""The GPU case table of libhode_real_dims.so (tests/test_hip_real_dims.py) and the kernels each case launches: the
real-data hybrid rhs (HODE_RHS_ROCHE_REAL) on the matrix cores at the latent sizes 5 .. 19, with 20 for the comparison
against libhode.so.  Restates, independently of the library, which kernel csrc/real_dims/ launches for a call: the
hidden-tile count HT = ceil(H / 16) and the method select real_dims_kernel<HT, method, bwd>; every backward is followed by
real_dims_fold_kernel<HT> (the flat weight gradient) and fold_partials_kernel (the three scalars).  The latent size is a
runtime argument: it selects no kernel.

Not a cross product.  Every case runs forward + backward.  The table holds every size 5 .. 19, every (HT, method) pair, and
the edge shapes
    D  5, 7, 8, 9, 19      M = D - 4 = 1, 3 (a partial quad), 4 (exactly one quad), 5, 15
    H  1, 16, 17, 43, 64   the hidden-tile boundaries
    B  1, 15, 16, 17, 37   the wave boundary (16 patients per wave); more than one wave through the fold
Time axis of every case of this table: Ta = 12 action rows and the grid t = 5, 6, .., 11 (six steps), so that doses fall
before and inside the window; perturb is True for midpoint / rk4 and False for euler, as in tests/test_hip_real.py.  That
is a unit grid (dt = 1, every stage of a step inside one hour); the library's kernels run on non-uniform and offset grids,
past the last action row and at negative times in tests/time_grids.py's real_dims family (tests/test_hip_time_grids.py)."""

DIMS = tuple(range(5, 20))        # what real_solver_library gives the side library
ACCEPTED = tuple(range(5, 21))    # what the library's entries accept
METHODS = {"euler": 0, "midpoint": 1, "rk4": 2}
HTS = (1, 2, 3, 4)
MAX_HIDDEN = 64
TA, T0 = 12, 6                    # t = arange(T0 - 1, TA): 7 grid points

EDGE_D = (5, 7, 8, 9, 19)
EDGE_H = (1, 16, 17, 43, 64)
EDGE_B = (1, 15, 16, 17, 37)


def ht(H):
    """csrc/real_dims/hode_real_dims.hip hidden_tiles."""
    return (H + 15) // 16


def perturb(method):
    return method != "euler"


def _c(D, H, B, method):
    return dict(D=D, H=H, B=B, method=method, perturb=perturb(method))


#: (D, H, B, method)
CASES = [_c(*row) for row in (
    # one row per (HT, method); the sizes 5 .. 16 along the way
    (5, 1, 17, "euler"), (6, 16, 37, "midpoint"), (7, 16, 15, "rk4"),
    (8, 17, 16, "euler"), (9, 17, 37, "midpoint"), (10, 32, 1, "rk4"),
    (11, 43, 37, "euler"), (12, 43, 33, "midpoint"), (13, 33, 17, "rk4"),
    (14, 64, 15, "euler"), (15, 49, 37, "midpoint"), (16, 64, 16, "rk4"),
    # the remaining sizes, and the edge sizes again with the largest and the smallest blocks around them
    (17, 43, 37, "rk4"), (18, 1, 37, "midpoint"), (19, 64, 37, "rk4"), (19, 43, 1, "midpoint"),
    (5, 64, 37, "rk4"), (7, 43, 37, "midpoint"), (8, 43, 17, "rk4"), (9, 1, 16, "euler"), (19, 17, 15, "euler"),
)]
#: the padding test: sentinels around h, grad_y0 and the flat weight gradient
PADDING_CASES = [_c(5, 43, 17, "midpoint"), _c(19, 43, 1, "midpoint")]
#: size 20 through the side library against libhode.so's default kernel, one per method and hidden-tile count between them
COMPARE_CASES = [_c(20, 43, 37, "midpoint"), _c(20, 16, 17, "euler"), _c(20, 64, 33, "rk4"), _c(20, 17, 16, "rk4")]
#: the model-level test (DDW-shaped inputs: obs 24, statics 11, hidden 43, t0 24, T 40, B 33)
MODEL_DIMS = (7, 12)
MODEL_STEP_DIVS = (1, 2)


def case_id(c):
    return "D%d-H%d-B%d-%s" % (c["D"], c["H"], c["B"], c["method"])


def kernels(c):
    """Forward + backward of one call."""
    args = "%d, %d" % (ht(c["H"]), METHODS[c["method"]])
    return ["hode::real_dims_kernel<%s, false>" % args, "hode::real_dims_kernel<%s, true>" % args,
            "hode::real_dims_fold_kernel<%d>" % ht(c["H"]), "hode::fold_partials_kernel"]


def expected_kernels():
    """Every kernel symbol of the library: HT x method x forward / backward, a fold per HT, the scalars' fold."""
    out = {"hode::fold_partials_kernel"}
    for n in HTS:
        out.add("hode::real_dims_fold_kernel<%d>" % n)
        out |= {"hode::real_dims_kernel<%d, %d, %s>" % (n, m, b) for m in METHODS.values() for b in ("false", "true")}
    return out


def kernels_reached(cases=None):
    return {k for c in (CASES if cases is None else cases) for k in kernels(c)}


def wflat_len(D, H):
    return 9 * H + 2 + 3 * (D - 4) ** 2
