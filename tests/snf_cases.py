"""The GPU test table of the Sylvester-flow posterior (tests/test_hip_snf.py), its inputs, and which compiled kernels each
case reaches (kernels()), read by the no-GPU coverage guard in tests/test_snf_host.py.  A plain helper module."""
import torch

TILES = (4, 8, 16, 32)
DS = (1, 3, 4, 5, 8, 9, 16, 17, 32)   # every tile edge
KS, SS, BS, HS = (1, 2, 3, 16), (1, 3, 64, 65, 256), (1, 2, 7, 65), (1, 2, 8)
BIG_B, BIG_SUBSET = 4099, 192
#: cases that cannot hold FLOW_TOL / FLOW_GTOL get a bound of their own here: case_id -> (tol, gtol), four times the error
#: of the float32 eager path against float64 on the same inputs.  None so far.
OWN_BOUNDS = {}


def tile(D):
    return next(t for t in TILES if D <= t)


def _case(mode, D, K, S, B, H=0, s_kl=1):
    assert (mode == "tri") == (H == 0)
    return {"mode": mode, "D": D, "K": K, "S": S, "B": B, "H": H, "s_kl": min(s_kl, S - 1)}


def _grid():
    """A covering subset of the product: every D once per type, with K, S, B, H and s_kl walking their lists at different
    strides so that every value of each occurs in both types; then the pairs the walk does not guarantee -- the largest
    tile with more draws than lanes and 16 flows in both types, a ragged last workgroup with S just past a lane group,
    the flow script's shape -- and the B = 4 099 case."""
    cases, i = [], 0
    for mode in ("tri", "hh"):
        for D in DS:
            H = HS[i % 3] if mode == "hh" else 0
            cases.append(_case(mode, D, KS[i % 4], SS[(2 * i + 1) % 5], BS[(3 * i + 2) % 4], H, i % 2))
            i += 1
        i += 1   # shift the second type's walk against the first
    cases.append(_case("hh", 32, 16, 256, 2, 8))      # flows streamed through LDS, four rounds of 64 lanes, eight reflections
    cases.append(_case("tri", 32, 16, 256, 2))
    cases.append(_case("hh", 6, 4, 65, 7, 6, 0))      # S one past the lane group, 7 patients in workgroups of 4
    cases.append(_case("tri", 6, 4, 51, 10))          # the flow script's shape
    cases.append(_case("hh", 6, 4, 51, 10, 6))
    cases.append(_case("tri", 12, 3, 51, 65))
    cases.append(_case("hh", 12, 4, 51, BIG_B, 2))
    return cases


CASES = _grid()


def case_id(c):
    return "%s_D%d_K%d_S%d_B%d_H%d_kl%d" % (c["mode"], c["D"], c["K"], c["S"], c["B"], c["H"], c["s_kl"])


def kernels(c):
    t = tile(c["D"])
    return {"hode_snf::snf_fwd_kernel<%d>" % t, "hode_snf::snf_bwd_kernel<%d>" % t}


HEADS = ("mu", "log_var", "full_d", "diag1", "diag2", "bias", "v")


def inputs(c, seed=None):
    """The raw heads, the noise and the two cotangents of a case, float32 on the CPU.  full_d is dense (the kernels must
    apply the masks themselves); the raw diagonals lie in [-1.7, 1.7], so |r1_mm r2_mm| <= tanh(1.7)^2 < 0.88 and the
    log's argument stays above 0.12."""
    D, K, S, B, H = c["D"], c["K"], c["S"], c["B"], c["H"]
    g = torch.Generator().manual_seed(seed if seed is not None else 11 + 1000 * D + 100 * H + 10 * K + S + B)
    r = lambda *shape: torch.randn(*shape, generator=g)   # noqa: E731
    ins = {"mu": 0.5 * r(B, D), "log_var": -1.0 + 0.5 * r(B, D), "full_d": 0.5 * r(B, K, D, D) / D ** 0.5,
           "diag1": (torch.rand(B, K, D, generator=g) * 2 - 1) * 1.7, "diag2": (torch.rand(B, K, D, generator=g) * 2 - 1) * 1.7,
           "bias": 0.3 * r(B, K, D), "v": r(B, K, H, D) if H else None,
           "noise": r(S, B, D), "gz": r(S, B, D), "gk": r(B)}
    ins["s_kl"] = c["s_kl"]
    return ins


def subset(B):
    """Patients of a large batch the float64 yardstick runs on: the first, the last and random ones (each patient's sums are
    its own)."""
    if B < BIG_B:
        return None
    g = torch.Generator().manual_seed(B)
    n = BIG_SUBSET // 3
    return torch.cat([torch.arange(n), torch.randint(0, B, (n,), generator=g), torch.arange(B - n, B)])
