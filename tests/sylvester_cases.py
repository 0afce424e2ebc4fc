"""The GPU test table of the Sylvester flows (tests/test_hip_sylvester.py), its inputs, and which compiled kernels each
case reaches (kernels()), read by the no-GPU coverage guard in tests/test_sylvester_host.py.  A plain helper module."""
import torch

TILES = (4, 8, 16, 32)
DENSE_DM = ((1, 1), (3, 2), (4, 4), (5, 3), (8, 8), (9, 5), (16, 16), (17, 9), (32, 32), (32, 1))
TRI_D = (1, 3, 4, 5, 8, 9, 16, 17, 32)
PERMS = ("none", "flip", "random")
KS, SS, BS = (1, 2, 16), (1, 3, 64, 65, 256), (1, 2, 7, 65)
BIG_B, BIG_SUBSET = 4099, 192


def tile(D, M):
    return next(t for t in TILES if max(D, M) <= t)


def _case(mode, D, M, K, S, B, perm="none"):
    return {"mode": mode, "D": D, "M": M, "K": K, "S": S, "B": B, "perm": perm}


def _grid():
    """A covering subset of the product: every (D, M) of the dense list and every D x perm of the triangular list once, with
    K, S and B walking their lists at different strides so that every value of each occurs in both modes; then the pairs
    the walk does not guarantee -- the largest tile with more draws than lanes and 16 flows, a ragged last workgroup with
    S just past a lane group -- and the B = 4 099 case."""
    cases, i = [], 0
    for D, M in DENSE_DM:
        cases.append(_case("dense", D, M, KS[i % 3], SS[(2 * i + 1) % 5], BS[(3 * i + 2) % 4]))
        i += 1
    for D in TRI_D:
        for perm in PERMS:
            cases.append(_case("tri", D, D, KS[i % 3], SS[(2 * i + 1) % 5], BS[(3 * i + 2) % 4], perm))
            i += 1
    cases.append(_case("dense", 32, 32, 16, 256, 2))      # flows streamed through LDS, four rounds of 64 lanes
    cases.append(_case("dense", 6, 6, 4, 65, 7))          # S one past the lane group, 7 patients in workgroups of 4
    cases.append(_case("tri", 12, 12, 2, 51, 65, "random"))
    cases.append(_case("dense", 12, 12, 4, 51, BIG_B))
    return cases


CASES = _grid()


def case_id(c):
    return "%s_D%d_M%d_K%d_S%d_B%d_%s" % (c["mode"], c["D"], c["M"], c["K"], c["S"], c["B"], c["perm"])


def kernels(c):
    t = tile(c["D"], c["M"])
    return {"hode_sylvester::sylvester_fwd_kernel<%d>" % t, "hode_sylvester::sylvester_bwd_kernel<%d>" % t}


def make_perm(kind, K, D, g):
    if kind == "none":
        return None
    if kind == "flip":
        return torch.arange(D - 1, -1, -1).repeat(K, 1)
    return torch.stack([torch.randperm(D, generator=g) for _ in range(K)])


def inputs(c, seed=None):
    """z0, r1, r2, b, q, perm and the three cotangents of a case, float32 on the CPU.  r1 and r2 are upper triangular plus a
    small dense perturbation (the kernels must not assume triangularity) with their diagonals set afterwards so that
    |r1_mm r2_mm| <= 0.94^2 < 0.9: the log's argument stays above 0.1.  q has orthonormal columns (M <= D) plus a
    perturbation."""
    D, M, K, S, B = c["D"], c["M"], c["K"], c["S"], c["B"]
    g = torch.Generator().manual_seed(seed if seed is not None else 7 + 1000 * D + 100 * M + 10 * K + S + B)

    def tri():
        r = torch.triu(torch.randn(B, K, M, M, generator=g), diagonal=1) / max(M, 1) ** 0.5 + 0.02 * torch.randn(B, K, M, M, generator=g)
        diag = (torch.rand(B, K, M, generator=g) * 2 - 1) * 0.94
        return r - torch.diag_embed(torch.diagonal(r, dim1=-2, dim2=-1)) + torch.diag_embed(diag)

    z0 = torch.randn(S, B, D, generator=g)
    r1, r2 = tri(), tri()
    b = 0.3 * torch.randn(B, K, M, generator=g)
    q = None
    if c["mode"] == "dense":
        raw = torch.randn(B, K, D, M, generator=g)
        q = ((torch.linalg.qr(raw)[0] if M <= D else raw / D ** 0.5) + 0.02 * torch.randn(B, K, D, M, generator=g)).contiguous()
    perm = make_perm(c["perm"], K, D, g)
    gz = torch.randn(S, B, D, generator=g)
    gl = torch.randn(S, B, generator=g)
    gd = torch.randn(S, B, K, M, generator=g)
    return {"z0": z0, "r1": r1, "r2": r2, "b": b, "q": q, "perm": perm, "gz": gz, "gl": gl, "gd": gd}


def subset(B):
    """Patients of a large batch the float64 yardstick runs on: the first, the last and random ones (each patient's sums are
    its own)."""
    if B < BIG_B:
        return None
    g = torch.Generator().manual_seed(B)
    n = BIG_SUBSET // 3
    return torch.cat([torch.arange(n), torch.randint(0, B, (n,), generator=g), torch.arange(B - n, B)])
