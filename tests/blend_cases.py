"""The blend kernels (libhode_blend.so): the GPU test tables (NNLS_CASES, HORIZON_CASES; CASES is both), which compiled
kernel each case reaches (kernels(), read by the no-GPU coverage guard in tests/test_blend_host.py) and seeded inputs.
The float64 yardsticks are in tests/blend_eager.py.  A plain helper module."""
import collections

import torch

NnlsCase = collections.namedtuple("NnlsCase", "Tn B obs problem")
HorizonCase = collections.namedtuple("HorizonCase", "Tn B obs horizons weights")

WAVE_ROWS = 256                       # csrc/blend/hode_blend.hip: kWaveRows, the threshold between the two fit kernels
REAL_HORIZONS = (6, 12, 24, 72)
# rows per step: 1, 15, 64 (one pass of a wave), 65, 256 / 257 (either side of the kernels' threshold), 259, 24 000 (the
# scripts' validation fold: 1 000 x 24)
NNLS_SHAPES = ((1, 1), (3, 5), (2, 32), (5, 13), (2, 128), (257, 1), (7, 37), (1000, 24))
# b = 0.7 x_e + 0.4 x_m + noise / x_e - 0.8 x_m / -0.8 x_e + x_m / -x_e - x_m: the four active sets by construction; an
# all-zero second column; a near-collinear pair x_m = x_e + 1e-3 noise; exactly collinear pairs: x_m = 2 x_e (the three
# products that make the determinant round alike: it is 0) and x_m = 3 x_e with x_e cut to 22 bits, so that 3 x_e is exact (the sums round
# apart: the determinant is a residue of rounding of either sign)
PROBLEMS = ("both", "expert", "ml", "none", "zero_col", "near_collinear")
RANK_DEFICIENT = ("collinear", "collinear3")
WEIGHT_FORMS = ("single", "numbers", "t1o", "to")   # absent / absent; (0.1, 1); (T', 1, obs) tables; (T', obs) tables


def rank_deficient(c):
    """det <= 0 by construction: no unique minimiser, the contract is a finite non-negative minimiser of the objective."""
    return c.B * c.obs == 1 or c.problem in RANK_DEFICIENT


def _nnls_table():
    cases = [NnlsCase(5, B, obs, p) for B, obs in NNLS_SHAPES for p in PROBLEMS + RANK_DEFICIENT]
    cases += [NnlsCase(Tn, B, obs, "both") for Tn in (1, 73) for B, obs in NNLS_SHAPES]
    cases += [NnlsCase(73, 1000, 24, p) for p in PROBLEMS[1:]]
    cases += [NnlsCase(6, 40, 3, "mixed")]   # every step another active set
    cases += [NnlsCase(73, B, obs, "collinear3") for B, obs in ((3, 5), (7, 37))]   # many signs of the residue
    return cases


def _horizon_table():
    cases = [HorizonCase(73, B, obs, REAL_HORIZONS, w) for B in (1, 3, 65, 130) for obs in (1, 24, 37, 128) for w in WEIGHT_FORMS]
    for B, obs in ((3, 24), (65, 1), (130, 37)):
        for w in WEIGHT_FORMS:
            cases.append(HorizonCase(10, B, obs, REAL_HORIZONS, w))          # clipped to (6, 10, 10, 10)
        cases.append(HorizonCase(73, B, obs, (24,), "t1o"))                    # H = 1
        cases.append(HorizonCase(73, B, obs, (1, 2, 3, 5, 8, 8, 21, 100), "to"))  # H = 8, a repeated and a clipped end
    return cases


NNLS_CASES = _nnls_table()
HORIZON_CASES = _horizon_table()
CASES = NNLS_CASES + HORIZON_CASES


def case_id(c):
    if isinstance(c, NnlsCase):
        return "nnls_T%d_B%d_obs%d_%s" % c
    return "hz_T%d_B%d_obs%d_H%d_%d_%s" % (c.Tn, c.B, c.obs, len(c.horizons), c.horizons[-1], c.weights)


def kernels(c):
    if isinstance(c, NnlsCase):
        return {"hode_blend::nnls2_wave_kernel" if c.B * c.obs <= WAVE_ROWS else "hode_blend::nnls2_block_kernel"}
    return {"hode_blend::horizon_sse_kernel"}


def nnls_inputs(c, seed):
    """CPU float32 (x_e, x_m, truth), each (Tn, B, obs)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(c.Tn, c.B, c.obs, generator=g)
    x_e, x_m, noise = r(), r(), 0.1 * r()
    if c.problem == "zero_col":
        x_m = torch.zeros_like(x_e)
    elif c.problem == "near_collinear":
        x_m = x_e + 1e-3 * r()
    elif c.problem == "collinear":
        x_m = 2.0 * x_e
    elif c.problem == "collinear3":
        x_e = (x_e.view(torch.int32) & ~3).view(torch.float32)   # 22 significant bits: 3 x_e is exact
        x_m = 3.0 * x_e
    mix = {"both": (0.7, 0.4), "expert": (1.0, -0.8), "ml": (-0.8, 1.0), "none": (-1.0, -1.0)}
    if c.problem == "mixed":
        coef = torch.tensor([mix[k] for k in ("both", "expert", "ml", "none", "both", "ml")])[:c.Tn]
        truth = coef[:, 0, None, None] * x_e + coef[:, 1, None, None] * x_m + noise
    elif c.problem in ("expert", "ml", "none"):
        truth = mix[c.problem][0] * x_e + mix[c.problem][1] * x_m
    else:
        truth = 0.7 * x_e + 0.4 * x_m + noise
    return x_e, x_m, truth


def horizon_inputs(c, seed):
    """CPU float32 tensors of a case: dict with x_e, x_m, truth, mask (Tn, B, obs) and weight_e, weight_m in the case's
    form; x_m is None for the single-model form.  Patient 1 (when there is one) is fully unobserved."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    i = {"x_e": r(c.Tn, c.B, c.obs), "x_m": r(c.Tn, c.B, c.obs), "truth": r(c.Tn, c.B, c.obs),
         "mask": (torch.rand(c.Tn, c.B, c.obs, generator=g) < 0.6).float(), "weight_e": None, "weight_m": None}
    if c.B > 1:
        i["mask"][:, 1] = 0.0
    if c.weights == "single":
        i["x_m"] = None
    elif c.weights == "numbers":
        i["weight_e"], i["weight_m"] = 0.1, 1
    elif c.weights == "t1o":
        w = 1.2 * torch.rand(2, c.Tn, 1, 1, generator=g)
        i["weight_e"], i["weight_m"] = w[0].expand(c.Tn, 1, c.obs).contiguous(), w[1].expand(c.Tn, 1, c.obs).contiguous()
    else:
        i["weight_e"], i["weight_m"] = 1.2 * torch.rand(c.Tn, c.obs, generator=g), 1.2 * torch.rand(c.Tn, c.obs, generator=g)
    return i
