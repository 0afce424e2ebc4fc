"""The case table of libhode_real_pp.so (tests/test_real_pp_host.py on the CPU, tests/test_hip_real_pp.py on the GPU): dopri5
with per-patient step control for the real-data hybrid rhs.  Restates, independently of the library, which kernels a call
launches: HT = ceil(H / 16) selects real_pp_fwd_kernel<HT>; a backward launches real_pp_bwd_kernel<HT>,
real_pp_fold_kernel<HT> (the flat weight gradient) and fold_partials_kernel (the three scalars).  The latent size is a runtime
argument: it selects no kernel.

Shapes, the smallest that can still go wrong: B 1, 15, 16, 17, 33 (a partial, an exact and a spilled tile of 16 patients);
D 5, 12, 20 (M = 1, 8, 16 GRU rows of the 16-row tile); H 1, 16, 17, 43, 64 (every hidden-tile count, both tile edges); T 2,
3, 8 on each of the grids
    uniform  3, 4, 5, ..      DecoderReal's: integer hours, every output time a dose switch
    ragged   0 .. 1.1         tests/time_grids.py: neighbouring intervals a factor >= 4 apart, crossing hour 1 inside a step
    offset+  2.5 .. 3.6       non-integer nodes, doses before the window already decaying
    offset-  -1 .. 0.1        negative stage times (no dose yet)
    late     3 - 1/32, 4, 5, ..  the `stiff` cases': a dose switch 1/32 hour after t[0]
with Ta = the last hour + 1 action rows.  Patient 0 has a dose in the first and in the last hour, patient ZERO_PATIENT (when
B > 1) none at all, hour ZERO_HOUR nobody (when Ta > 2).  Tolerances rtol 1e-5 / atol 1e-7, one case at DecoderReal's 1e-7 /
1e-8.  The `stiff` cases scale the start state of patient STIFF of the tile by STIFF_SCALE, picked on the CPU from the float64
eager controller's own counts (tests/real_pp_eager.py): that patient then takes a different number of steps than its
tile-mates and has rejections they do not have.  Unlike the synthetic Roche rhs this one is bounded (tanh / sigmoid
everywhere), and Hairer's rule is conservative on it: over scales 0.01 .. 1e5 the first attempt's ratio stayed below 1e-5,
so no scale makes a FIRST attempt fail.  The stiff cases therefore run on the `late` grid, whose t[0] lies 1/32 hour before
the dose switch of hour 3, and give patient STIFF a dose of LATE_DOSE there: Hairer's second evaluation at t0 + h0 lies
before the switch, the first attempt crosses it, and is rejected -- in every stiff case for some patients of STIFF's tile and
not for others, in two of them for patient STIFF itself.  tests/test_real_pp_host.py holds every case to these promises."""
import copy
import functools

import numpy as np
import torch

import real_pp_eager as eager
import time_grids as tg

HTS = (1, 2, 3, 4)
MIN_LATENT, MAX_LATENT, MAX_HIDDEN = 5, 20, 64
EDGE_B = (1, 15, 16, 17, 33)
EDGE_D = (5, 12, 20)
EDGE_H = (1, 16, 17, 43, 64)
EDGE_T = (2, 3, 8)
GRIDS = ("uniform", "ragged", "offset+", "offset-", "late")
LATE_START, LATE_DOSE_ROW, LATE_DOSE = 3.0 - 1.0 / 32.0, 2, 30.0
TOL = (1e-5, 1e-7)
DECODER_TOL = (1e-7, 1e-8)
UNIFORM_START = 3.0
ZERO_PATIENT, ZERO_HOUR = 1, 1
STIFF = 3  # this patient's start state is scaled up (cases with `stiff`)
STIFF_SCALE = 40.0
#: the GRU and MLP weights are drawn larger than nn.Linear's default, so that a step of an hour is not accepted at once
WEIGHT_GAIN = 3.0


def ht(H):
    """csrc/hode_real_side_host.hpp real_side_hidden_tiles."""
    return (H + 15) // 16


def _c(D, H, B, T, grid, tol=TOL, stiff=False):
    return dict(D=D, H=H, B=B, T=T, grid=grid, rtol=tol[0], atol=tol[1], stiff=stiff)


CASES = [_c(*row) for row in (
    # T x grid, the sizes a Latin square over the edges
    (5, 1, 1, 2, "uniform"), (12, 16, 15, 3, "uniform"), (20, 17, 16, 8, "uniform"),
    (12, 43, 17, 2, "ragged"), (20, 64, 33, 3, "ragged"), (5, 17, 15, 8, "ragged"),
    (20, 16, 33, 2, "offset+"), (5, 64, 17, 3, "offset+"), (12, 1, 16, 8, "offset+"),
    (12, 43, 1, 8, "offset-"),
)] + [
    # one patient of a tile with a scaled-up start state, at every hidden-tile count
    _c(12, 16, 17, 8, "late", stiff=True), _c(20, 17, 15, 3, "late", stiff=True),
    _c(5, 43, 33, 8, "late", stiff=True), _c(20, 64, 16, 8, "late", stiff=True),
    # the decoder's own tolerances
    _c(20, 43, 17, 8, "uniform", tol=DECODER_TOL),
]


def case_id(c):
    return "D%d-H%d-B%d-T%d-%s-rtol%g%s" % (c["D"], c["H"], c["B"], c["T"], c["grid"], c["rtol"], "-stiff" if c["stiff"] else "")


def kernels(c, backward=True):
    n = ht(c["H"])
    out = ["hode::real_pp_fwd_kernel<%d>" % n]
    if backward:
        out += ["hode::real_pp_bwd_kernel<%d>" % n, "hode::real_pp_fold_kernel<%d>" % n, "hode::fold_partials_kernel"]
    return out


def expected_kernels():
    """Every kernel symbol of the library: a forward, a sweep and a fold per HT, the scalars' fold."""
    out = {"hode::fold_partials_kernel"}
    for n in HTS:
        out |= {"hode::real_pp_fwd_kernel<%d>" % n, "hode::real_pp_bwd_kernel<%d>" % n, "hode::real_pp_fold_kernel<%d>" % n}
    return out


def kernels_reached(cases=None):
    return {k for c in (CASES if cases is None else cases) for k in kernels(c)}


def wflat_len(D, H):
    return 9 * H + 2 + 3 * (D - 4) ** 2


# -------------------------------------------------------------------------------------------------------------- inputs
def grid(c):
    if c["grid"] == "uniform":
        return torch.arange(c["T"], dtype=torch.float32) + UNIFORM_START
    if c["grid"] == "late":
        t = torch.arange(c["T"], dtype=torch.float32) + 3.0
        t[0] = LATE_START
        return t
    return tg.grid(c["grid"], c["T"])


def n_action_rows(c):
    return max(1, int(np.ceil(float(grid(c)[-1])))) + 1


def flat(f):
    ps = [f.dx1_net[0].weight, f.dx1_net[0].bias, f.dx1_net[2].weight, f.dx1_net[2].bias,
          f.dx2_net[0].weight, f.dx2_net[0].bias, f.dx2_net[2].weight, f.dx2_net[2].bias]
    return ps + [f.lin_hh.weight, f.lin_hz.weight, f.lin_hr.weight]


@functools.lru_cache(maxsize=None)
def _inputs(D, H, B, T, grid_name, stiff):
    from oracle.rhs import RocheRealRHS
    c = dict(T=T, grid=grid_name)
    Ta = n_action_rows(c)
    gen = torch.Generator().manual_seed(1000 * D + 10 * H + B + 7 * T)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    with torch.no_grad():
        for q in flat(f):
            q.mul_(WEIGHT_GAIN)
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen)
    a[0, 0, 0], a[Ta - 1, 0, 0] = 0.7, 0.4
    if B > 1:
        a[:, ZERO_PATIENT] = 0.0
    if Ta > 2:
        a[ZERO_HOUR] = 0.0
    y0 = torch.randn(B, D, generator=gen) * 0.3
    if stiff:
        y0[STIFF] *= STIFF_SCALE
        a[LATE_DOSE_ROW, STIFF, 0] = LATE_DOSE
    t = grid(c)
    cot = torch.randn(T, B, D, generator=gen)
    wflat = torch.cat([q.detach().reshape(-1) for q in flat(f)])
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return f, dict(y0=y0, a=a, t=t, cot=cot, wflat=wflat, theta=theta)


def inputs(c):
    """(the rhs module, fp32 tensors y0 (B, D), a (Ta, B, 1), t (T,), cot (T, B, D), wflat, theta (3,))."""
    return _inputs(c["D"], c["H"], c["B"], c["T"], c["grid"], c["stiff"])


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def patient_rhs(c, p, dtype):
    """A copy of the case's rhs in `dtype` that sees patient p's column of the dose table alone."""
    f, q = inputs(c)
    f = copy.deepcopy(f).to(dtype)
    f.set_action_static(q["a"][:, p:p + 1].to(dtype))
    return f


# ------------------------------------------------------------------------------------------------ eager runs, per case
@functools.lru_cache(maxsize=None)
def _controller(key, dtype):
    c = dict(key)
    _, q = inputs(c)
    return [eager.controller(patient_rhs(c, p, dtype), q["y0"][p:p + 1].to(dtype), q["t"], c["rtol"], c["atol"],
                             max_steps=max_steps(c)) for p in range(c["B"])]


def _key(c):
    return tuple(sorted(c.items(), key=lambda kv: kv[0]))


def controller(c, dtype=torch.float64):
    """The eager controller on every patient of the case at batch one; computed once per (case, dtype) and left unchanged."""
    return _controller(_key(c), dtype)


def max_steps(c):
    """The launch functions' default."""
    return 16 * c["T"] + 64


def replay(c, tapes, dtype=torch.float64):
    """h and the gradients of sum(h * cot) along the given per-patient tapes [(t0, dt_used, j)], one patient at a time with
    the weights shared: dict(h (T, B, D), gy0 (B, D), gw (flat), gth (3,))."""
    f, q = inputs(c)
    f = copy.deepcopy(f).to(dtype)
    y0 = q["y0"].to(dtype).clone().requires_grad_(True)
    hs = []
    for p in range(c["B"]):
        f.set_action_static(q["a"][:, p:p + 1].to(dtype))
        hs.append(eager.replay(f, y0[p:p + 1], q["t"], tapes[p]))
    h = torch.cat(hs, dim=1)
    (h * q["cot"].to(dtype)).sum().backward()
    return dict(h=h.detach(), gy0=y0.grad, gw=torch.cat([w.grad.reshape(-1) for w in flat(f)]),
                gth=torch.stack([f.k_immunity.grad, f.kel.grad, f.kel2.grad]))
