"""The case table of libhode_real_dose.so (tests/test_real_dose_host.py on the CPU, tests/test_hip_real_dose.py on the GPU):
the adjoint of the real-data hybrid solve that also returns d loss / d act of the dose table act (Ta, B).  Restates,
independently of the library, which kernels a call launches: HT = ceil(H / 16) and the method select
real_dose_bwd_kernel<HT, method>, followed by real_dose_fold_kernel<HT> (the flat weight gradient) and fold_partials_kernel
(the three scalars).  The latent size is a runtime argument: it selects no kernel.

Time axis of the `unit` cases: that of tests/real_dims_cases.py -- Ta = 12 action rows, t = 5, 6, .., 11, perturb for
midpoint / rk4 only -- so that doses fall before the window, inside it, and at hours 11 and 12, at or after the last stage
time, where the gradient is exactly zero.  The other grids are tests/time_grids.py's with its action-row counts REAL_TA:
    ragged   0 .. 1.875, Ta 1    stages with floor(t) = 0 (no dose yet) and with floor(t) = 1 = Ta
    offset+  2.5 .. 4.375, Ta 3  floor(t) = 2, 3 and 4 > Ta: stages past the last action row read the last one
    offset-  -1 .. 0.875, Ta 2   negative stage times; NO stage reaches hour 1, so the oracle's d loss / d act is exactly zero
                                 everywhere and the kernel must write exactly that (the flush alone)
Two cases run sub-stepped (options["step_size"] = 0.5 on the unit axis: stages at the half hours, outputs read off every
second grid point).

Also here: the inputs of a case, its float64 / fp32 oracle with the action a leaf, and a restatement in numpy of what the
kernel adds to the plain backward -- the tap of the stage cotangent and the reverse scan, in the fused form one lane runs --
fed the oracle's own stage cotangents from a restated fixed-grid loop."""
import copy
import functools

import numpy as np
import torch

import real_dims_cases as rd
import time_grids as tg

METHODS = rd.METHODS
HTS = rd.HTS
MIN_LATENT, MAX_LATENT, MAX_HIDDEN = 5, 20, 64
EDGE_D = (5, 7, 8, 9, 19, 20)
EDGE_H = rd.EDGE_H
EDGE_B = rd.EDGE_B
GRIDS = ("unit", "ragged", "offset+", "offset-")
#: family bound of the gradients (tests/test_hip_real.py, tests/test_hip_real_dims.py) and the oracle's own share of it
GRAD_TOL = 1e-4
ORACLE_TOL = GRAD_TOL / 10


def ht(H):
    """csrc/real_dose/hode_real_dose.hip hidden_tiles."""
    return (H + 15) // 16


def _c(D, H, B, method, grid="unit", step_size=None, perturb=None, zero=False):
    return dict(D=D, H=H, B=B, method=method, perturb=rd.perturb(method) if perturb is None else perturb, grid=grid,
                step_size=step_size, zero=zero)


CASES = [_c(*row) for row in (
    # one row per (HT, method); the six cases measured on the oracle before any kernel existed among them
    (5, 1, 17, "euler"), (6, 16, 37, "midpoint"), (7, 16, 15, "rk4"),
    (8, 17, 16, "euler"), (9, 17, 37, "midpoint"), (10, 32, 1, "rk4"),
    (11, 43, 37, "euler"), (12, 43, 33, "midpoint"), (13, 33, 17, "rk4"),
    (14, 64, 15, "euler"), (15, 49, 37, "midpoint"), (19, 64, 37, "rk4"),
    # the edge sizes again: M = 16 through the ragged tile at every method, the smallest blocks, one patient
    (20, 43, 37, "midpoint"), (20, 64, 16, "rk4"), (20, 1, 17, "euler"), (19, 43, 1, "midpoint"), (5, 64, 37, "rk4"), (9, 1, 16, "euler"),
)] + [
    # one case per method on each of the three grids
    _c(7, 16, 17, "euler", "ragged", perturb=False), _c(9, 17, 37, "midpoint", "ragged", perturb=True),
    _c(19, 43, 1, "rk4", "ragged", perturb=False),
    _c(8, 43, 37, "euler", "offset+", perturb=True), _c(5, 64, 17, "midpoint", "offset+", perturb=False),
    _c(20, 17, 16, "rk4", "offset+", perturb=True),
    _c(9, 17, 17, "euler", "offset-", perturb=False), _c(12, 43, 37, "midpoint", "offset-", perturb=True),
    _c(7, 64, 15, "rk4", "offset-", perturb=False),
    # sub-stepped
    _c(12, 43, 33, "midpoint", step_size=0.5), _c(7, 16, 17, "rk4", step_size=0.5),
]
#: the same problem with the column of act of patient ZERO_PATIENT zeroed: the gradient of the table does not depend on the table
ZERO_PATIENT = 16
ZERO_CASES = [_c(9, 17, 37, "midpoint", zero=True), _c(20, 43, 17, "rk4", zero=True)]
#: size 20 is served by libhode.so in the plain solve: the comparison against libhode_real_dims.so's backward stops at 19
PLAIN_DIMS = rd.DIMS
#: the model-level test (DDW-shaped inputs: obs 24, statics 11, hidden 43, t0 24, T 40, B 33)
MODEL_DIMS = (7, 12, 20)
MODEL_STEP_DIVS = (1, 2)


def case_id(c):
    return "D%d-H%d-B%d-%s%s-%s%s%s" % (c["D"], c["H"], c["B"], c["method"], "-perturb" if c["perturb"] else "", c["grid"],
                                        "-step%s" % c["step_size"] if c["step_size"] else "", "-zerocol" if c["zero"] else "")


def kernels(c):
    """The backward of one call (the forward is hode.real.real_solve's: tests/real_dims_cases.py)."""
    n = ht(c["H"])
    return ["hode::real_dose_bwd_kernel<%d, %d>" % (n, METHODS[c["method"]]), "hode::real_dose_fold_kernel<%d>" % n,
            "hode::fold_partials_kernel"]


def expected_kernels():
    """Every kernel symbol of the library: HT x method, a fold per HT, the scalars' fold."""
    out = {"hode::fold_partials_kernel"}
    for n in HTS:
        out.add("hode::real_dose_fold_kernel<%d>" % n)
        out |= {"hode::real_dose_bwd_kernel<%d, %d>" % (n, m) for m in METHODS.values()}
    return out


def kernels_reached(cases=None):
    return {k for c in (CASES + ZERO_CASES if cases is None else cases) for k in kernels(c)}


# -------------------------------------------------------------------------------------------------------------- inputs
def n_action_rows(c):
    return rd.TA if c["grid"] == "unit" else tg.REAL_TA[c["grid"]]


def never_dosed(c):
    """No stage time of the case reaches hour 1: Dose(t) = 0 throughout and d loss / d act is exactly zero everywhere."""
    return c["grid"] == "offset-"


@functools.lru_cache(maxsize=None)
def _inputs(D, H, B, grid, zero):
    """fp32 inputs: on the unit axis those of tests/test_hip_real_dims._inputs; on the other grids the same draw with that
    grid and its number of action rows (doses on 40 % of the few cells there; patient 0 has one in the first row)."""
    from test_hip_real_dims import _flat, _inputs as unit_inputs
    if grid == "unit":
        f, p = unit_inputs(D, H, B)
    else:
        from oracle.rhs import RocheRealRHS
        Ta = tg.REAL_TA[grid]
        gen = torch.Generator().manual_seed(1000 * D + 10 * H + B)
        torch.manual_seed(D + 3 * H)
        f = RocheRealRHS(D, H)
        a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen)
        a[0, 0, 0] = 0.7
        t = tg.grid(grid, tg.REAL_T)
        y0 = torch.randn(B, D, generator=gen) * 0.3
        cot = torch.randn(t.numel(), B, D, generator=gen)
        wflat = torch.cat([q.detach().reshape(-1) for q in _flat(f)])
        theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
        p = dict(y0=y0, a=a, t=t, cot=cot, wflat=wflat, theta=theta)
    if zero:  # a patient who never gets a dose
        p = dict(p, a=p["a"].clone())
        p["a"][:, ZERO_PATIENT, 0] = 0.0
    return f, p


def inputs(c):
    return _inputs(c["D"], c["H"], c["B"], c["grid"], c["zero"])


def _options(c):
    o = {"perturb": c["perturb"]}
    if c["step_size"] is not None:
        o["step_size"] = c["step_size"]
    return o


def _weights(f):
    from test_hip_real_dims import _flat
    return _flat(f)


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _oracle(key, dtype):
    from oracle.solvers import odeint as oracle_odeint
    c = dict(key)
    f, p = inputs(c)
    f = copy.deepcopy(f).to(dtype)
    a = p["a"].detach().clone().to(dtype).requires_grad_(True)
    f.set_action_static(a)
    y = p["y0"].detach().clone().to(dtype).requires_grad_(True)
    h = oracle_odeint(f, y, p["t"].to(dtype), method=c["method"], options=_options(c))
    (h * p["cot"].to(dtype)).sum().backward()
    return dict(h=h.detach(), gact=a.grad[..., 0], gy0=y.grad, gw=torch.cat([q.grad.reshape(-1) for q in _weights(f)]),
                gth=torch.stack([f.k_immunity.grad, f.kel.grad, f.kel2.grad]))


def oracle(c, dtype=torch.float64):
    """h, d loss / d act (Ta, B), grad_y0, the flat weight gradient and the theta gradient of loss = sum(h * cot) from the
    oracle in `dtype`, with the action a leaf; computed once per case and left unchanged."""
    return _oracle(tuple(sorted(c.items(), key=lambda kv: kv[0])), dtype)


# --------------------------------------------------------------------------- the tap and the reverse scan, restated
def stage_cotangents(c):
    """The float64 oracle's fixed-grid loop restated with the gradient of every rhs output retained: returns
    (stages, ref) with stages = [(ts, g3)] in the order the rhs was called -- ts the stage time, g3 (B,) the cotangent of
    KX[3] after backward of sum(h * cot) -- and ref the oracle's own result of the same problem (the loop's h is checked
    against it)."""
    from oracle.solvers import _fixed_grid, _nextafter
    ref = oracle(c)
    f, p = inputs(c)
    f = copy.deepcopy(f).double()
    f.set_action_static(p["a"].double())
    t = p["t"].double()
    grid = _fixed_grid(t, c["step_size"])
    calls = []

    def rhs(ts, y):
        k = f(ts, y)
        k.retain_grad()
        calls.append((float(ts), k))
        return k

    y, out, j = p["y0"].double(), [p["y0"].double()], 1
    third = 1 / 3
    for t0, t1 in zip(grid[:-1], grid[1:]):
        dt = t1 - t0
        first = _nextafter(t0, True) if c["perturb"] else t0
        last = _nextafter(t1, False) if c["perturb"] else t1
        k1 = rhs(first, y)
        if c["method"] == "euler":
            y_next = y + dt * k1
        elif c["method"] == "midpoint":
            y_next = y + dt * rhs(t0 + 0.5 * dt, y + k1 * (0.5 * dt))
        else:
            k2 = rhs(t0 + dt * third, y + dt * k1 * third)
            k3 = rhs(t0 + dt * (2 / 3), y + dt * (k2 - k1 * third))
            k4 = rhs(last, y + dt * (k1 - k2 + k3))
            y_next = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        while j < len(t) and t1 >= t[j]:
            out.append(y if t[j] == t0 else y_next if t[j] == t1 else y + (t[j] - t0) / (t1 - t0) * (y_next - y))
            j += 1
        y = y_next
    h = torch.stack(out, dim=0)
    assert torch.equal(h.detach(), ref["h"]), "the restated loop is not the oracle's"
    (h * p["cot"].double()).sum().backward()
    return [(ts, k.grad[:, 3].numpy().copy()) for ts, k in calls], ref


def tap_and_scan(stages, kel, Ta, B):
    """What one lane of real_dose_bwd_kernel does for its patient, for all patients at once in numpy float64: walk the
    stages from the last to the first with (n_cur, R), write the rows n_cur - 1 .. n out before a tap at n < n_cur, flush
    down to row 0 at the end.  Asserts that the taps' n never increases and that every row is written exactly once."""
    E = np.exp(-kel)
    grad_act = np.full((Ta, B), np.nan)
    written = np.zeros(Ta, dtype=int)
    n_cur, R = Ta, np.zeros(B)

    def flush_to(n):
        nonlocal n_cur, R
        while n_cur > n:
            grad_act[n_cur - 1] = R
            written[n_cur - 1] += 1
            R = R * E
            n_cur -= 1

    for ts, g3 in reversed(stages):
        n = min(Ta, int(np.floor(ts)))
        if n < 1:
            continue
        assert n <= n_cur, "a tap's action row increased along the reverse sweep"
        flush_to(n)
        R = R + g3 * kel * np.exp(kel * (n - ts))
    flush_to(0)
    assert (written == 1).all()
    return grad_act


def wflat_len(D, H):
    return rd.wflat_len(D, H)
