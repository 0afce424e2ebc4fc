"""Non-uniform and offset time grids for every solver kernel that takes a grid: the grids, the dose placements, the table
of calls (CASES) and their float64 problems.  A plain helper module, not a conftest.

* tests/test_time_grid_cases.py (CPU) checks the grids' invariants, that every fp32 stage time of the kernels falls on the
  same side of every dose time (the same action row) as the fp64 oracle's, that the inputs tell a neighbour's step size
  from the right one, the fp32 oracle's distance from fp64, and the table's reach through tests/kernel_variants.py.
* tests/test_hip_time_grids.py (GPU) runs every CASES entry against the fp64 oracle.

Every other GPU test feeds the kernels a uniform grid that starts at 0 or at an integer: there dt is one number, and a
kernel that took the step size or a stage time of step n +- 1 instead of step n would still be right.

The families real_dims, real_step, neural_odd and neural_odd_dopri5 (SIDE_CASES) put the ragged-size side libraries
libhode_real_dims.so, libhode_real_step.so and libhode_neural_odd.so on the same grids; the one-step-ahead solve also gets
sub2 and sub3, whose intervals take two / three solver steps with a clipped last one of another length in every interval.

All nodes are multiples of 1/64 (1/256 on the clustered grid), so t[n], dt and dt / 2 are exact in fp32 and in fp64."""
import copy
import functools

import numpy as np
import torch

import kernel_variants as kv

# ------------------------------------------------------------------------------------------------------------- grids
# steps in units of 1/64: any four consecutive ones pairwise different, neighbours a factor >= 4 apart, 1 .. 24
RAGGED_STEPS = (8, 1, 24, 4, 16, 2, 12, 3, 20, 5, 24, 1, 9, 2)
GRID_START = {"ragged": 0.0, "offset+": 2.5, "offset-": -1.0}
# dopri5 only, units of 1/256: a run of eight nodes 1/256 apart (one accepted step covers several output times), then a
# gap of more than 1.0 (many accepted steps cover none)
CLUSTERED_256 = (0, 48, 104, 105, 106, 107, 108, 109, 110, 111, 432, 480)
MAX_T = len(RAGGED_STEPS) + 1


def grid64(name, T):
    """The first T nodes of a grid as float64 (exactly representable in fp32 too)."""
    if name == "clustered":
        assert T == len(CLUSTERED_256)
        return np.asarray(CLUSTERED_256, dtype=np.float64) / 256.0
    if name == "uniform":  # today's grid of the synthetic problems, for comparison only
        return np.arange(T, dtype=np.float64) * 0.125
    assert 1 <= T <= MAX_T, T
    units = np.concatenate([[0], np.cumsum(RAGGED_STEPS[:T - 1])])
    return GRID_START[name] + units / 64.0


def grid(name, T):
    return torch.tensor(grid64(name, T), dtype=torch.float32)


def rotated(t):
    """The same t[0] and span with the step sizes rotated by one position (every step gets its neighbour's dt)."""
    t = np.asarray(t, dtype=np.float64)
    return np.concatenate([[t[0]], t[0] + np.cumsum(np.roll(np.diff(t), 1))])


def uniform_like(t):
    t = np.asarray(t, dtype=np.float64)
    return np.linspace(t[0], t[-1], len(t))


# ------------------------------------------------------------------------------------------------------ stage times
F32_THIRD, F32_TWO_THIRDS = np.float32(1.0 / 3.0), np.float32(2.0 / 3.0)


def stage_times32(t, method, perturb):
    """(T-1, stages) fp32 times of every rhs call as the kernels form them (StageTimes, SpTimes, NStageTimes, RStageTimes:
    t0 + dt * (float)(1 / 3) with separately rounded mul and add, nextafter on the first / last stage with perturb)."""
    t = np.asarray(t, dtype=np.float32)
    t0, t1 = t[:-1], t[1:]
    dt = (t1 - t0).astype(np.float32)
    first = np.nextafter(t0, np.float32(np.inf)) if perturb else t0
    last = np.nextafter(t1, np.float32(-np.inf)) if perturb else t1
    if method == "euler":
        cols = [first]
    elif method == "midpoint":
        cols = [first, (t0 + (np.float32(0.5) * dt).astype(np.float32)).astype(np.float32)]
    else:
        cols = [first, (t0 + (dt * F32_THIRD).astype(np.float32)).astype(np.float32),
                (t0 + (dt * F32_TWO_THIRDS).astype(np.float32)).astype(np.float32), last]
    out = np.stack(cols, axis=1)
    assert out.dtype == np.float32
    return out


def stage_times64(t, method, perturb):
    """The same times as the fp64 oracle forms them (oracle.solvers: t0 + dt * (1 / 3) in double, nextafter in double)."""
    t = np.asarray(t, dtype=np.float64)
    t0, t1 = t[:-1], t[1:]
    dt = t1 - t0
    first = np.nextafter(t0, np.inf) if perturb else t0
    last = np.nextafter(t1, -np.inf) if perturb else t1
    if method == "euler":
        cols = [first]
    elif method == "midpoint":
        cols = [first, t0 + 0.5 * dt]
    else:
        cols = [first, t0 + dt * (1 / 3), t0 + dt * (2 / 3), last]
    return np.stack(cols, axis=1)


# --------------------------------------------------------------------------------------------------------- dose times
BEFORE = 0.375  # offset grids: a dose this long before t[0], already decaying when the solve starts


def dose_slots(t, grid_name, inside):
    """Candidate dose times of a grid: every node but the last (t[0] and the last-but-one included), for the offset grids
    a time before t[0], and with `inside` (Roche only: the NeuralODE impulse needs an exact hit) t[n] + dt / 4 of every step."""
    t = np.asarray(t, dtype=np.float64)
    slots = []
    for n in range(len(t) - 1):
        slots.append(t[n])
        if inside:
            slots.append(t[n] + (t[n + 1] - t[n]) / 4)
    if grid_name.startswith("offset"):
        slots.append(t[0] - BEFORE)
    return np.asarray(slots)


def dose_times(t, grid_name, B, K, inside):
    """(B, K) fp32 dose times: patient p takes slots p, p + 5, p + 10 (mod the number of slots), so a batch of more than
    the number of slots puts a dose on every slot; with fewer slots than K a patient takes one twice (the dose counts twice)."""
    slots = dose_slots(t, grid_name, inside)
    idx = (np.arange(B)[:, None] + 5 * np.arange(K)[None, :]) % len(slots)
    out = slots[idx].reshape(B, K)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return torch.tensor(out, dtype=torch.float32)


def outputs_per_step(tape, t):
    """Output times t[j], j >= 1, each accepted step (t_n, t_n + dt_n] of a dopri5 tape of (t_n, dt_n) pairs covers."""
    t = np.asarray(t, dtype=np.float64)[1:]
    return [int(((t > tn) & (t <= tn + dtn)).sum()) for tn, dtn in tape]


# ---------------------------------------------------------------------------------------------------------- the table
SPLIT_TS = (2, 3, 4, 5, 6, 7, 9)  # every residue mod 2 and mod 3 (the unrolled tails), T = 2 and 3 (the prologue's special cases)
ROCHE_LAYOUTS = (  # (lanes, the dimensions the layout serves, kv.roche_layout's name)
    (1, (4, 6), "lane"), (4, (12, 20, 8), "lane"), (48, (8, 12), "split"), (0, (12, 8), "split"), (16, (16, 8, 12), "mf"))


def _roche_cases():
    out, i = [], 0

    def add(lanes, D, method, grid_name, T, tape=None, perturb=None):
        nonlocal i
        out.append(dict(family="roche", D=D, lanes=lanes, method=method, ablate=i % 4 == 3, need_theta=i % 2 == 0,
                        tape=bool((i // 2) % 2) if tape is None else tape,
                        perturb=bool((i // 3) % 2) if perturb is None else perturb,
                        n_dose=(1, 3)[(i // 2) % 2] if tape is None else (1, 3)[i % 2], grid=grid_name, T=T))
        i += 1

    # every layout x method x perturb on the ragged grid at an odd and an even T
    for lanes, dims, _ in ROCHE_LAYOUTS:
        for method in kv.METHODS:
            for perturb in (False, True):
                for T in (5, 8):
                    add(lanes, dims[i % len(dims)], method, "ragged", T, perturb=perturb)
    # every layout x method on both offset grids
    for lanes, dims, _ in ROCHE_LAYOUTS:
        for method in kv.METHODS:
            for g in ("offset+", "offset-"):
                add(lanes, dims[i % len(dims)], method, g, (7, 6, 9)[i % 3])
    # the split layout at every T of SPLIT_TS x method, with the tape and without it
    for T in SPLIT_TS:
        for method in kv.METHODS:
            for tape in (True, False):
                lanes, dims, _ = ROCHE_LAYOUTS[2 + i % 2]
                add(lanes, dims[(i // 2) % 2], method, "ragged", T, tape=tape)
    return out


def _neural_cases():
    out, i = [], 0
    ts = ((8, 5, 2, 8), (5, 8, 8, 2), (8, 2, 5, 5))  # T of the four (perturb, grid) calls: every one has a ragged T = 8
    for layout, onchip, dims in (("mf", True, kv.NEURAL_DIMS), ("mf", False, kv.NEURAL_DIMS), ("lane", False, kv.NEURAL_LANE_DIMS)):
        for method in kv.METHODS:
            for perturb in (False, True):
                for g in ("ragged", "offset-"):
                    out.append(dict(family="neural", D=dims[i % len(dims)], method=method, layout=layout, onchip=onchip,
                                    B=(65, 100, 37)[i % 3], T=ts[(i // 4) % 3][i % 4], perturb=perturb,
                                    n_dose=(1, 3)[(i // 2) % 2], grid=g))
                    i += 1
    return out


DOPRI5_T = len(CLUSTERED_256)


def _dopri5_cases():
    out, i = [], 0
    for D, lanes in ((4, 1), (6, 1), (8, 1), (8, 4), (12, 1), (12, 4)):
        for detach in (True, False):
            for g in ("clustered", "offset+"):
                out.append(dict(family="dopri5", D=D, lanes=lanes, ablate=i % 4 == 3, need_theta=i % 2 == 0, detach=detach,
                                theta="default", n_dose=(1, 3, 0)[i % 3], grid=g, T=DOPRI5_T))
                i += 1
    for j, D in enumerate(kv.NEURAL_DOPRI5_DIMS):
        for detach in (True, False):
            g = ("clustered", "offset+")[(j + detach) % 2]
            out.append(dict(family="neural_dopri5", D=D, detach=detach, B=(17, 70, 33)[(j + detach) % 3], grid=g, T=DOPRI5_T))
    return out


REAL_T = 13  # ragged: 0 .. 1.875 across t = 1; offset+: 2.5 .. 4.375 across 3 and 4; offset-: -1 .. 0.875 across 0
REAL_TA = {"ragged": 1, "offset+": 3, "offset-": 2}  # action rows: stages at floor / trunc(t) >= Ta read past the end


def _real_cases():
    out, i = [], 0
    for D, H, onchip in ((20, 17, True), (20, 33, False), (4, 9, True), (20, 65, True)):
        for method in kv.METHODS:
            for g in ("ragged", "offset+"):
                out.append(dict(family="real", D=D, H=H, method=method, onchip=onchip, perturb=bool(i % 2), grid=g, T=REAL_T))
                i += 1
    for kind, dims in (("neural", (14, 16, 30)), ("2nd", (28, 32, 34))):
        for method in kv.METHODS:
            for g in ("ragged", "offset-"):
                # offset-: without perturb, so that the first stage of the first step is t = -1.0 exactly (action row -1)
                out.append(dict(family="neural_real", kind=kind, D=dims[i % 3], H=(16, 17, 43)[i % 3], method=method,
                                B=(37, 100)[i % 2], perturb=bool((i // 2) % 2) and g != "offset-", grid=g, T=REAL_T))
                i += 1
    return out


# ------------------------------------------------------------------------------------- the ragged-size side libraries
# libhode_real_dims.so, libhode_real_step.so and libhode_neural_odd.so are separately compiled instantiations: the families
# above say nothing about them.  The bindings route by latent size, so the same calls reach them.
def _real_dims_cases():
    """real_dims_kernel<HT, method, fwd / bwd>: every (HT, method) pair on the ragged and the offset+ grid, one case per method
    on offset- (negative stage times); sizes from the edges tests/real_dims_cases.py names.  perturb alternates, so rk4 runs
    without it too (the last stage exactly on t1).  The library serves the on-chip backward only (no operand-tape mode:
    csrc/real_dims/hode_real_dims.hip refuses a NULL grad_w1)."""
    out, i = [], 0
    hs = {1: (1, 16), 2: (17, 17), 3: (43, 43), 4: (64, 64)}
    ds, bs = (5, 7, 8, 9, 19), (1, 17, 37)

    def add(ht, method, g):
        nonlocal i
        out.append(dict(family="real_dims", D=ds[i % 5], H=hs[ht][(i // 2) % 2], B=bs[i % 3], method=method,
                        perturb=bool((i // 2 + i) % 2), grid=g, T=REAL_T))
        i += 1

    for ht in (1, 2, 3, 4):
        for method in kv.METHODS:
            add(ht, method, "ragged")
            add(ht, method, "offset+")
    for ht, method in ((2, "euler"), (3, "midpoint"), (4, "rk4")):
        add(ht, method, "offset-")
    return out


# one-step-ahead: N intervals, each solved on its own row of the (N, S + 1) table of hode.real_step.interval_grids
SUB_LENGTHS = {"sub2": (48, 64, 40, 56, 36, 64, 44),   # units of 1/64 with step_size 0.5: two sub-steps, the last one clipped
               "sub3": (36, 48, 40, 44, 48, 34, 47)}   # with step_size 0.25: three sub-steps, the last one clipped
SUB_STEP_SIZE = {"ragged": None, "sub2": 0.5, "sub3": 0.25}
SUB_STEPS = {"ragged": 1, "sub2": 2, "sub3": 3}
STEP_STARTS = (0.0, 2.5, -1.0)
# action rows per (grid, start), so that over its three starts every grid has doses before the window and inside it and a
# stage past the last row (the min(Ta, .) clamp).  ragged spans 1.05 hours: from 0.0 the dose of hour 1 falls inside it, from
# 2.5 both doses lie before it and the stages from t = 3 on read past them.  sub2 / sub3 span 5.5 / 4.6 hours: from 0.0 and
# 2.5 they hold doses and end past the last row.  The grids from -1.0 start with negative stage times (no dose yet).
STEP_TA = {("ragged", 0.0): 1, ("ragged", 2.5): 2, ("ragged", -1.0): 2,
           ("sub2", 0.0): 4, ("sub2", 2.5): 5, ("sub2", -1.0): 3,
           ("sub3", 0.0): 3, ("sub3", 2.5): 5, ("sub3", -1.0): 2}


def step_grid64(grid_name, start, N):
    """The N + 1 nodes of a one-step-ahead grid as float64 (exact in fp32)."""
    steps = RAGGED_STEPS if grid_name == "ragged" else SUB_LENGTHS[grid_name]
    assert 1 <= N <= len(steps)
    return start + np.concatenate([[0], np.cumsum(steps[:N])]) / 64.0


def _real_step_cases():
    """real_step_kernel<HT, method, fwd / bwd>: every (HT, method) pair; every (grid, start) twice; S 1, 2, 3; C 0, 1, 2, 3, N,
    N + 2; N 2 and 7.  The first three ragged rows (starts 0.0, 2.5, -1.0; D 5, 20, 8) are the ones held bit for bit to the
    chained kernels."""
    rows = (  # D, H, B, N, C, method, grid, start
        (5, 1, 17, 7, 0, "euler", "ragged", 0.0), (8, 16, 37, 7, 2, "midpoint", "sub2", 0.0), (19, 16, 1, 2, 1, "rk4", "sub3", 0.0),
        (20, 17, 37, 7, 3, "euler", "sub3", 2.5), (20, 17, 17, 2, 4, "midpoint", "ragged", 2.5), (19, 17, 37, 7, 7, "rk4", "sub2", 2.5),
        (8, 43, 1, 7, 9, "euler", "sub2", -1.0), (19, 43, 17, 7, 1, "midpoint", "sub3", -1.0), (8, 43, 37, 7, 0, "rk4", "ragged", -1.0),
        (20, 64, 37, 2, 2, "euler", "sub3", 0.0), (5, 64, 17, 7, 3, "midpoint", "sub2", 2.5), (19, 49, 1, 7, 0, "rk4", "sub3", -1.0),
        (19, 33, 37, 7, 7, "midpoint", "ragged", 0.0), (20, 1, 17, 7, 1, "rk4", "sub2", 0.0), (8, 16, 17, 7, 2, "rk4", "sub3", 2.5),
        (19, 64, 17, 7, 3, "euler", "ragged", 2.5), (5, 17, 37, 2, 0, "midpoint", "sub2", -1.0), (20, 43, 1, 2, 4, "rk4", "ragged", -1.0))
    return [dict(family="real_step", D=D, H=H, B=B, N=N, S=SUB_STEPS[g], C=C, method=m, perturb=bool(i % 2), grid=g, start=s)
            for i, (D, H, B, N, C, m, g, s) in enumerate(rows)]


NEURAL_ODD_DIMS = (5, 7, 9, 11, 13, 15)  # hode._neural_odd_lib.DIMS


def _neural_odd_cases():
    """neural_mf_fwd_kernel<D, method> and neural_mf_bwd_kernel<D, method, true> at the odd sizes: every D x method on the
    ragged and the offset- grid (the library has the on-chip backward only)."""
    out = []
    for j, D in enumerate(NEURAL_ODD_DIMS):
        for m, method in enumerate(kv.METHODS):
            for k, g in enumerate(("ragged", "offset-")):
                out.append(dict(family="neural_odd", D=D, method=method, B=(17, 37, 65)[(j + k) % 3], T=(8, 5, 2)[(j + m + k) % 3],
                                perturb=bool((j + m + k) % 2), n_dose=(1, 3)[(j + m) % 2], grid=g))
    return out


def _neural_odd_dopri5_cases():
    return [dict(family="neural_odd_dopri5", D=D, detach=detach, B=(17, 37, 33)[(j + detach) % 3],
                 grid=("clustered", "offset+")[(j + detach) % 2], T=DOPRI5_T)
            for j, D in enumerate(NEURAL_ODD_DIMS) for detach in (True, False)]


OLD_CASES = _roche_cases() + _neural_cases() + _dopri5_cases() + _real_cases()
SIDE_CASES = _real_dims_cases() + _real_step_cases() + _neural_odd_cases() + _neural_odd_dopri5_cases()
CASES = OLD_CASES + SIDE_CASES
FIXED_FAMILIES = ("roche", "neural", "real", "neural_real", "real_dims", "real_step", "neural_odd")


def case_id(case):
    return "-".join("%s=%s" % (k, v) for k, v in case.items() if not (k == "theta" and v == "default"))


def family(name):
    return [c for c in CASES if c["family"] == name]


def kernels(case):
    """Kernel names the case launches, through the dispatch rules tests/kernel_variants.py restates."""
    f = case["family"]
    if f == "roche":
        return kv.roche_fixed(case["D"], case["lanes"], kv.METHODS[case["method"]], case["ablate"], case["need_theta"],
                              case["tape"], case["T"], kv.ROCHE_N)
    if f == "neural":
        return kv.neural_fixed(case["D"], kv.METHODS[case["method"]], kv.neural_lanes(case), case["onchip"])
    if f == "dopri5":
        return kv.dopri5_kernels(case["D"], case["lanes"], case["ablate"], case["need_theta"], case["detach"], kv.DOPRI5_N)
    if f == "neural_dopri5":
        return kv.neural_dopri5_kernels(case["D"], case["T"] - 1, case["detach"])
    if f == "real":
        return kv.real_kernels(case["D"], case["H"], kv.METHODS[case["method"]], case["onchip"])
    if f == "neural_real":
        return kv.neural_real_kernels(case["kind"], case["D"], case["H"], kv.METHODS[case["method"]])
    if f == "real_dims":
        import real_dims_cases
        return real_dims_cases.kernels(case)
    if f == "real_step":
        import real_step_cases
        return real_step_cases.kernels(case)
    if f == "neural_odd":
        return kv.neural_fixed(case["D"], kv.METHODS[case["method"]], 0, True)
    if f == "neural_odd_dopri5":
        return kv.neural_dopri5_kernels(case["D"], case["T"] - 1, case["detach"])
    raise ValueError(f)


# families of kv.FAMILIES that take no time grid (the recurrent decoders, the LSTM encoder, the readouts, folds and packs)
NO_GRID_FAMILIES = ("tlstm_fwd_kernel", "tlstm_bwd_kernel", "gruode_fwd_kernel", "gruode_bwd_kernel", "seqdec_fold_kernel",
                    "neural_real_fold_kernel", "real_grad_fold_kernel", "split_fold_kernel", "mf_fold_kernel",
                    "dp_persist_kernel",  # compiled, never launched by the product build (kv.UNREACHABLE)
                    "neural_grad_fold_kernel", "transpose_w2_kernel", "lstm_fwd_kernel", "lstm_bwd_kernel",
                    "lstm_fill_operand_kernel", "lstm_pack_kernel", "lstm_pack_hh_kernel", "readout_sse_kernel",
                    "readout_mf_kernel", "readout_fold_kernel", "readout_mlp_kernel", "readout_mlp_fold_kernel")


# -------------------------------------------------------------------------------------------------------- the problems
def _t(case, t=None):
    return grid(case["grid"], case["T"]) if t is None else torch.tensor(np.asarray(t), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _roche_inputs(D, ablate, n_dose, grid_name, T):
    """Inputs of a fixed-grid Roche problem, shared by every layout and flag: test_hip_kernel_variants' setup (state, dose
    amounts, weights) on the named grid, with the dose times of dose_times()."""
    from oracle.rhs import dose_schedule
    from test_hip_kernel_variants import _roche_setup, _theta_names
    N = kv.ROCHE_N
    t = grid(grid_name, T)
    inp, f = _roche_setup(D, ablate, N, T, seed=300 + D + 7 * ablate + T, n_dose=n_dose, t=t)
    dosage, _ = dose_schedule(inp["actions"], f.step_size)
    # a quarter of synth's dose amounts: the largest step here is three times synth's 0.125, and with the full dose the
    # -Dose2 * ir term drives ir below zero inside a stage, where the log of ir ** HillPatho (grad theta) is NaN in fp64 too
    dosage = dosage * 0.25
    times = dose_times(grid64(grid_name, T), grid_name, N, n_dose, inside=True)
    cot = torch.randn(T, N, D, generator=torch.Generator().manual_seed(D + T))
    theta = torch.stack([getattr(f, n).detach().reshape(()) for n in _theta_names(ablate)])
    w = f.ml_net[0].weight.detach() if D > 4 else None
    b = f.ml_net[0].bias.detach() if D > 4 else None
    return dict(y0=inp["z0"], t=t, dosage=dosage, times=times, theta=theta, w=w, b=b, cot=cot, f=f)


def roche_inputs(case):
    return _roche_inputs(case["D"], case["ablate"], case["n_dose"], case["grid"], case["T"])


def roche_solve_cpu(p, method, perturb, ablate, dtype=torch.float64, t=None):
    """sum(h * cot) and its gradients by oracle.solvers.odeint on oracle.rhs.RocheRHS in `dtype`, on the fp32 inputs; `t`
    replaces the grid (the dose times stay)."""
    from oracle.solvers import odeint as oracle_odeint
    from test_hip_kernel_variants import _theta_names
    f = copy.deepcopy(p["f"]).to(dtype)
    f.dosage, f.times = p["dosage"].to(dtype), p["times"].to(dtype)
    y = p["y0"].detach().to(dtype).clone().requires_grad_(True)
    tt = (p["t"] if t is None else torch.tensor(np.asarray(t))).to(dtype)
    h = oracle_odeint(f, y, tt, method=method, options={"perturb": perturb})
    (h * p["cot"].to(dtype)).sum().backward()
    zero = torch.zeros((), dtype=dtype)
    ref = dict(h=h.detach(), gy0=y.grad,
               gth=torch.stack([getattr(f, n).grad if getattr(f, n).grad is not None else zero for n in _theta_names(ablate)]))
    if f.ml_dim > 0:
        ref["gw"], ref["gb"] = f.ml_net[0].weight.grad, f.ml_net[0].bias.grad
    return ref


@functools.lru_cache(maxsize=None)
def _roche_ref(D, ablate, n_dose, grid_name, T, method, perturb):
    return roche_solve_cpu(_roche_inputs(D, ablate, n_dose, grid_name, T), method, perturb, ablate)


def roche_ref(case):
    return _roche_ref(case["D"], case["ablate"], case["n_dose"], case["grid"], case["T"], case["method"], case["perturb"])


@functools.lru_cache(maxsize=None)
def _neural_inputs(D, B, T, K, grid_name):
    from oracle.rhs import NeuralRHS
    gen = torch.Generator().manual_seed(D * 1000 + B + 7 * T)
    torch.manual_seed(D + B)
    f = NeuralRHS(D, kv.NEURAL_STEP)
    with torch.no_grad():
        f.ml_net[2].weight.mul_(2.0)
    y0 = torch.randn(B, D, generator=gen) * 0.5
    dosage = 0.5 + torch.rand(B, generator=gen) * 2
    cot = torch.randn(T, B, D, generator=gen)
    times = dose_times(grid64(grid_name, T), grid_name, B, K, inside=False)
    return dict(f=f, t=grid(grid_name, T), y0=y0, dosage=dosage, times=times, cot=cot)


def neural_inputs(case):
    return _neural_inputs(case["D"], case["B"], case["T"], case["n_dose"], case["grid"])


def neural_solve_cpu(p, method, perturb, dtype=torch.float64, t=None):
    from oracle.solvers import odeint as oracle_odeint
    f = copy.deepcopy(p["f"]).to(dtype)
    f.dosage, f.times = p["dosage"].to(dtype), p["times"].to(dtype)
    y = p["y0"].detach().to(dtype).clone().requires_grad_(True)
    tt = (p["t"] if t is None else torch.tensor(np.asarray(t))).to(dtype)
    h = oracle_odeint(f, y, tt, method=method, options={"perturb": perturb})
    (h * p["cot"].to(dtype)).sum().backward()
    n = f.ml_net
    g = [q.grad if q.grad is not None else torch.zeros_like(q) for q in (n[0].weight, n[0].bias, n[2].weight, n[2].bias)]
    return dict(h=h.detach(), gy0=y.grad, gw1=g[0], gb1=g[1], gw2=g[2], gb2=g[3])


def real_problem(case):
    """test_hip_kernel_variants._real_problem (inputs and the fp64 oracle on oracle.rhs.RocheRealRHS) on the case's grid."""
    from test_hip_kernel_variants import _real_problem
    t = tuple(float(x) for x in grid64(case["grid"], case["T"]))
    return _real_problem(case["D"], case["H"], case["method"], case["perturb"], B=case.get("B", 37), Ta=REAL_TA[case["grid"]], t=t)


def real_solve_cpu(case, p, dtype=torch.float64, t=None):
    """The same oracle from the flat inputs of real_problem(), in `dtype` and optionally on another grid."""
    from oracle.rhs import RocheRealRHS
    from oracle.solvers import odeint as oracle_odeint
    from test_hip_kernel_variants import _real_flat
    D, H = case["D"], case["H"]
    f = RocheRealRHS(D, H).to(dtype)
    flat, o = _real_flat(f), 0
    with torch.no_grad():
        for q in flat:
            q.copy_(p["wflat"][o:o + q.numel()].reshape(q.shape))
            o += q.numel()
        for q, v in zip((f.k_immunity, f.kel, f.kel2), p["theta"]):
            q.copy_(v)
    assert o == p["wflat"].numel()
    f.set_action_static(p["a"].to(dtype))
    y = p["y0"].detach().to(dtype).clone().requires_grad_(True)
    tt = (p["t"] if t is None else torch.tensor(np.asarray(t))).to(dtype)
    h = oracle_odeint(f, y, tt, method=case["method"], options={"perturb": p["perturb"]})
    (h * p["cot"].to(dtype)).sum().backward()
    return dict(h=h.detach(), gy0=y.grad, gw=torch.cat([q.grad.reshape(-1) for q in flat]),
                gth=torch.stack([f.k_immunity.grad, f.kel.grad, f.kel2.grad]))


def neural_real_inputs(case):
    """The inputs tests/test_hip_kernel_variants._neural_real draws for this case (same generator, same order), for the CPU
    checks: (y0, action, grid, cot, seed)."""
    D, H, B, T = case["D"], case["H"], case["B"], case["T"]
    Ta, seed = REAL_TA[case["grid"]], case["D"] + case["H"]
    gen = torch.Generator().manual_seed(seed)
    y0 = torch.randn(B, D, generator=gen) * 0.5
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen) * 2
    cot = torch.randn(T, B, D, generator=gen)
    return y0, a, grid(case["grid"], T), cot, seed


def neural_real_solve_cpu(case, dtype=torch.float64, t=None):
    """tests/neural_real_eager.py on CPU weights drawn like model.NeuralODEReal*'s ml_net (for the CPU checks only: the GPU
    test takes the module's own weights), in `dtype`; returns the result and the action rows the rhs read."""
    import warnings

    import neural_real_eager
    y0, a, tg, cot, seed = neural_real_inputs(case)
    D, H = case["D"], case["H"]
    torch.manual_seed(seed)
    out = D if case["kind"] == "neural" else D // 2
    net = torch.nn.Sequential(torch.nn.Linear(D + 1, H), torch.nn.Tanh(), torch.nn.Linear(H, out), torch.nn.Tanh())
    ps = [q.detach().to(dtype).requires_grad_(True) for q in net.parameters()]
    y = y0.to(dtype).clone().requires_grad_(True)
    tt = (tg if t is None else torch.tensor(np.asarray(t))).to(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h, rows = neural_real_eager.solve(case["kind"], y, *ps, a.to(dtype), tt, case["method"], perturb=case["perturb"])
    (h * cot.to(dtype)).sum().backward()
    return dict(h=h.detach(), gy0=y.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad, gb2=ps[3].grad), rows


# ------------------------------------------------------------------------------------------- one-step-ahead (real_step)
@functools.lru_cache(maxsize=None)
def _real_step_inputs(D, H, B, N, grid_name, start):
    """fp32 inputs of a one-step-ahead problem as tests/test_hip_real_step.py draws them, on the named grid: the rhs module,
    doses on half of the (hour, patient) cells (patient 0 has the first and the last row whatever the draw), a start state
    per interval and the cotangent of h."""
    from oracle.rhs import RocheRealRHS
    from test_hip_kernel_variants import _real_flat
    Ta = STEP_TA[(grid_name, start)]
    gen = torch.Generator().manual_seed(1000 * D + 10 * H + B + 7 * N)
    torch.manual_seed(D + 3 * H)
    f = RocheRealRHS(D, H)
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.5).float() * torch.rand(Ta, B, 1, generator=gen) * 2
    a[0, 0, 0], a[Ta - 1, 0, 0] = 0.7, 0.4
    t = torch.tensor(step_grid64(grid_name, start, N), dtype=torch.float32)
    init = torch.randn(N, B, D, generator=gen) * 0.3
    cot = torch.randn(N + 1, B, D, generator=gen)
    wflat = torch.cat([q.detach().reshape(-1) for q in _real_flat(f)])
    theta = torch.stack([f.k_immunity, f.kel, f.kel2]).detach()
    return dict(f=f, init=init, a=a, t=t, cot=cot, wflat=wflat, theta=theta, Ta=Ta, step_size=SUB_STEP_SIZE[grid_name])


def real_step_inputs(case):
    return _real_step_inputs(case["D"], case["H"], case["B"], case["N"], case["grid"], case["start"])


def real_step_rows(case, t=None):
    """The (N, S + 1) table the kernels walk: hode.real_step.interval_grids on the fp32 grid."""
    from hode.real_step import interval_grids
    t = real_step_inputs(case)["t"] if t is None else torch.tensor(np.asarray(t), dtype=torch.float32)
    return interval_grids(t, SUB_STEP_SIZE[case["grid"]])


def real_step_solve_cpu(case, p, dtype=torch.float64, t=None, rows=None):
    """sum(h * cot) and its gradients with one oracle solve per interval in `dtype`, on the fp32 inputs: interval i from
    init[i] over t[i : i + 2] with the grid's step_size (`t` replaces the grid, the start states stay in place).  With `rows`
    (an (N, S + 1) table) interval i is stepped along rows[i] as it stands, increasing or not, with oracle.solvers' own step
    functions: what a kernel that walked those numbers would compute."""
    from oracle.solvers import _FIXED, _Rhs, odeint as oracle_odeint
    from test_hip_kernel_variants import _real_flat
    f = copy.deepcopy(p["f"]).to(dtype)
    f.set_action_static(p["a"].to(dtype))
    init = p["init"].detach().to(dtype).clone().requires_grad_(True)
    method, perturb = case["method"], case["perturb"]
    ends = []
    for i in range(case["N"]):
        if rows is None:
            tt = (p["t"] if t is None else torch.tensor(np.asarray(t))).to(dtype)
            opts = {"perturb": perturb} if p["step_size"] is None else {"perturb": perturb, "step_size": p["step_size"]}
            ends.append(oracle_odeint(f, init[i], tt[i:i + 2], method=method, options=opts)[-1])
        else:
            rhs, y, row = _Rhs(f), init[i], rows[i].to(dtype)
            for t0, t1 in zip(row[:-1], row[1:]):
                y = y + _FIXED[method](rhs, t0, t1 - t0, t1, y, perturb)
            ends.append(y)
    h = torch.stack([torch.zeros_like(ends[0])] + ends)
    (h * p["cot"].to(dtype)).sum().backward()
    return dict(h=h.detach(), ginit=init.grad, gw=torch.cat([q.grad.reshape(-1) for q in _real_flat(f)]),
                gth=torch.stack([f.k_immunity.grad, f.kel.grad, f.kel2.grad]))


@functools.lru_cache(maxsize=None)
def _real_step_ref(D, H, B, N, grid_name, start, method, perturb):
    case = dict(N=N, method=method, perturb=perturb)
    return real_step_solve_cpu(case, _real_step_inputs(D, H, B, N, grid_name, start))


def real_step_ref(case):
    """The fp64 oracle of the case, computed once and left unchanged."""
    return _real_step_ref(case["D"], case["H"], case["B"], case["N"], case["grid"], case["start"], case["method"], case["perturb"])
