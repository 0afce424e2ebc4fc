"""The per-patient dopri5 controller of libhode_real_pp.so (include/hode_real_pp.h) in torch, at batch one, in float64 or
float32, on oracle.rhs.RocheRealRHS -- a plain helper module, not a conftest.

controller(): Hairer's first step (order 4, RMS over the patient's D components), attempts clipped to the next output time
(dt_used = min(dt, t[j] - t0); a clipped attempt ends at t[j] exactly), accept on ratio <= 1, dt <- dt_used * factor(ratio)
after every attempt, FSAL, the c = 1 stages at the left limit of t1.  The clock is float64, the stage times are cast to the
state dtype -- oracle.solvers' own _initial_step / _dp_attempt / _next_dt do the arithmetic.

replay(): the accepted steps of a GIVEN tape [(t0, dt_used, j)] with autograd: every step size is a constant, dt_0
included, so the gradient is the discrete adjoint the kernel computes."""
import torch

from oracle.solvers import DP_ALPHA, DP_BETA, DP_C_ERR, _Rhs, _dp_attempt, _initial_step, _next_dt, _rms

NONFINITE, DT_UNDERFLOW, MAX_STEPS = 1, 2, 4


def _tableau(dtype):
    return (tuple(float(torch.tensor(a, dtype=torch.float64).to(dtype)) for a in DP_ALPHA),
            tuple(torch.tensor(b, dtype=torch.float64).to(dtype) for b in DP_BETA),
            torch.tensor(DP_C_ERR, dtype=torch.float64).to(dtype))


@torch.no_grad()
def controller(func, y0, t, rtol, atol, max_steps=1 << 20, max_attempts=None):
    """One patient: y0 (1, D) in the dtype of the run, t (T,) increasing.  Returns dict(h (T, 1, D), tape [(t0, dt_used, j)]
    with j the output index the step reached or -1, states (the start state of every accepted step), n_accepted,
    n_rejected, status, ratios (one per attempt))."""
    assert y0.shape[0] == 1
    f = _Rhs(func)
    tab = _tableau(y0.dtype)
    t = t.to(torch.float64)
    T = t.numel()
    attempts_max = 8 * max_steps + 1024 if max_attempts is None else max_attempts
    f0 = f(t[0], y0)
    dt = _initial_step(f, t[0], y0, 4, rtol, atol, f0)
    t0, y, fy = t[0], y0, f0
    h = [y0] + [torch.full_like(y0, float("nan"))] * (T - 1)
    tape, states, ratios = [], [], []
    n_acc = n_rej = status = it = 0
    j = 1
    while j < T:
        if not bool(torch.isfinite(y).all()):
            status |= NONFINITE
            break
        if not bool(t0 + dt > t0):
            status |= DT_UNDERFLOW
            break
        if n_acc >= max_steps or it >= attempts_max:
            status |= MAX_STEPS
            break
        rem = t[j] - t0
        clip = not bool(dt < rem)
        dtu = rem if clip else dt
        t1 = t[j] if clip else t0 + dtu
        y1, f1, err, _ = _dp_attempt(f, y, fy, t0, dtu, t1, tab)
        tol = atol + rtol * torch.max(y.abs(), y1.abs())
        ratio = _rms(err / tol).abs()
        ratios.append(float(ratio))
        if bool(ratio <= 1):
            tape.append((float(t0), float(dtu), j if clip else -1))
            states.append(y)
            if clip:
                h[j] = y1
                j += 1
            t0, y, fy = t1, y1, f1
            n_acc += 1
        else:
            n_rej += 1
        dt = _next_dt(dtu, ratio)
        it += 1
    return dict(h=torch.stack(h, dim=0), tape=tape, states=states, n_accepted=n_acc, n_rejected=n_rej, status=status, ratios=ratios)


def replay(func, y0, t, tape):
    """One patient along a given tape, with autograd: h (T, 1, D); rows no step reached stay y0 (detached zeros never occur
    for a finished patient: every output is a step endpoint)."""
    f = _Rhs(func)
    tab = _tableau(y0.dtype)
    t = t.to(torch.float64)
    out = [y0] * t.numel()
    y, fy = y0, f(t[0], y0)
    for t_n, dt_n, j in tape:
        t_lo, dt = torch.tensor(float(t_n), dtype=torch.float64), torch.tensor(float(dt_n), dtype=torch.float64)
        t_hi = t[j] if j >= 0 else t_lo + dt
        y1, f1, _, _ = _dp_attempt(f, y, fy, t_lo, dt, t_hi, tab)
        if j >= 0:
            out[j] = y1
        y, fy = y1, f1
    return torch.stack(out, dim=0)


def tape_is_clipped(tape, t, T=None):
    """The invariants of a finished patient's tape: steps are contiguous, none crosses an output time, a step that reaches
    output j ends at t[j] exactly, and the outputs are reached in order 1 .. T - 1."""
    t = [float(x) for x in t.to(torch.float64)]
    j_next, now = 1, t[0]
    for t0, dtu, j in tape:
        if t0 != now or not dtu > 0:
            return False
        if j >= 0:
            if j != j_next or t0 + dtu > t[j] + 1e-12 * max(1.0, abs(t[j])) or abs(t0 + dtu - t[j]) > 1e-9 * max(1.0, abs(t[j])):
                return False
            now, j_next = t[j], j_next + 1
        else:
            if not t0 + dtu < t[j_next]:
                return False
            now = t0 + dtu
    return j_next == len(t)
