"""A float64 audit of a dopri5 step CONTROLLER at batch one (tests/test_hip_dopri5_pp.py, tests/test_dopri5_pp_host.py): given
one patient's inputs, tolerances, accepted-step tape (t_n, dt_n and the fp32 start state y_n of every accepted step) and
rejected count, re-run the controller in float64 with oracle.solvers' own pieces and say whether the tape is the one
torchdiffeq's controller takes.  The float64 replay of a tape checks the accepted-step algebra GIVEN the step sequence;
this checks the sequence: Hairer's first step, the error norm and its count, rtol / atol, the tolerance vector, the step
factor, and every accept / reject decision.  A plain helper module, not a conftest.  No GPU here.

The audit re-synchronises to the tape's own state at every accepted step, so differences do not accumulate: what is
compared at step n is one controller decision chain from (t_n, y_n) and the dt proposed after step n - 1.

What fp32 leaves open.  An fp32 error ratio sits within `ratio_margin * max(1, ratio)` of float64's (measured on the fp32
oracle, tests/dopri5_pp_cases.py).  Two things follow.  (1) A decision whose float64 ratio is that close to 1 is
undecidable; the patient is then left out.  (2) The step size proposed from a ratio r is dt * min(10, max(0.9 r^-1/5, ..)),
so a ratio uncertainty d moves the proposal by 0.2 d / r: nothing at r ~ 0.5, but Hairer's conservative first step and
every step cut down by a dose are followed by a ratio of 1e-6 .. 1e-5, where the estimate is roundoff and the fp32
oracle's proposal differs from float64's by up to 75 %.  So a proposal is carried as the interval of step sizes that the
ratios within the margin give, both of its ends are run through the reject chain (SPREAD starts across it where the
margin is more than PINNED of the ratio), and the tape's dt_n has to lie between the results (widened by `dt_rtol`).
Where the starts reject a different number of times -- which chain the audited controller took was decided by the last
bits of a roundoff-level ratio -- the step is OPEN: it must not be longer than the largest proposal, float64 must accept
it, it counts one rejection if it is shorter than the smallest proposal, and the patient's rejected count is then held
from below only ("exact" False).  At ratios of 0.01 and more the interval is narrower than 2 % and a wrong safety
factor, norm or tolerance vector falls outside it; the first step's proposal, Hairer's, is a point."""
import copy

import torch

from oracle import solvers as S

SPREAD = 5  # starts across a proposal that is not pinned
PINNED = 0.05  # a proposal is followed through its chain when the margin is at most this share of the ratio it comes from
MAX_CHAIN = 64  # attempts at one (t_n, y_n): dfactor 0.2 per rejection, far more than any tape here needs


def patient_rhs(f, dosage, times, p, dtype=torch.float64):
    """A copy of the rhs `f` in `dtype` that serves patient `p` alone (batch one) with the given dose schedule."""
    fm = copy.deepcopy(f).to(dtype)
    fm.dosage, fm.times = dosage[p:p + 1].to(dtype), times[p:p + 1].to(dtype)
    return fm


def tableau(dtype):
    """oracle.solvers._odeint_dopri5's tableau: the fp32-rounded coefficients in `dtype`."""
    return (tuple(float(torch.tensor(a, dtype=torch.float64).to(dtype)) for a in S.DP_ALPHA),
            tuple(torch.tensor(b, dtype=torch.float64).to(dtype) for b in S.DP_BETA),
            torch.tensor(S.DP_C_ERR, dtype=torch.float64).to(dtype))


def error_ratio(f, y, f0, t0, dt, tab, rtol, atol):
    """The error ratio of one attempt, as _odeint_dopri5 forms it."""
    y1, _, err, _ = S._dp_attempt(f, y, f0, t0, dt, t0 + dt, tab)
    tol = atol + rtol * torch.max(y.abs(), y1.abs())
    return S._rms(err / tol).abs()


def _f0(f, t, n, t_n, y):
    """k1 of accepted step n from its start state: f(t[0], y0), afterwards FSAL's f just before t_n."""
    return f(t[0], y) if n == 0 else f(t_n, y, S._Rhs.PREV)


def implied_ratio(factor):
    """The ratio a step factor dt_next / dt strictly inside the clamps (1 < factor < 10) comes from, else None."""
    return (0.9 / factor) ** 5 if 1.0 + 1e-9 < factor < 10.0 - 1e-9 else None


@torch.no_grad()
def audit(rhs64, y0, t, rtol, atol, tape, n_rejected, ratio_margin, dt_rtol):
    """`tape` = {"t": [...], "dt": [...], "y": (n, D) fp32 tensor}.  Returns a report: "ok", "why" (the first disagreement),
    "left_out" (undecidable, see above: nothing is claimed about the patient), "dt_dist" (the largest relative distance of
    an accepted dt from the interval float64 allows it), "ratio_dist" (where a step follows its predecessor without a
    rejection and inside the clamps, the tape's dt_n / dt_{n-1} names the ratio the audited controller saw: its largest
    distance from float64's, relative to max(1, ratio)), "clearance" (the smallest |ratio - 1| of a decision),
    "n_rejected" (float64's count: the tape's has to equal it when "exact", else to reach it), "steps" and "open_steps"."""
    f = S._Rhs(rhs64)
    tab = tableau(torch.float64)
    t = t.to(torch.float64)
    rep = {"ok": False, "why": "", "left_out": False, "dt_dist": 0.0, "ratio_dist": 0.0, "clearance": float("inf"), "n_rejected": 0,
           "open_steps": 0, "steps": len(tape["t"]), "exact": False}

    def fail(why):
        rep["why"] = why
        return rep

    def leave_out(why):
        rep["left_out"] = True
        return fail("undecidable: " + why)

    def decide(ratio):  # True: accept, False: reject, None: undecidable
        rep["clearance"] = min(rep["clearance"], abs(float(ratio) - 1.0))
        if not abs(float(ratio) - 1.0) > ratio_margin * max(1.0, float(ratio)):  # a NaN ratio lands here too
            return None
        return bool(ratio <= 1)

    def propose(dt, ratio):  # the step sizes the ratios within the margin propose: (smallest, largest)
        d = ratio_margin * max(1.0, float(ratio))
        return S._next_dt(dt, ratio + d), S._next_dt(dt, torch.clamp(ratio - d, min=0.0))

    def chain(y, f0, t_n, dt, side):  # attempts from one end of the proposal: (accepted dt, rejections), None: undecidable
        for rejected in range(MAX_CHAIN):
            ratio = error_ratio(f, y, f0, t_n, dt, tab, rtol, atol)
            verdict = decide(ratio)
            if verdict is None:
                return None
            if verdict:
                return dt, rejected
            dt = propose(dt, ratio)[side]
        return dt, MAX_CHAIN

    n_steps = len(tape["t"])
    if n_steps == 0:
        return fail("empty tape")
    if tape["t"][0] != float(t[0]) or not torch.equal(tape["y"][0].reshape(-1), y0.reshape(-1).to(tape["y"].dtype)):
        return fail("step 0 does not start at (t[0], y0)")
    lo = hi = last = None  # the proposal for the next step and the ratio it comes from
    for n in range(n_steps):
        t_n = torch.tensor(tape["t"][n], dtype=torch.float64)
        dt_n = torch.tensor(tape["dt"][n], dtype=torch.float64)
        if n > 0 and float(t[-1]) <= tape["t"][n]:
            return fail("step %d starts after the last output time was covered" % n)
        y = tape["y"][n].to(torch.float64).reshape(1, -1)
        f0 = _f0(f, t, n, t_n, y)
        if n == 0:
            lo = hi = S._initial_step(f, t[0], y, 4, rtol, atol, f0)
        # a proposal known to 1 % is followed through its chain from both ends, a wider one from SPREAD starts across it
        pinned = n == 0 or ratio_margin * max(1.0, float(last)) <= PINNED * float(last)
        if pinned:
            runs = [chain(y, f0, t_n, lo, 0), chain(y, f0, t_n, hi, 1)]
        else:
            runs = [chain(y, f0, t_n, lo * (hi / lo) ** (i / (SPREAD - 1.0)), int(2 * i >= SPREAD)) for i in range(SPREAD)]
        if pinned and None in runs:
            return leave_out("step %d: a ratio within the margin of 1" % n)
        if None not in runs and max(r[1] for r in runs) == MAX_CHAIN:
            return fail("step %d: float64 rejects %d times in a row" % (n, MAX_CHAIN))
        if None not in runs and len({r[1] for r in runs}) == 1:  # every start rejects the same number of times
            a = runs[0]
            rep["n_rejected"] += a[1]
            low, high = min(float(r[0]) for r in runs), max(float(r[0]) for r in runs)
            dist = max(low - float(dt_n), float(dt_n) - high, 0.0) / abs(float(dt_n))
            rep["dt_dist"] = max(rep["dt_dist"], dist)
            if not dist <= dt_rtol:
                return fail("step %d at t = %.9g: dt %.9g, float64's controller takes %.9g .. %.9g after %d rejections (relative %.3e > %.3e)"
                            % (n, float(t_n), float(dt_n), low, high, a[1], dist, dt_rtol))
            if n > 0 and a[1] == 0 and implied_ratio(tape["dt"][n] / tape["dt"][n - 1]) is not None:
                seen = implied_ratio(tape["dt"][n] / tape["dt"][n - 1])
                rep["ratio_dist"] = max(rep["ratio_dist"], abs(seen - float(last)) / max(1.0, float(last)))
        else:
            # an open step: the proposal is not known well enough to follow its chain (or its two ends reject a different
            # number of times).  What still holds: the step is no longer than the largest proposal, it took a rejection
            # to get below the smallest, and float64 accepts it (below)
            rep["open_steps"] += 1
            dist = max(float(dt_n) - float(hi), 0.0) / abs(float(dt_n))
            rep["dt_dist"] = max(rep["dt_dist"], dist)
            if not dist <= dt_rtol:
                return fail("step %d at t = %.9g: dt %.9g is longer than the largest proposal %.9g (relative %.3e > %.3e)"
                            % (n, float(t_n), float(dt_n), float(hi), dist, dt_rtol))
            rep["n_rejected"] += int(float(dt_n) < float(lo) * (1.0 - dt_rtol))
        ratio = error_ratio(f, y, f0, t_n, dt_n, tab, rtol, atol)  # the tape's own step
        verdict = decide(ratio)
        if verdict is None:
            return leave_out("step %d: the ratio of the tape's own step is within the margin of 1" % n)
        if not verdict:
            return fail("step %d: float64 rejects the tape's own step (ratio %.6f)" % (n, float(ratio)))
        lo, hi = propose(dt_n, ratio)
        last = ratio
    if not tape["t"][-1] + tape["dt"][-1] >= float(t[-1]):
        return fail("the tape ends before the last output time")
    rep["exact"] = rep["open_steps"] == 0
    if int(n_rejected) < rep["n_rejected"] or (rep["exact"] and int(n_rejected) != rep["n_rejected"]):
        return fail("%d rejected attempts, float64's controller rejects %s%d" % (int(n_rejected), "" if rep["exact"] else "at least ", rep["n_rejected"]))
    rep["ok"] = True
    return rep


@torch.no_grad()
def ratio_distances(rhs64, t, rtol, atol, stats):
    """For a free run of oracle.solvers' dopri5 at batch one (its `stats` with "states" and "attempts"): the distance
    |ratio - ratio64| / max(1, ratio64) of every attempt's error ratio from the float64 ratio of the SAME attempt (same
    start state, t and dt)."""
    f = S._Rhs(rhs64)
    tab = tableau(torch.float64)
    t = t.to(torch.float64)
    out = []
    for n, t_a, dt_a, ratio in stats["attempts"]:
        y = stats["states"][n].to(torch.float64)
        t_a, dt_a = torch.tensor(t_a, dtype=torch.float64), torch.tensor(dt_a, dtype=torch.float64)
        r64 = float(error_ratio(f, y, _f0(f, t, n, t_a, y), t_a, dt_a, tab, rtol, atol))
        out.append(abs(ratio - r64) / max(1.0, r64))
    return out


@torch.no_grad()
def free_run(rhs, y0, t, rtol, atol):
    """oracle.solvers' dopri5 free-running on one patient in the dtype of `rhs`: (h, stats, tape) with the tape in the
    form audit() takes."""
    dtype = next(rhs.parameters()).dtype
    st = {}
    h = S.odeint(rhs, y0.to(dtype).reshape(1, -1), t.to(dtype), method="dopri5", rtol=rtol, atol=atol, stats=st)
    tape = {"t": [a for a, _ in st["tape"]], "dt": [b for _, b in st["tape"]], "y": torch.cat(st["states"], dim=0)}
    return h, st, tape
