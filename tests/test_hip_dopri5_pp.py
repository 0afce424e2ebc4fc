"""dopri5 with per-patient step control (libhode_dopri5_pp.so, hode.patient_dopri5, RocheODE.step_control = "patient") on the
GPU: independence of the patients, every case of tests/dopri5_pp_cases.py -- synth's uniform grid and the non-uniform and
offset grids of tests/time_grids.py -- against the float64 replay of its own tapes, the free-running oracle per patient,
the float64 audit of the step controller at loose tolerances (tests/dopri5_pp_audit.py), a fine fixed-grid solve, the
tape-less forward, sentinels, repeats, the status paths and the model level.  GPU only.

Per-patient mode is torchdiffeq run on each patient as a batch of one, with every step size a constant in the backward
(dt_0 included), so the references are the CPU oracle at batch one: `oracle.solvers.odeint(method="dopri5")` free-running
and `odeint_dopri5_replay(..., first_attempt_accepted=False)` along the device's own tape."""
import copy
import ctypes

import pytest
import torch

import dopri5_pp_cases as cases
from oracle.rhs import RocheRHS, THETA_NAMES
from oracle.solvers import odeint as oracle_odeint, odeint_dopri5_replay

pytestmark = pytest.mark.gpu

RTOL, ATOL = cases.RTOL, cases.ATOL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _names(f):
    return list(THETA_NAMES) + (["theta_1", "theta_2"] if f.ablate else [])


def _device_args(inp, f, dev):
    """(y0, theta, w, b, t, dosage, dose_times) on the device, as the launch functions take them."""
    from hode.solver import pack_theta
    scal = [getattr(f, n).detach().to(dev) for n in _names(f)]
    dosage, times = cases.schedule(inp, f)
    w = f.ml_net[0].weight.detach().to(dev) if f.ml_dim > 0 else None
    b = f.ml_net[0].bias.detach().to(dev) if f.ml_dim > 0 else None
    return (inp["z0"].to(dev), pack_theta(scal, dev), w, b, inp["t"].to(dev), dosage.to(dev), times.to(dev))


def _tape_states(ws, B, D, max_steps, n_acc):
    """The fp32 start state of every accepted step, per patient, out of a forward's workspace: tape_y is
    [max_steps][B][D] at the last offset hode_dopri5_pp_tape_offsets reports."""
    from hode import _dopri5_pp_lib as PL
    d = PL.new_desc()
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.max_steps = B, D, 1, 1, int(max_steps)
    off = (ctypes.c_size_t * 5)()
    PL.check(PL.lib().hode_dopri5_pp_tape_offsets(d, off), "hode_dopri5_pp_tape_offsets")
    assert off[4] % 4 == 0 and off[4] // 4 + max_steps * B * D <= ws.numel()
    y = ws[off[4] // 4:off[4] // 4 + max_steps * B * D].cpu().view(torch.float32).reshape(max_steps, B, D)
    return [y[:n, p].clone() for p, n in enumerate(n_acc.cpu().tolist())]


def _solve(inp, f, dev, cot=None, need_theta=True, rtol=RTOL, atol=ATOL, **kw):
    """Forward (+ backward when `cot` is given) through the two launch functions; everything comes back on the CPU."""
    from hode import patient_dopri5 as PP
    args = _device_args(inp, f, dev)
    h, ws, stats = PP.patient_dopri5_forward(*args, rtol=rtol, atol=atol, ablate=f.ablate, **kw)
    B, D = inp["z0"].shape
    out = {"h": h.cpu(), "n_acc": stats["n_accepted"].cpu(), "n_rej": stats["n_rejected"].cpu(), "status": stats["status"].cpu(),
           "max_steps": stats["max_steps"], "workspace_bytes": stats["workspace_bytes"], "ws": ws}
    if not kw.get("no_tape"):
        out["tapes"] = PP.read_tape(ws, B, D, stats["max_steps"], stats["n_accepted"])
        out["tape_y"] = _tape_states(ws, B, D, stats["max_steps"], stats["n_accepted"])
    if cot is not None:
        gy0, gth, gw, gb = PP.patient_dopri5_backward(*args, h, ws, stats["n_accepted"], stats["max_steps"], cot.to(dev), rtol=rtol,
                                                      atol=atol, ablate=f.ablate, need_theta=need_theta)
        out["gy0"] = gy0.cpu()
        if gth is not None:
            out["gtheta"] = gth.cpu()[:len(_names(f))]
        if gw is not None:
            out["gw"], out["gb"] = gw.cpu(), gb.cpu()
    torch.cuda.synchronize()
    return out


def _replay(inp, f, cot, tapes, patients, double):
    """The oracle's accepted-step algebra at batch ONE along each listed patient's own device tape, every step size a
    constant (first_attempt_accepted=False): h rows, grad_y0 rows, and the parameter gradients summed over the patients."""
    fm = copy.deepcopy(f).double() if double else copy.deepcopy(f)
    dt = torch.float64 if double else torch.float32
    for p_ in fm.parameters():
        p_.grad = None
    hs, gy = [], []
    dosage, times = cases.schedule(inp, f)
    for p in patients:
        fm.dosage, fm.times = dosage[p:p + 1].to(dt), times[p:p + 1].to(dt)
        y0 = inp["z0"][p:p + 1].to(dt).clone().requires_grad_(True)
        tape = tapes[p]
        h = odeint_dopri5_replay(fm, y0, inp["t"].to(dt), RTOL, ATOL, list(zip(tape["t"], tape["dt"])), False)
        (h * cot[:, p:p + 1].to(dt)).sum().backward()  # parameter gradients accumulate over the patients
        hs.append(h.detach())
        gy.append(y0.grad)
    zero = torch.zeros((), dtype=dt)
    out = {"h": torch.cat(hs, dim=1), "gy0": torch.cat(gy, dim=0),
           "gtheta": torch.stack([getattr(fm, n).grad if getattr(fm, n).grad is not None else zero for n in _names(f)])}
    if f.ml_dim > 0:
        out["gw"], out["gb"] = fm.ml_net[0].weight.grad, fm.ml_net[0].bias.grad
    return out


# --------------------------------------------------------------------------------------- 2. tape replay, every case
@pytest.mark.parametrize("case", cases.CASES + cases.GRID_CASES, ids=cases.case_id)
def test_every_case_follows_the_float64_replay_of_its_own_tapes(case, record_property):
    """Every compiled instantiation (tests/test_dopri5_pp_host.py holds the table against the library's symbols).  The
    cotangent is non-zero on the patients of cases.subset(B) -- all of them up to B = 5, else both ends of both waves -- so
    that the float64 replay of exactly those patients gives the h rows, the grad_y0 rows and the parameter gradients summed
    over patients; the other patients' grad_y0 rows are exact zeros.

    Bounds: values within 2e-5 * scale (case (a) of test_dopri5_gradients_follow_the_tape_replay_oracle: the same algebra);
    gradients at a relative distance of at most max(1e-5, 2 x the fp32 oracle replay's distance from the fp64 replay on
    that tape) -- calibrated on the oracle, not on the kernel.

    Measured on an MI355X over the 21 cases that integrate: |h - h64| at most 5.1e-6 (the bound is at least 2e-5); gradient
    distances 5.5e-8 .. 2.0e-6 with the fp32 oracle replay at 3.3e-8 .. 2.3e-6 from the fp64 one, i.e. at most 0.2 of the
    bound.

    GRID_CASES: the same on the clustered grid (one accepted step covers several output times -- the forward's inner j loop
    and the sweep's sum over several grad_h rows -- and many cover none: empty tape_j ranges) and on the grids that start at
    2.5 and at -1.0 and cross 0 (nextafter_down of a negative t0f), with a dose before t[0], on t[0] and strictly inside
    grid steps, up to three per patient.  Measured over these 16 cases: |h - h64| at most 1.5e-6, gradient distances
    5.1e-8 .. 9.3e-7 with the fp32 oracle replay at 9.0e-8 .. 2.5e-6, at most 0.09 of the bound."""
    dev = _dev()
    inp, f = cases.setup(case)
    B, D, T = case["B"], case["D"], case["T"]
    S = cases.subset(B)
    cot = torch.zeros(T, B, D)
    cot[:, S] = torch.randn(T, len(S), D, generator=torch.Generator().manual_seed(3))
    hip = _solve(inp, f, dev, cot, need_theta=case["need_theta"])
    assert hip["h"].shape == (T, B, D) and torch.equal(hip["h"][0], inp["z0"]) and not hip["status"].any()
    assert ("gtheta" in hip) == case["need_theta"] and ("gw" in hip) == (D > 4)
    if T == 1:  # nothing to integrate
        assert not hip["n_acc"].any() and not hip["n_rej"].any() and torch.equal(hip["gy0"], cot[0])
        for k in ("gw", "gb", "gtheta"):
            assert k not in hip or not hip[k].any()
        return
    assert int(hip["n_acc"].min()) >= 1 and all(len(tp["t"]) == int(n) for tp, n in zip(hip["tapes"], hip["n_acc"]))
    t64 = inp["t"].double().tolist()
    for tp in hip["tapes"]:  # every tape starts at t[0], is contiguous in time and hands out every output index once
        assert tp["t"][0] == float(inp["t"][0]) and all(a + b == c for a, b, c in zip(tp["t"], tp["dt"], tp["t"][1:]))
        assert tp["j"][0][0] == 1 and tp["j"][-1][1] == T and all(a[1] == b[0] for a, b in zip(tp["j"], tp["j"][1:]))
        # and a step's range is exactly the output times inside (t_n, t_n + dt_n]
        assert all(all(a < t64[j] <= a + b for j in range(lo, hi)) and (hi == T or t64[hi] > a + b)
                   for a, b, (lo, hi) in zip(tp["t"], tp["dt"], tp["j"]))
    if case.get("grid") == "clustered":  # one accepted step covers several output times, several cover none
        widths = [[hi - lo for lo, hi in hip["tapes"][p]["j"]] for p in S]
        assert max(map(max, widths)) >= 3 and all(sum(1 for w in ws if w == 0) >= 2 for ws in widths), widths
    elif "grid" in case:  # from the inputs: a replayed patient with a dose before t[0] and one with a dose exactly on it
        times = inp["times"][S]
        assert bool((times < inp["t"][0]).any()) and bool((times == inp["t"][0]).any())
    r64 = _replay(inp, f, cot, hip["tapes"], S, True)
    r32 = _replay(inp, f, cot, hip["tapes"], S, False)
    scale = 1 + r64["h"].abs().max().item()
    herr = (hip["h"][:, S].double() - r64["h"]).abs().max().item()
    print("%s: |h - h64| = %.3e (bound %.3e)" % (cases.case_id(case), herr, 2e-5 * scale))
    figures = {}
    others = [p for p in range(B) if p not in S]
    for k in ("gy0", "gw", "gb", "gtheta"):
        if k not in hip:
            continue
        got = hip[k][S] if k == "gy0" else hip[k]
        if float(r64[k].abs().max()) < 1e-12:
            assert float(got.abs().max()) < 1e-12, k
            continue
        figures[k] = (_rel(got, r64[k]), _rel(r32[k], r64[k]))
        print("  %s: rel %.3e, fp32 oracle %.3e" % ((k,) + figures[k]))
    record_property("err_h", herr)
    record_property("err_h_bound", 2e-5 * scale)
    for k, (err, noise) in figures.items():
        record_property("err_" + k, err)
        record_property("fp32_oracle_" + k, noise)
    assert herr <= 2e-5 * scale
    assert not hip["gy0"][others].any()
    for k, (err, noise) in figures.items():
        assert err <= max(1e-5, 2.0 * noise), (k, err, noise)


# ------------------------------------------------------------------------------------------------- 1. independence
def test_a_patient_is_solved_the_same_alone_and_anywhere_in_a_batch():
    """The defining property: a patient's h rows, tape, step counts and grad_y0 row are bit-identical whether it is solved
    in a batch of 70, alone, or at another position of a shuffled batch."""
    dev = _dev()
    case = cases.CASES[0]
    assert (case["B"], case["D"], case["T"]) == (70, 12, 20)
    inp, f = cases.setup(case)
    B, D, T = 70, 12, 20
    cot = torch.randn(T, B, D, generator=torch.Generator().manual_seed(5))
    full = _solve(inp, f, dev, cot)
    assert len(set(full["n_acc"].tolist())) > 1  # the patients do take different numbers of steps
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(6))
    shuf = _solve({"z0": inp["z0"][perm], "actions": inp["actions"][:, perm], "t": inp["t"]}, f, dev, cot[:, perm])
    for new, old in enumerate(perm.tolist()):
        assert torch.equal(shuf["h"][:, new], full["h"][:, old]) and torch.equal(shuf["gy0"][new], full["gy0"][old]), old
        assert shuf["tapes"][new] == full["tapes"][old], old
        assert (shuf["n_acc"][new], shuf["n_rej"][new]) == (full["n_acc"][old], full["n_rej"][old]), old
    for p in cases.subset(B):
        one = _solve({"z0": inp["z0"][p:p + 1], "actions": inp["actions"][:, p:p + 1], "t": inp["t"]}, f, dev, cot[:, p:p + 1])
        assert torch.equal(one["h"][:, 0], full["h"][:, p]) and torch.equal(one["gy0"][0], full["gy0"][p]), p
        assert one["tapes"][0] == full["tapes"][p], p
        assert (int(one["n_acc"][0]), int(one["n_rej"][0])) == (int(full["n_acc"][p]), int(full["n_rej"][p])), p


# ------------------------------------------------------------------------------------------- 3. free-running oracle
STIFF = 1  # this patient's start state is scaled up: Hairer's first step is then too long and its first attempt rejected
STIFF_SCALE = {12: 300.0, 6: 1000.0}  # picked on the CPU from the oracle's own counts


@pytest.mark.parametrize("D", [12, 6])
def test_forward_against_the_free_running_oracle_per_patient(D):
    """`oracle.solvers.odeint(method="dopri5")` on each patient as a batch of one.  Total accepted steps within the 15 % and
    the trajectory within the 1e-4 * scale of test_dopri5_forward_backward_vs_oracle.  That the inputs exercise the
    controller is asserted on the ORACLE's counts: the patients take different numbers of steps, some reject, and one
    patient's first attempt is rejected (seed and the scaled patient were picked on the CPU so that this holds)."""
    dev = _dev()
    B, T = 6, 12
    from hode import synth
    inp = synth.solver_inputs(B, T, D, seed=50)
    inp["z0"][STIFF] *= STIFF_SCALE[D]
    torch.manual_seed(50)
    f = RocheRHS(D, synth.STEP)
    with torch.no_grad():
        f.ml_net[0].weight.mul_(2.0)
    rows, counts = [], []
    with torch.no_grad():
        for p in range(B):
            f.set_action(inp["actions"][:, p:p + 1])
            st = {}
            rows.append(oracle_odeint(f, inp["z0"][p:p + 1], inp["t"], method="dopri5", rtol=RTOL, atol=ATOL, stats=st))
            counts.append((st["n_accepted"], st["n_rejected"], st["first_attempt_accepted"]))
    assert len({c[0] for c in counts}) > 1 and any(c[1] > 0 for c in counts) and any(not c[2] for c in counts), counts
    ora = torch.cat(rows, dim=1)
    hip = _solve(inp, f, dev)
    total, total_o = int(hip["n_acc"].sum()), sum(c[0] for c in counts)
    scale = 1 + ora.abs().max().item()
    err = (hip["h"] - ora).abs().max().item()
    print("accepted %d (oracle %d), rejected %d (oracle %d), |h - h_oracle| = %.3e (bound %.3e); per patient %s vs oracle %s"
          % (total, total_o, int(hip["n_rej"].sum()), sum(c[1] for c in counts), err, 1e-4 * scale,
             list(zip(hip["n_acc"].tolist(), hip["n_rej"].tolist())), [c[:2] for c in counts]))
    assert abs(total - total_o) <= 0.15 * total_o
    assert torch.equal(hip["h"][0], ora[0]) and err <= 1e-4 * scale
    first = hip["tapes"][STIFF]
    assert int(hip["n_rej"][STIFF]) > 0 and first["t"][0] == 0.0


# ------------------------------------------------------------------------------------------ 3b. the controller audit
@pytest.mark.parametrize("case", cases.AUDIT_CASES, ids=cases.audit_id)
def test_the_controller_follows_the_float64_controller(case, record_property):
    """WHICH steps are taken (the replay above checks the algebra given the steps): tests/dopri5_pp_audit.py re-runs
    torchdiffeq's controller in float64 from the kernel's own (t_n, y_n) of every accepted step -- Hairer's first step, the
    RMS norm over the patient's D components, atol + rtol * max(|y|, |y1|), accept / reject, 0.9 ratio^(-1/5) with its
    clamps -- at tolerances where the error estimate is more than roundoff, on non-uniform grids with doses inside steps.
    Every accepted dt has to lie where float64's controller, with ratios within RATIO_MARGIN of its own, puts it (within
    DT_RTOL), float64 has to accept every step of the tape, and the rejected count has to be float64's.  Both constants
    are 8 x what the fp32 oracle shows when it is audited the same way (tests/dopri5_pp_cases.py;
    tests/test_dopri5_pp_host.py shows that a norm over the wrong count, swapped tolerances, a safety factor of 0.8, a
    tolerance from |y| alone and half of Hairer's step each fail this audit).  At most one audited patient in ten may be
    undecidable, i.e. none of five.

    Measured on an MI355X over the 45 audited patients: none undecidable, every dt inside its interval with the largest
    distance 4.6e-5 (DT_RTOL 5.4e-3), the ratios that dt_n / dt_{n-1} names within 5.1e-5 of float64's (RATIO_MARGIN
    7.0e-4); the two scaled-up patients take 42 / 39 steps with 10 / 6 rejections, float64's counts exactly."""
    import dopri5_pp_audit as audit
    dev = _dev()
    inp, f = cases.setup(case)
    B, S = case["B"], cases.subset(case["B"])
    hip = _solve(inp, f, dev, rtol=case["rtol"], atol=case["atol"])
    assert not hip["status"].any() and torch.isfinite(hip["h"]).all()
    dosage, times = cases.schedule(inp, f)
    left_out, worst = [], {"dt": 0.0, "ratio": 0.0}
    for p in S:
        tape = dict(hip["tapes"][p], y=hip["tape_y"][p])
        rep = audit.audit(audit.patient_rhs(f, dosage, times, p), inp["z0"][p], inp["t"], case["rtol"], case["atol"], tape,
                          int(hip["n_rej"][p]), cases.RATIO_MARGIN, cases.DT_RTOL)
        print("patient %d: %d accepted, %d rejected (float64 %s%d), %d of %d steps open, dt distance %.3e, ratio distance %.3e, "
              "clearance %.3e %s" % (p, int(hip["n_acc"][p]), int(hip["n_rej"][p]), "" if rep.get("exact") else ">= ", rep["n_rejected"],
                                    rep["open_steps"], rep["steps"], rep["dt_dist"], rep["ratio_dist"], rep["clearance"], rep["why"]))
        worst["dt"], worst["ratio"] = max(worst["dt"], rep["dt_dist"]), max(worst["ratio"], rep["ratio_dist"])
        if rep["left_out"]:
            left_out.append(p)
        else:
            assert rep["ok"], (p, rep["why"])
    record_property("audit_dt_dist", worst["dt"])
    record_property("audit_ratio_dist", worst["ratio"])
    record_property("left_out", len(left_out))
    assert 10 * len(left_out) <= len(S), left_out
    if "stiff" in case:  # the scaled patient's first attempt is rejected: its first step is shorter than Hairer's
        assert int(hip["n_rej"][cases.STIFF]) > 0
    assert len(set(hip["n_acc"][S].tolist())) > 1 and int(hip["n_rej"][S].sum()) > 0


# ------------------------------------------------------------------------------------- 4. fine grid, growing tapes
def test_matches_a_much_finer_rk4_solve_and_the_tapes_grow():
    """Property at a batch of several waves: agreement with a fixed-grid solve on a grid 8 times finer, in float64, within
    the 5e-4 * scale of test_dopri5_matches_fine_rk4_and_tape_grows.  The fine solve uses the 3/8 rule with
    options["perturb"], which evaluates the first and last stage just inside the step: the fine grid contains every dose
    time, so the jumps cost it nothing and no time point has to be excluded.  The solve starts from tapes of 4 rows and has
    to grow them."""
    from hode import synth
    dev = _dev()
    N, T, D, sub = 300, 30, 12, 8
    inp, f = cases.setup({"B": N, "T": T, "D": D, "K": 1, "ablate": False, "hill": "two", "seed": 5})
    hip = _solve(inp, f, dev, max_steps=4)
    assert torch.isfinite(hip["h"]).all() and hip["max_steps"] > 4 and int(hip["n_acc"].max()) <= hip["max_steps"]
    assert int(hip["n_acc"].min()) >= 1 and int(hip["n_acc"].max()) > 4 and len(set(hip["n_acc"].tolist())) > 1
    pick = [0, 63, 64, 127, 128, 255, 256, 299]
    f64 = copy.deepcopy(f).double()
    f64.set_action(inp["actions"][:, pick])
    f64.dosage, f64.times = f64.dosage.double(), f64.times.double()
    t = inp["t"].double()
    fine = torch.cat([t[:-1, None] + (t[1:, None] - t[:-1, None]) * torch.arange(sub, dtype=torch.float64) / sub, t[-1:, None].expand(1, sub)], 0)
    fine = fine.reshape(-1)[:(T - 1) * sub + 1]
    assert torch.equal(fine[::sub], t)
    with torch.no_grad():
        ref = oracle_odeint(f64, inp["z0"][pick].double(), fine, method="rk4", options={"perturb": True})[::sub]
    err = (hip["h"][:, pick].double() - ref).abs().max().item()
    print("|h - h_fine| = %.3e (bound %.3e), tapes grew to %d rows" % (err, 5e-4 * (1 + ref.abs().max().item()), hip["max_steps"]))
    assert err <= 5e-4 * (1 + ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------- 5. no tape
def test_the_forward_without_a_tape_is_the_same_forward():
    dev = _dev()
    inp, f = cases.setup(cases.CASES[0])
    taped = _solve(inp, f, dev)
    bare = _solve(inp, f, dev, no_tape=True)
    assert torch.equal(bare["h"], taped["h"]) and torch.equal(bare["n_acc"], taped["n_acc"]) and torch.equal(bare["n_rej"], taped["n_rej"])
    huge = _solve(inp, f, dev, no_tape=True, max_steps=1 << 20)  # the step bound costs nothing without a tape
    assert torch.equal(huge["h"], taped["h"])
    assert huge["workspace_bytes"] == bare["workspace_bytes"] < 4096 < taped["workspace_bytes"]
    assert taped["workspace_bytes"] >= taped["max_steps"] * 70 * (12 * 4 + 24)
    # a backward cannot follow: the library refuses it, nothing is launched
    from hode import HodeConfigError, patient_dopri5 as PP
    args = _device_args(inp, f, dev)
    with pytest.raises(HodeConfigError, match="workspace"):
        PP.patient_dopri5_backward(*args, bare["h"].to(dev), bare["ws"], bare["n_acc"].to(dev), bare["max_steps"],
                                   torch.zeros(20, 70, 12, device=dev), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------ 6. sentinels, repeats
GUARD = 64  # elements in front of and behind every buffer


class _Guarded:
    """A buffer between two guard zones filled with a pattern; the pointer handed out is 256-byte aligned."""

    def __init__(self, n, dtype, dev, fill):
        self.n, self.fill = int(n), fill
        self.whole = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        assert self.whole.data_ptr() % 256 == 0 and (GUARD * self.whole.element_size()) % 256 == 0

    @property
    def body(self):
        return self.whole[GUARD:GUARD + self.n]

    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        return bool((self.whole[:GUARD] == self.fill).all()) and bool((self.whole[GUARD + self.n:] == self.fill).all())


@pytest.mark.parametrize("D,B,T,K,grid", [(12, 70, 9, 1, None), (6, 3, 7, 2, None), (4, 65, 5, 1, None), (12, 70, 12, 3, "clustered")],
                         ids=["12-70-9-1", "6-3-7-2", "4-65-5-1", "clustered-12-70-12-3"])
def test_nothing_is_written_outside_the_buffers_and_repeats_are_bit_identical(D, B, T, K, grid):
    """Through the C ABI with buffers of our own: guard zones around h, the per-patient counters, the status word, the
    workspace and every gradient stay as they were, and a second forward + backward gives the same bits everywhere."""
    from hode import _dopri5_pp_lib as PL, _lib as L
    dev = _dev()
    if grid is None:
        inp, f = cases.setup({"B": B, "T": T, "D": D, "K": K, "ablate": False, "hill": "two", "seed": 70 + D})
    else:  # several h rows per step, steps without one, three doses inside grid steps
        inp, f = cases.setup(cases._grid_case(grid, D, B, K))
        assert inp["t"].numel() == T
    y0, theta, w, b, t, dosage, times = _device_args(inp, f, dev)
    lib = PL.lib()
    M, steps = D - 4, 16 * T + 64
    cot = torch.randn(T, B, D, generator=torch.Generator().manual_seed(8)).to(dev)
    snaps = []
    for _ in range(2):
        d = PL.new_desc()
        d.rhs_kind, d.batch, d.latent_dim, d.n_times, d.n_dose, d.max_steps = L.RHS_ROCHE, B, D, T, K, steps
        d.need_theta_grad, d.rtol, d.atol = 1, RTOL, ATOL
        d.t, d.y0, d.dosage, d.dose_times, d.theta = t.data_ptr(), y0.data_ptr(), dosage.data_ptr(), times.data_ptr(), theta.data_ptr()
        d.w1, d.b1 = (w.data_ptr(), b.data_ptr()) if M else (0, 0)
        nbytes = lib.hode_dopri5_pp_workspace_bytes(d)
        f32 = {"h": T * B * D, "grad_y0": B * D, "grad_w1": max(M * D, 1), "grad_b1": max(M, 1), "grad_theta": 16}
        i32 = {"status": 1, "n_accepted": B, "n_rejected": B, "patient_status": B}
        bufs = {k: _Guarded(n, torch.float32, dev, 7.5) for k, n in f32.items()}
        bufs.update({k: _Guarded(n, torch.int32, dev, -77) for k, n in i32.items()})
        bufs["workspace"] = _Guarded(nbytes // 4, torch.int32, dev, -77)
        for k in ("grad_w1", "grad_b1", "grad_theta") + tuple(i32):
            bufs[k].body.zero_()  # accumulators and the words the caller zeroes
        for k, g in bufs.items():
            if M or k not in ("grad_w1", "grad_b1"):
                setattr(d, k, g.ptr())
        d.workspace_bytes = nbytes
        d.grad_h = cot.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        PL.check(lib.hode_dopri5_pp_fwd(ctypes.byref(d), stream), "fwd")
        PL.check(lib.hode_dopri5_pp_bwd(ctypes.byref(d), stream), "bwd")
        torch.cuda.synchronize()
        assert int(bufs["status"].body[0]) == 0 and int(bufs["n_accepted"].body.min()) >= 1
        assert int(bufs["n_accepted"].body.max()) <= steps
        for k, g in bufs.items():
            assert g.intact(), k
        assert torch.isfinite(bufs["h"].body).all() and torch.isfinite(bufs["grad_y0"].body).all()
        assert not (bufs["h"].body == 7.5).any() and not (bufs["grad_y0"].body == 7.5).any()  # every element was written
        snaps.append({k: g.body.clone() for k, g in bufs.items() if k != "workspace"})
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], snaps[1][k]), k
    # and the launch functions give these bits too
    hip = _solve(inp, f, dev, cot.cpu())
    assert torch.equal(hip["h"].flatten(), snaps[0]["h"].cpu()) and torch.equal(hip["gy0"].flatten(), snaps[0]["grad_y0"].cpu())
    assert torch.equal(hip["gtheta"], snaps[0]["grad_theta"].cpu()[:13])
    if M:
        assert torch.equal(hip["gw"].flatten(), snaps[0]["grad_w1"].cpu()) and torch.equal(hip["gb"], snaps[0]["grad_b1"].cpu())


# ----------------------------------------------------------------------------------------------------- 7. status
def test_a_failing_patient_raises_and_is_named_while_the_others_finish():
    """The problem of test_dopri5_failure_is_a_runtime_error (a NaN in one patient's start state): HodeError, a
    RuntimeError, with the batch-global path's text and the patient's index; that patient's lane stops, the others' solves
    are complete.  A status path: nothing here hangs or faults."""
    import hode
    from hode import patient_dopri5 as PP
    dev = _dev()
    inp, f = cases.setup({"B": 6, "T": 8, "D": 8, "K": 1, "ablate": False, "hill": "two", "seed": 9})
    args = list(_device_args(inp, f, dev))
    args[0] = args[0].clone()
    args[0][2, 1] = float("nan")
    with pytest.raises(RuntimeError, match=r"non-finite values in state `y` \(first failing patient: 2\)") as info:
        PP.patient_dopri5_forward(*args, rtol=RTOL, atol=ATOL)
    assert isinstance(info.value, hode.HodeError)
    st = PP.last_stats
    assert st["status"].tolist() == [0, 0, 1, 0, 0, 0] and int(st["n_accepted"][2]) == 0
    good = _solve(inp, f, dev)
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(st["n_accepted"].cpu()[keep], good["n_acc"][keep]) and torch.equal(st["n_rejected"].cpu()[keep], good["n_rej"][keep])


def test_the_attempt_bound_ends_a_lane():
    """max_attempts is a bound of its own: with 2 attempts per patient no lane runs a third, the patients that needed more
    carry MAX_STEPS and the call raises `max_num_steps exceeded` (no retry: growing the tape would not help)."""
    import hode
    from hode import _lib as L, patient_dopri5 as PP
    dev = _dev()
    inp, f = cases.setup({"B": 70, "T": 8, "D": 8, "K": 1, "ablate": False, "hill": "two", "seed": 9})
    with pytest.raises(hode.HodeError, match=r"max_num_steps exceeded \(first failing patient: \d+\)"):
        PP.patient_dopri5_forward(*_device_args(inp, f, dev), rtol=RTOL, atol=ATOL, max_attempts=2)
    st = PP.last_stats
    assert int((st["n_accepted"] + st["n_rejected"]).max()) == 2 and st["max_steps"] == 16 * 8 + 64
    assert L.STATUS_MAX_STEPS in set(st["status"].tolist()) <= {0, L.STATUS_MAX_STEPS}
    # a tape of one row: the patients stop after their first accepted step and the solve is repeated with larger tapes
    grown = _solve(inp, f, dev, max_steps=1)
    assert grown["max_steps"] >= int(grown["n_acc"].max()) > 1 and not grown["status"].any()


# ------------------------------------------------------------------------------------------------ 8. model level
def _vi(obs, D, T, dev, seed=1, **kw):
    import model
    from hode import synth
    torch.manual_seed(seed)
    enc = model.EncoderLSTM(obs + 1, obs * 2, D, device=dev)
    dec = model.RocheExpertDecoder(obs, D, 1, (T - 1) * synth.STEP, synth.STEP, method="dopri5", device=dev)
    return model.VariationalInference(enc, dec, **(kw or {"elbo": False})), enc, dec


@pytest.mark.parametrize("obs,D", [(40, 6), (80, 12)])
def test_vi_loss_backward_with_patient_step_control(obs, D):
    """decoder.ode.step_control = "patient" is all a user sets: the loss is finite and every parameter the batch-global path
    gives a gradient gets one here too."""
    from hode import patient_dopri5 as PP, synth
    dev = _dev()
    T, B = 12, 21
    sol, ob = synth.solver_inputs(B, T, D, seed=3), synth.observation_inputs(B, T, obs, seed=3)
    data = {k: v.to(dev) for k, v in {"measurements": ob["measurements"], "actions": sol["actions"], "masks": ob["masks"]}.items()}
    grads = {}
    for control in ("batch", "patient"):
        vi, enc, dec = _vi(obs, D, T, dev)
        dec.ode.step_control = control
        PP.last_stats.clear()
        loss = vi.loss(data)
        loss.backward()
        assert torch.isfinite(loss)
        assert bool(PP.last_stats) == (control == "patient")
        grads[control] = {n: p.grad for n, p in list(enc.named_parameters()) + list(dec.named_parameters())}
    assert PP.last_stats["no_tape"] is False and PP.last_stats["n_accepted"].shape == (B,)
    for n, g in grads["batch"].items():
        gp = grads["patient"][n]
        assert (g is None) == (gp is None), n
        if g is not None:
            assert torch.isfinite(gp).all(), n
            assert bool(gp.any()) == bool(g.any()), n
    assert all(grads["patient"][n] is not None for n in ("ode.ml_net.0.weight", "ode.kel", "output_function.0.weight"))


@pytest.mark.parametrize("D", [6, 12])
def test_at_batch_one_both_controllers_give_the_same_trajectory(D):
    """With B = 1 the batch-global controller IS the patient's (the lane-per-patient layout on both sides: the same stage
    and error-norm expressions).  Two runs of one controller agree within the 1e-4 * scale of
    test_dopri5_forward_backward_vs_oracle whatever their accept / reject decisions, and with gradients within its 4e-2.
    Where both took the same step sequence (equal counts) the algebra is the same step for step: 2e-5 * scale, the bound
    of the replay comparison, and -- the batch side run with detach_first_step, dt_0's derivative being the one term
    per-patient mode does not form -- every gradient within 1e-4."""
    import hode
    import model
    from hode import adaptive, patient_dopri5 as PP, synth
    dev = _dev()
    T = 14
    sol = synth.solver_inputs(1, T, D, seed=21)
    torch.manual_seed(2)
    ode = model.RocheODE(D, 1, (T - 1) * synth.STEP, synth.STEP, device=dev)
    ode.set_action(sol["actions"].to(dev))
    t = sol["t"].to(dev)
    cot = torch.randn(T, 1, D, generator=torch.Generator().manual_seed(4)).to(dev)
    ya = sol["z0"].to(dev).requires_grad_(True)
    ha = hode.odeint(ode, ya, t, rtol=RTOL, atol=ATOL, method="dopri5", options={"step_control": "patient"})
    (ha * cot).sum().backward()
    gp = {n: p.grad.clone() for n, p in ode.named_parameters() if p.grad is not None}
    counts = (int(PP.last_stats["n_accepted"][0]), int(PP.last_stats["n_rejected"][0]))
    ode.zero_grad()
    yb = sol["z0"].to(dev).requires_grad_(True)
    hb = adaptive.roche_dopri5(yb, ode.theta_vector(), ode.ml_net[0].weight, ode.ml_net[0].bias, t, ode.dosage, ode.times, rtol=RTOL,
                               atol=ATOL, lanes_per_patient=1, detach_first_step=True)
    (hb * cot).sum().backward()
    same = counts == (adaptive.last_stats["n_accepted"], adaptive.last_stats["n_rejected"])
    scale = 1 + hb.detach().abs().max().item()
    err = (ha.detach() - hb.detach()).abs().max().item()
    print("counts %s vs %s, |h_patient - h_batch| = %.3e, rel grad_y0 %.3e" % (counts, (adaptive.last_stats["n_accepted"],
          adaptive.last_stats["n_rejected"]), err, _rel(ya.grad, yb.grad)))
    tol_h, tol_g = (2e-5, 1e-4) if same else (1e-4, 4e-2)
    assert err <= tol_h * scale
    assert _rel(ya.grad, yb.grad) <= tol_g
    for n, p in ode.named_parameters():
        if p.grad is not None and float(p.grad.abs().max()) > 1e-12:
            assert _rel(gp[n], p.grad) <= tol_g, (n, _rel(gp[n], p.grad))
    # the default route of hode.odeint is still the batch-global one
    PP.last_stats.clear()
    with torch.no_grad():
        hd = hode.odeint(ode, sol["z0"].to(dev), t, rtol=RTOL, atol=ATOL, method="dopri5")
    assert not PP.last_stats and adaptive.last_stats["no_tape"] is True and hd.shape == hb.shape


def test_evaluate_under_no_grad_runs_without_tapes(capsys):
    import training_utils
    from hode import patient_dopri5 as PP
    from hode.batches import DeviceFolds
    dev = _dev()
    T, obs, D = 12, 40, 6
    folds = DeviceFolds.synthetic(96, T, obs, D, 32, 32, dev, seed=4)
    import model
    vi, enc, dec = _vi(obs, D, T, dev, prior_log_pdf=model.ExponentialPrior.log_density)
    dec.ode.step_control = "patient"
    PP.last_stats.clear()
    out = training_utils.evaluate(vi, folds, 16, 6, mc_itr=4)
    assert len(out) == 6 and all(v == v for v in out)
    assert PP.last_stats["no_tape"] is True and PP.last_stats["workspace_bytes"] < 4096
    assert PP.last_stats["n_accepted"].shape[0] in (16, 4 * 16)  # the point estimate or the mc_itr * B draws
