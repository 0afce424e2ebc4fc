"""Failure reporting and patient isolation of the solver kernels with one patient poisoned (NaN, +inf, -inf).  GPU only.

The cases are tests/failure_cases.py's (tests/test_failure_cases.py holds them against the built kernel symbols and pins
the expected answer of a poisoned run to the float64 oracle):

* fixed grid: the status word of every Roche forward (rk_fwd_kernel, split_fwd_kernel, mf_fwd_kernel; libhode.so and
  libhode_roche_dims.so) through hode.roche_solve(check_finite=True) and through the descriptor -- exactly
  HODE_STATUS_NONFINITE after a poisoned run, 0 after a clean one and for patients that are merely unusual (y0 = 0, a
  subnormal y0, every dose after t[-1]), and a NULL status is accepted;
* isolation, bit for bit: a poisoned patient changes no other patient's trajectory, a poisoned cotangent no other patient's
  grad_y0 (taped and recomputing backward), and inputs that end right in front of NaN change nothing at all;
* the same isolation for the NeuralODE fixed-grid kernels (no status word there);
* the whole-batch dopri5 controllers (Roche, both layouts and both libraries; NeuralODE, both libraries): a non-finite start
  state, the step bound and its retry loop, dt underflow.  Every failing call passes max_steps <= 64, and the persistent
  attempt loop is not used;
* RocheODE.check_finite through hode.odeint, the sub-stepped solve and the dose-gradient route, and one restart of
  training_utils.variational_training_loop that the real kernel ends.

The only tolerance is TRAJ_TOL of tests/test_hip_kernel_variants.py, for the false-positive batch against the float64
oracle; everything else is torch.equal."""
import ctypes as C

import pytest
import torch

import failure_cases as fc
from reference_checks import TRAJ_TOL

pytestmark = pytest.mark.gpu

NONFINITE_TEXT = "non-finite values in state"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _opt(x, dev):
    return None if x is None else x.to(dev)


def _inputs(c, dev):
    """The case's clean inputs on the device (copies: the shared ones stay as they are)."""
    p = fc.setup(c)
    return {k: _opt(p[k], dev) for k in ("y0", "t", "dosage", "times", "theta", "w", "b", "cot")}


def _library(c):
    import hode
    return hode.roche_solver_library(c["D"]) if c["lib"] == "roche_dims" else None


def _solve(c, q, check_finite, **over):
    """hode.roche_solve on the case; a case with tape on hands y0 as a leaf, so that the forward leaves its stage tape
    (HODE_FLAG_TAPE: the taping instantiation of the split forward)."""
    import hode
    a = dict(q, **over)
    y0 = a["y0"].clone().requires_grad_(bool(c["tape"]))
    return hode.roche_solve(y0, a["theta"], a["w"], a["b"], a["t"], a["dosage"], a["times"], method=c["method"], ablate=c["ablate"],
                            lanes_per_patient=c["lanes"], check_finite=check_finite, library=_library(c)).detach()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _n_bad(x):
    return int((~torch.isfinite(x)).sum())


def _others(c, dev):
    keep = torch.ones(c["B"], dtype=torch.bool, device=dev)
    keep[c["row"]] = False
    return keep.nonzero().flatten()


# ------------------------------------------------------------------------------------------------- through the descriptor
class _Call:
    """hode_rk_fwd / hode_rk_bwd of the case's library through the descriptor, on exactly the tensors of `q` (no binding
    copies anything).  tape: the forward leaves its stage tape in the workspace and the backward reads it (HODE_FLAG_TAPE)."""

    def __init__(self, c, q, dev, tape=False, status=True):
        import hode
        from hode import _lib as L
        self.L, self.c, self.q = L, c, q
        self.lib = hode.roche_solver_library(c["D"]) if c["lib"] == "roche_dims" else L.lib()  # libhode.so holds D = 16 too (MFMA)
        B, D, T, K = c["B"], c["D"], c["T"], c["n_dose"]
        f32 = dict(device=dev, dtype=torch.float32)
        self.h = torch.full((T, B, D), -7.25, **f32)
        self.status = torch.zeros(1, device=dev, dtype=torch.int32) if status else None
        self.grad_h = torch.zeros((T, B, D), **f32)
        self.gy0 = torch.empty((B, D), **f32)
        self.gw = torch.empty((D - 4, D), **f32) if D > 4 else None
        self.gb = torch.empty((D - 4,), **f32) if D > 4 else None
        self.gth = torch.zeros(L.N_THETA, **f32)
        for k in ("y0", "t", "dosage", "theta") + (("times",) if K else ()) + (("w", "b") if D > 4 else ()):
            assert q[k].is_contiguous() and q[k].dtype == torch.float32 and q[k].data_ptr() % 16 == 0, k
        d = L.new_solve_desc()
        d.rhs_kind = L.RHS_ROCHE_ABLATE if c["ablate"] else L.RHS_ROCHE
        d.method, d.perturb, d.batch, d.latent_dim, d.n_times, d.n_dose = L.METHODS[c["method"]], 0, B, D, T, K
        d.lanes_per_patient, d.need_theta_grad = c["lanes"], 1
        d.t, d.y0, d.dosage, d.theta = q["t"].data_ptr(), q["y0"].data_ptr(), q["dosage"].data_ptr(), q["theta"].data_ptr()
        d.dose_times = q["times"].data_ptr() if K else 0
        d.w1, d.b1 = (q["w"].data_ptr(), q["b"].data_ptr()) if D > 4 else (0, 0)
        d.h = self.h.data_ptr()
        d.status = self.status.data_ptr() if status else 0
        d.grad_h, d.grad_y0, d.grad_theta = self.grad_h.data_ptr(), self.gy0.data_ptr(), self.gth.data_ptr()
        d.grad_w1, d.grad_b1 = (self.gw.data_ptr(), self.gb.data_ptr()) if D > 4 else (0, 0)
        self.tape_flag = L.FLAG_TAPE if tape else 0
        d.flags = L.FLAG_OVERWRITE_GRADS | self.tape_flag
        n = max(self.lib.hode_workspace_bytes(d, L.WS_RK_BWD), self.lib.hode_workspace_bytes(d, L.WS_RK_FWD))
        self.ws = torch.empty(max(n, 4), device=dev, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = self.ws.data_ptr(), n
        self.d = d

    def forward(self):
        """The return code of hode_rk_fwd, the status word (None without one) and h."""
        if self.status is not None:
            self.status.zero_()  # the caller zeroes the word: the kernels only ever OR into it
        self.d.flags = self.tape_flag
        code = self.lib.hode_rk_fwd(self.d, torch.cuda.current_stream().cuda_stream)
        self.L.check(code, "hode_rk_fwd")
        torch.cuda.synchronize()
        return code, (None if self.status is None else int(self.status)), self.h

    def backward(self, cot):
        """(grad_y0, [grad_w1, grad_b1,] grad_theta) of the cotangent on the states the last forward left in h."""
        self.grad_h.copy_(cot)
        self.d.flags = self.L.FLAG_OVERWRITE_GRADS | self.tape_flag
        self.L.check(self.lib.hode_rk_bwd(self.d, torch.cuda.current_stream().cuda_stream), "hode_rk_bwd")
        torch.cuda.synchronize()
        return [x.clone() for x in (self.gy0, self.gw, self.gb, self.gth) if x is not None]


def _tape_modes(c):
    return (True, False) if fc.has_both_backwards(c) else (bool(c["tape"]),)


PAD = 64  # floats either side of a fenced input: 256 bytes of NaN


def _guarded(x):
    if x is None or x.numel() == 0:
        return x
    buf = torch.full((x.numel() + 2 * PAD,), float("nan"), device=x.device, dtype=torch.float32)
    view = buf[PAD:PAD + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view  # keeps buf alive


def _check_binding(c, q, dev):
    """2. hode.roche_solve(check_finite=True): silent on the clean batch (the bits of the unchecked call) and on patients
    that are merely unusual (within TRAJ_TOL of the float64 oracle), HodeError on the poisoned one."""
    import hode
    plain = _solve(c, q, False)
    assert torch.equal(_solve(c, q, True), plain)
    assert torch.equal(plain[0], q["y0"]) and bool(torch.isfinite(plain).all())
    if c["B"] >= 5:
        y0, times = fc.quiet(c)
        h = _solve(c, q, True, y0=y0.to(dev), times=times.to(dev)).double().cpu()
        ref = fc.oracle(c, "quiet")
        err = (h - ref).abs().max().item()
        assert err <= TRAJ_TOL * (1 + ref.abs().max().item()), err
    with pytest.raises(hode.HodeError) as e:
        _solve(c, q, True, y0=fc.poisoned_y0(c).to(dev))
    assert NONFINITE_TEXT in str(e.value) and "fixed-grid" in str(e.value), str(e.value)
    return plain


def _check_adjoint(c, q, call, others, tape):
    """3. hode_rk_bwd on the clean states of `call` with grad_h[n, p, col] poisoned: grad_y0 of every other patient has the
    bits of the clean run and grad_y0[p] is non-finite.  A cotangent at n >= 1 passes through at least one step, so the
    patient's contribution to the parameter gradients is non-finite too (it was summed, not dropped; at D = 4 that gradient
    is grad_theta).  The cotangent of the first output time enters after the last step of the sweep and reaches grad_y0[p]
    alone: there the parameter gradients keep the bits of the clean run."""
    clean = call.backward(q["cot"])
    # finite, but for d / d HillCure with a negative Immunity: x ** p * log(x) is NaN in the float64 oracle as well
    # (tests/test_hip_kernel_variants.py::_ref_finite)
    assert all(bool(torch.isfinite(g).all()) for g in clean[:-1]), tape
    assert bool(torch.isfinite(clean[-1][2 if c.get("neg_imm") else 0:]).all()), tape
    got = call.backward(fc.poisoned_cot(c).to(q["cot"].device))
    assert torch.equal(got[0][others], clean[0][others]), tape
    assert not bool(torch.isfinite(got[0][c["row"]]).all()), tape
    if c["n"] >= 1:
        assert sum(_n_bad(g) for g in got[1:]) > sum(_n_bad(g) for g in clean[1:]), tape
        if c["D"] == 4:
            assert _n_bad(got[-1]) > _n_bad(clean[-1])
    else:
        assert all(torch.equal(_bits(g), _bits(k)) for g, k in zip(got[1:], clean[1:])), tape


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_a_poisoned_patient(c):
    """One case of the table, sections 2 and 3 of the file's docstring: the binding's check, then through the descriptor
    (taped and recomputing where the layout has both) the exact status word, NULL status, forward and adjoint isolation
    and the fenced inputs.  One test per case, so that the case's inputs reach the device once."""
    from hode import _lib as L
    dev = _dev()
    q = _inputs(c, dev)
    plain = _check_binding(c, q, dev)
    bad = dict(q, y0=fc.poisoned_y0(c).to(dev))
    # y0, dosage, dose_times, t, theta, w1 and b1 each inside a larger buffer of NaN: a read past a ragged last wave, past
    # t[T - 1] or past a row that reaches arithmetic turns h or the status word
    fenced = dict(q, **{k: _guarded(q[k]) for k in ("y0", "dosage", "times", "t", "theta", "w", "b")})
    others, p = _others(c, dev), c["row"]
    for tape in _tape_modes(c):
        call = _Call(c, q, dev, tape)
        code, word, clean = call.forward()
        assert (code, word) == (0, 0) and torch.equal(clean, plain), (tape, code, word)  # exactly 0 after a clean run
        _check_adjoint(c, q, call, others, tape)
        code, word, h = _Call(c, bad, dev, tape).forward()
        assert code == 0 and word == L.STATUS_NONFINITE, (tape, code, word)  # exactly the one bit
        # isolation: every other patient has the bits of the clean run, at every output time
        assert torch.equal(h[:, others], clean[:, others]), tape
        assert not bool(torch.isfinite(h[-1, p]).all()), tape
        # status = NULL ("may be NULL"): the same call returns 0 and writes the same h
        code, word, h_null = _Call(c, bad, dev, tape, status=False).forward()
        assert code == 0 and word is None and torch.equal(_bits(h_null), _bits(h)), tape
        code, word, h = _Call(c, fenced, dev, tape).forward()
        assert (code, word) == (0, 0) and torch.equal(h, clean), tape


# ------------------------------------------------------------------------------------- NeuralODE fixed grid: isolation
@pytest.mark.parametrize("c", fc.NEURAL_CASES, ids=fc.neural_case_id)
def test_neural_fixed_grid_isolation(c):
    from hode.neural import neural_solve
    dev = _dev()
    p = fc.neural_problem(c["D"], c["B"], c["T"], seed=700 + c["D"])
    lanes = 1 if c["layout"] == "lane-per-patient" else 0
    prm = [x.to(dev).requires_grad_(True) for x in p["prm"]]
    t, dosage, times, cot = (p[k].to(dev) for k in ("t", "dosage", "times", "cot"))
    row, value = c["row"], fc.VALUE_NAMES[c["value"]]
    keep = torch.ones(c["B"], dtype=torch.bool, device=dev)
    keep[row] = False

    def run(y0, cot):
        y0 = y0.clone().requires_grad_(True)
        h = neural_solve(y0, *prm, t, dosage, times, method=c["method"], lanes_per_patient=lanes)
        grads = torch.autograd.grad(h, [y0] + prm, grad_outputs=cot)
        torch.cuda.synchronize()
        return h.detach(), grads

    y0 = p["y0"].to(dev)
    h, g = run(y0, cot)
    assert bool(torch.isfinite(h).all()) and all(bool(torch.isfinite(x).all()) for x in g)
    y0_bad = y0.clone()
    y0_bad[row, c["col"]] = value
    h_bad, _ = run(y0_bad, cot)
    assert torch.equal(h_bad[:, keep], h[:, keep]) and not bool(torch.isfinite(h_bad[-1, row]).all())
    cot_bad = cot.clone()
    cot_bad[c["n"], row, c["col"]] = value
    _, g_bad = run(y0, cot_bad)
    assert torch.equal(g_bad[0][keep], g[0][keep]) and not bool(torch.isfinite(g_bad[0][row]).all())
    if c["n"] >= 1:
        assert any(not bool(torch.isfinite(x).all()) for x in g_bad[1:])
    else:  # the cotangent of t[0] enters after the last step of the sweep: it reaches grad_y0[p] alone
        assert all(torch.equal(x, k) for x, k in zip(g_bad[1:], g[1:]))


# ------------------------------------------------------------------------------------------------ 4. whole-batch dopri5
MAX_STEPS = 64  # every failing call: the host's attempt bound 64 * (max_steps + 64) is then a few thousand launches
DP_TEXT = "hode dopri5: non-finite values in state `y`"
DP_ROCHE = [dict(D=4, lanes=1, ablate=False), dict(D=4, lanes=1, ablate=True), dict(D=8, lanes=1, ablate=True),
            dict(D=8, lanes=4, ablate=False), dict(D=12, lanes=4, ablate=True), dict(D=12, lanes=1, ablate=False),
            dict(D=16, lanes=4, ablate=False), dict(D=10, lanes=1, ablate=True)]  # 16 and 10: libhode_roche_dims.so
DP_NEURAL = [4, 14, 15]  # 15: libhode_neural_odd.so


def _dp_id(c):
    return "D%d-l%d%s" % (c["D"], c["lanes"], "-ablate" if c["ablate"] else "")


def _roche_dopri5(p, dev, c, rtol=1e-7, atol=1e-8, max_steps=MAX_STEPS, grad=False, **over):
    import hode
    from hode import adaptive
    a = {k: _opt(v, dev) for k, v in dict(p, **over).items() if k != "f"}
    y0 = a["y0"].clone().requires_grad_(grad)
    return adaptive.roche_dopri5(y0, a["theta"], a["w"], a["b"], a["t"], a["dosage"], a["times"], rtol=rtol, atol=atol,
                                 ablate=c["ablate"], lanes_per_patient=c["lanes"], max_steps=max_steps,
                                 library=hode.roche_solver_library(c["D"])).detach()


def _neural_dopri5(p, dev, rtol=1e-7, atol=1e-8, max_steps=MAX_STEPS, grad=False, **over):
    from hode import adaptive
    a = dict(p, **over)
    y0 = a["y0"].to(dev).clone().requires_grad_(grad)
    return adaptive.neural_dopri5(y0, *[x.to(dev) for x in a["prm"]], a["t"].to(dev), a["dosage"].to(dev), a["times"].to(dev),
                                  rtol=rtol, atol=atol, max_steps=max_steps).detach()


def _start_states(p):
    """(row, value) at both ends of the batch, NaN and inf alternating; column by row."""
    B, D = p["y0"].shape
    for i, (row, value) in enumerate(((0, float("nan")), (B - 1, float("inf")), (0, float("-inf")), (B - 1, float("nan")))):
        y0 = p["y0"].clone()
        y0[row, (1, 3, D - 1, 0)[i]] = value
        yield row, value, y0


@pytest.mark.parametrize("c", DP_ROCHE, ids=_dp_id)
def test_roche_dopri5_non_finite_start_state(c):
    import hode
    from hode import adaptive
    dev = _dev()
    for B in (5, 50):
        p = fc.roche_problem(c["D"], B, 8, seed=600 + c["D"], ablate=c["ablate"])
        for row, value, y0 in _start_states(p):
            adaptive.last_stats.update(n_accepted=-1)
            with pytest.raises(hode.HodeError) as e:
                _roche_dopri5(p, dev, c, y0=y0)
            assert str(e.value) == DP_TEXT, (B, row, value, str(e.value))
            assert adaptive.last_stats["n_accepted"] == 0, (B, row, value)
        adaptive.last_stats.update(n_accepted=-1)
        assert bool(torch.isfinite(_roche_dopri5(p, dev, c)).all()) and adaptive.last_stats["n_accepted"] > 0  # the clean batch solves
    p = fc.roche_problem(c["D"], 5, 1, seed=600 + c["D"], ablate=c["ablate"])  # one output time: no step, the state is still refused
    for row, value, y0 in _start_states(p):
        adaptive.last_stats.update(n_accepted=-1)
        with pytest.raises(hode.HodeError) as e:
            _roche_dopri5(p, dev, c, y0=y0)
        assert str(e.value) == DP_TEXT and adaptive.last_stats["n_accepted"] == 0, (row, value, str(e.value))
    assert torch.equal(_roche_dopri5(p, dev, c)[0], p["y0"].to(dev))


@pytest.mark.parametrize("D", DP_NEURAL)
def test_neural_dopri5_non_finite_start_state(D):
    import hode
    from hode import adaptive
    dev = _dev()
    for B in (5, 50):
        p = fc.neural_problem(D, B, 8, seed=620 + D)
        for row, value, y0 in _start_states(p):
            adaptive.last_stats.update(n_accepted=-1)
            with pytest.raises(hode.HodeError) as e:
                _neural_dopri5(p, dev, y0=y0)
            assert str(e.value) == DP_TEXT, (B, row, value, str(e.value))
            assert adaptive.last_stats["n_accepted"] == 0, (B, row, value)
        adaptive.last_stats.update(n_accepted=-1)
        assert bool(torch.isfinite(_neural_dopri5(p, dev)).all()) and adaptive.last_stats["n_accepted"] > 0  # the clean batch solves
    p = fc.neural_problem(D, 5, 1, seed=620 + D)  # one output time: no step, the state is still refused
    for row, value, y0 in _start_states(p):
        adaptive.last_stats.update(n_accepted=-1)
        with pytest.raises(hode.HodeError) as e:
            _neural_dopri5(p, dev, y0=y0)
        assert str(e.value) == DP_TEXT and adaptive.last_stats["n_accepted"] == 0, (row, value, str(e.value))
    assert torch.equal(_neural_dopri5(p, dev)[0], p["y0"].to(dev))


def _dopri5_descriptor(c, p, dev, rtol, atol, max_steps):
    """hode_dopri5_fwd through the descriptor as hode.adaptive fills it (no tape kept: HODE_FLAG_NO_TAPE).  Returns the
    return code, the status word the caller zeroed, and the accepted / rejected counts."""
    import hode
    from hode import _lib as L
    from hode._neural_odd_lib import neural_solver_library
    neural = c["family"] == "neural"
    lib = neural_solver_library(c["D"]) if neural else hode.roche_solver_library(c["D"])
    keep = {k: _opt(v, dev) for k, v in p.items() if k in ("y0", "t", "dosage", "times", "theta", "w", "b")}
    keep["prm"] = [x.to(dev) for x in p.get("prm", ())]
    B, D = p["y0"].shape
    T = p["t"].numel()
    h = torch.empty((T, B, D), device=dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    n_acc, n_rej = C.c_int32(-1), C.c_int32(-1)
    d = L.new_solve_desc()
    d.rhs_kind = L.RHS_NEURAL if neural else (L.RHS_ROCHE_ABLATE if c.get("ablate") else L.RHS_ROCHE)
    d.batch, d.latent_dim, d.n_times, d.n_dose, d.lanes_per_patient = B, D, T, keep["times"].shape[1], c["lanes"]
    d.t, d.y0, d.dosage, d.dose_times = (keep[k].data_ptr() for k in ("t", "y0", "dosage", "times"))
    if neural:
        d.hidden_dim = keep["prm"][0].shape[0]
        d.w1, d.b1, d.w2, d.b2 = (x.data_ptr() for x in keep["prm"])
    else:
        d.theta = keep["theta"].data_ptr()
        d.w1, d.b1 = (keep["w"].data_ptr(), keep["b"].data_ptr()) if D > 4 else (0, 0)
    d.h, d.status = h.data_ptr(), status.data_ptr()
    d.rtol, d.atol, d.max_steps, d.flags = rtol, atol, max_steps, L.FLAG_NO_TAPE
    d.host_n_accepted, d.host_n_rejected = C.pointer(n_acc), C.pointer(n_rej)
    n = lib.hode_workspace_bytes(d, L.WS_DOPRI5_FWD)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    code = lib.hode_dopri5_fwd(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    # the two controller records (csrc/hode_dopri5_kernels.hpp DpCtrl: t0, dt as doubles, h0, d1 as floats, then n_acc,
    # n_rej, j_next, done, status, attempt) open the workspace, double-buffered by attempt parity: `attempt` of the later
    # one is the number of attempt launches that did any work
    words = ws[:96].cpu().view(torch.int32).view(2, 12)
    return code, int(status), n_acc.value, n_rej.value, int(words[:, 11].max())


DP_BOUND = [dict(family="roche", D=8, lanes=1), dict(family="roche", D=8, lanes=4), dict(family="roche", D=16, lanes=4),
            dict(family="neural", D=8, lanes=0), dict(family="neural", D=15, lanes=0)]


def _problem(c, B, T, seed):
    return (fc.neural_problem if c["family"] == "neural" else fc.roche_problem)(c["D"], B, T, seed=seed)


@pytest.mark.parametrize("c", DP_BOUND, ids=lambda c: "%s-D%d-l%d" % (c["family"], c["D"], c["lanes"]))
def test_dopri5_step_bound(c):
    """max_steps = 2 on a T = 8 problem that needs more.  Through the descriptor: return value 0, status exactly
    HODE_STATUS_MAX_STEPS, two accepted steps.  Through the binding: the retry loop (steps *= 4) ends, and h and n_accepted
    have the bits of the solve with max_steps = 64 and of the default bound, without and with a tape to grow:
    the trajectory does not depend on the tape size."""
    from hode import _lib as L
    from hode import adaptive
    dev = _dev()
    p = _problem(c, 5, 8, seed=640 + c["D"])
    code, word, n_acc, n_rej, attempts = _dopri5_descriptor(c, p, dev, 1e-7, 1e-8, 2)
    assert (code, word, n_acc) == (0, L.STATUS_MAX_STEPS, 2) and attempts == n_acc + n_rej + 1
    solve = (lambda **kw: _neural_dopri5(p, dev, **kw)) if c["family"] == "neural" else (lambda **kw: _roche_dopri5(p, dev, dict(c, ablate=False), **kw))
    for grad in (False, True):
        runs = []
        for max_steps in (2, MAX_STEPS, 0):
            adaptive.last_stats.update(n_accepted=-1)
            h = solve(max_steps=max_steps, grad=grad)
            runs.append((h, adaptive.last_stats["n_accepted"], adaptive.last_stats["n_rejected"]))
        assert runs[0][1] > 2 and bool(torch.isfinite(runs[0][0]).all())  # the retry loop grew the bound and ended
        for h, n_acc, n_rej in runs[1:]:
            assert torch.equal(h, runs[0][0]) and (n_acc, n_rej) == runs[0][1:], grad


@pytest.mark.parametrize("c", fc.UNDERFLOW_CASES, ids=fc.underflow_id)
def test_dopri5_dt_underflow(c):
    """The constructions tests/test_failure_cases.py fixed with the eager restatement: a finite start state on which the
    controller gives up on dt.  The status word is exactly HODE_STATUS_DT_UNDERFLOW (the state is not flagged), the error
    says `underflow in dt`, and the attempts are bounded."""
    import hode
    from hode import _lib as L
    from hode import adaptive
    dev = _dev()
    p, rtol, atol = fc.underflow_problem(c)
    assert bool(torch.isfinite(p["y0"]).all())
    code, word, n_acc, n_rej, attempts = _dopri5_descriptor(c, p, dev, rtol, atol, MAX_STEPS)
    assert code == 0 and word & L.STATUS_DT_UNDERFLOW and not word & L.STATUS_NONFINITE, (code, word)
    # bounded: the controller gave up at attempt 0, on dt_0 itself (the eager restatement's bound is 200 attempts)
    assert (n_acc, n_rej, attempts) == (0, 0, 1), (n_acc, n_rej, attempts)
    adaptive.last_stats.update(n_accepted=-1, n_rejected=-1)
    with pytest.raises(hode.HodeError) as e:
        if c["family"] == "neural":
            _neural_dopri5(p, dev, rtol=rtol, atol=atol)
        else:
            _roche_dopri5(p, dev, dict(c, ablate=False), rtol=rtol, atol=atol)
    assert str(e.value) == "hode dopri5: underflow in dt", str(e.value)
    assert (adaptive.last_stats["n_accepted"], adaptive.last_stats["n_rejected"]) == (0, 0)


# ------------------------------------------------------------------------------------------------------- 5. model level
def _decoder(dev, D=8, T=12, B=9, method="rk4"):
    import model
    from hode import synth
    torch.manual_seed(5)
    dec = model.RocheExpertDecoder(5, D, 1, (T - 1) * synth.STEP, synth.STEP, method=method, device=dev)
    inp = synth.solver_inputs(B, T, D, seed=9)
    z0 = inp["z0"].to(dev)
    z0[B - 1, 1] = float("nan")
    return dec, z0, inp["actions"].to(dev)


@pytest.mark.parametrize("route", ["odeint", "step_size", "dose_grad"])
def test_rocheode_check_finite(route):
    import hode
    dev = _dev()
    dec, z0, a = _decoder(dev)
    ode = dec.ode
    options = {"step_size": dec.step_size / 2} if route == "step_size" else {}
    if route == "dose_grad":
        ode.dose_grad = True
        a = a.clone().requires_grad_(True)

    def solve():
        ode.set_action(a)
        return hode.odeint(ode, z0, dec.t, method="midpoint" if route == "step_size" else "rk4", options=dict(options))

    assert ode.check_finite is False
    h = solve()  # the flag off: a non-finite h comes back and nothing is raised
    assert not bool(torch.isfinite(h[-1, -1]).all()) and bool(torch.isfinite(h[:, :-1]).all())
    ode.check_finite = True
    with pytest.raises(hode.HodeError, match=NONFINITE_TEXT):
        solve()
    good = z0.clone()
    good[-1, 1] = 0.01
    ode.set_action(a)
    assert bool(torch.isfinite(hode.odeint(ode, good, dec.t, method="rk4", options=dict(options))).all())


def test_the_training_loop_ends_a_restart_on_the_kernels_own_error(tmp_path, capsys):
    """tests/test_host_logic.py shows the loop's handling with a model that raises by hand; here model.loss runs the
    decoder, and the error is the fixed-grid kernel's status word."""
    import training_utils
    dev = _dev()
    dec, z0, a = _decoder(dev)

    class _Gen:
        train_size = val_size = 9

        def get_mini_batch(self, fold, n):
            return {"z0": z0, "actions": a}

        get_split = get_mini_batch

    class _Model:
        model_name = "m"

        def __init__(self):
            self.encoder, self.decoder, self.calls, self.saved = torch.nn.Linear(1, 1), dec, 0, 0

        def loss(self, data):
            self.calls += 1
            x_hat, _ = self.decoder(data["z0"], data["actions"])
            return (x_hat ** 2).mean()

        def save(self, path, itr, best):
            self.saved += 1
            torch.save({"encoder_state_dict": self.encoder.state_dict(), "decoder_state_dict": self.decoder.state_dict(),
                        "best_loss": best}, path + self.model_name)

    opt = torch.optim.SGD(dec.parameters(), lr=0.0)
    dec.ode.check_finite = True
    m = _Model()
    training_utils.variational_training_loop(3, _Gen(), m, 9, opt, 5, path=str(tmp_path) + "/")
    assert (m.calls, m.saved) == (1, 1)  # the first loss raised, the restart ended, the untrained model was checkpointed
    assert NONFINITE_TEXT in capsys.readouterr().out
    dec.ode.check_finite = False  # unchecked, the same data trains on: every iteration reaches the kernel
    m = _Model()
    training_utils.variational_training_loop(3, _Gen(), m, 9, opt, 5, path=str(tmp_path) + "/")
    assert m.calls == 3 and NONFINITE_TEXT not in capsys.readouterr().out
