"""The bindings of hode/ with the tensors a caller, and autograd itself, really hands them.  GPU only.

One test per (op, presentation) pair of tests/binding_cases.py.  Each runs the plain call (fresh, contiguous, fp32,
default stream, one backward) and the presented call, compares the presented call with the float64 reference at the
bounds the family's own test file uses (TOLERANCES; the numbers live in tests/reference_checks.py for both), and, for the ops in
binding_cases.DETERMINISTIC, with the plain call bit for bit: a presentation changes where the values sit in memory, not
the values, so for a deterministic kernel any difference is a bug.

A pointer audit is active in every test: each exported hode_* / hode_flow_* function of the loaded libraries is wrapped,
and a non-NULL device pointer in its descriptor that is not 16-byte aligned raises AssertionError before anything is
launched.  include/hode.h and include/hode_flow.h document no pointer as element-aligned, so ELEMENT_ALIGNED is empty."""
import ctypes

import pytest
import torch

import binding_cases as bc
import reference_checks as rc

pytestmark = pytest.mark.gpu

#: (descriptor type name, field) -> the header line that documents the field as element-aligned.  None exist.
ELEMENT_ALIGNED = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------- pointer audit
def _audited(name, real):
    def call(*args):
        for a in args:
            if isinstance(a, ctypes.Structure):
                for field, ftype in a._fields_:
                    v = getattr(a, field) if ftype is ctypes.c_void_p else None
                    if v and v % 16 and (type(a).__name__, field) not in ELEMENT_ALIGNED:
                        raise AssertionError("%s: %s.%s = %#x is not 16-byte aligned" % (name, type(a).__name__, field, v))
        return real(*args)
    return call


@pytest.fixture(autouse=True, scope="module")
def pointer_audit():
    if not torch.cuda.is_available():
        yield
        return
    from hode import _flow_lib as F
    from hode import _lib as L
    saved = []
    for mod in (L, F):
        handle = mod.lib()
        for name, _, _ in mod.EXPORTS:
            real = getattr(handle, name)
            saved.append((handle, name, real))
            setattr(handle, name, _audited(name, real))
    yield
    for handle, name, real in saved:
        setattr(handle, name, real)


# ---------------------------------------------------------------------------------------------------- tolerances
def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _check_traj(tol):
    def check(got, ref, what):
        err = (got.double() - ref).abs().max().item()
        assert err <= tol * (1 + ref.abs().max().item()), (what, err)
    return check


def _check_abs(tol):
    def check(got, ref, what):
        err = (got.double() - ref).abs().max().item()
        assert err <= tol, (what, err)
    return check


def _check_rel(tol):
    def check(got, ref, what):
        err = _rel(got, ref) if float(ref.abs().max()) > 0 else float(got.abs().max())
        assert err <= tol, (what, err)
    return check


def _flow_close(tol):
    return lambda got, ref, what: rc.close(got.cpu(), ref, tol, what)


_GRAD = _check_rel(rc.GRAD_TOL)
#: family -> (one check per output, the gradient check); the bounds are those of the family's own test file
#: (tests/reference_checks.py holds them for both).  None: per-element scales that need the inputs, see _check_*.
TOLERANCES = {
    "roche": ((_check_traj(rc.TRAJ_TOL),), _GRAD),
    "neural_dopri5": ((_check_traj(rc.NEURAL_DOPRI5_TRAJ_TOL),), _GRAD),
    "neural_real": ((_check_traj(rc.TRAJ_TOL),), _check_rel(rc.NEURAL_REAL_GRAD_TOL)),
    "lstm": ((_check_abs(rc.LSTM_H_TOL), _check_abs(rc.LSTM_C_TOL)), _GRAD),
    "readout": ((_check_rel(rc.READOUT_TOL),), _check_rel(rc.READOUT_TOL)),
    "readout_mlp": ((_check_rel(rc.READOUT_TOL),), _check_rel(rc.READOUT_MLP_GRAD_TOL)),
    "flow": ((_flow_close(rc.FLOW_TOL), _flow_close(rc.FLOW_TOL)), _flow_close(rc.FLOW_GTOL)),
    "mckl": None,
    "crps": None,
}


def _check_crps(got, ref, inputs):
    """The op's float64 reference at tests/test_hip_metric_cases.py's bound: CRPS_TOL of the element's own scale."""
    h = inputs["h"]
    Tn, MB, Dv = h.shape
    _, scale = rc.crps_oracle(h.view(Tn, bc.CRPS_MEMBERS, MB // bc.CRPS_MEMBERS, Dv), inputs["truth"], inputs["weight"], inputs["bias"])
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= rc.CRPS_TOL * scale).all()), float((err / scale).max())


def _check_mckl(outs, grads, r_outs, r_grads, inputs, cots, factor):
    """tests/test_hip_metric_cases.py test_mckl_case: per element MCKL_KL_TOL (kl) / MCKL_GRAD_TOL (gradients) plus the
    S-term sum error, of that element's own term magnitudes (mckl_scales); a gradient's scale is multiplied by the
    cotangent it was scaled with."""
    S = inputs["noise"].shape[0]
    s_kl, s_gmu, s_glv, _ = rc.mckl_scales(inputs["mu"].flatten(), inputs["log_var"].flatten(), inputs["noise"].reshape(S, -1),
                                           bc.MCKL_RATE, bc.MCKL_CLAMP)
    acc = rc.mckl_sum_error(S)
    rc.within(outs[0].cpu().flatten(), r_outs[0].flatten(), s_kl, rc.MCKL_KL_TOL + acc, "kl")
    c = cots[0].double().flatten().abs() * factor
    for k, scale in (("mu", s_gmu), ("log_var", s_glv)):
        if k in grads:
            rc.within(grads[k].cpu().flatten(), r_grads[k].flatten() * factor, scale * c, rc.MCKL_GRAD_TOL + acc, "grad_" + k)


# ------------------------------------------------------------------------------------------------------ the runs
def _cots(op, outs, pres, seed):
    """The cotangent each output effectively receives (CPU, fp32): ones under cot_sum, seeded normal draws otherwise."""
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.ones(o.shape) if pres == "cot_sum" else torch.randn(o.shape, generator=g) for o in outs]


def _requires(op, pres):
    if pres.startswith("one_grad["):
        return (op.diff[int(pres[9:-1])],)
    if pres == "no_grad_inputs":
        return ()
    if pres == "nondiff_requires_grad":
        return op.diff + op.nondiff
    return op.diff


def _leaves(op, tensors, req):
    out = {}
    for k, v in tensors.items():
        out[k] = v.detach().requires_grad_(True) if (v is not None and k in req) else v
    return out


def _loss(op, pres, leaves, outs, cots, dev):
    """sum(out * cot) with the output consumed the way the presentation says; the cotangent that reaches the binding has
    the values of `cots` in every case."""
    total = 0.0
    if pres == "cot_stack":        # two calls stacked: this one's share of the stack's gradient is a view at an offset
        other, _ = op.call({k: (v.detach() if v is not None else None) for k, v in leaves.items()})
    for n, (o, c) in enumerate(zip(outs, cots)):
        c = c.to(dev)
        if pres == "cot_stack":
            o2 = other[n]
            big = torch.stack([torch.randn_like(c), c])
            total = total + (torch.stack([o2.detach(), o]) * big).sum()
        elif pres == "cot_cat":    # one extra leading row
            o1 = o.reshape(1) if o.dim() == 0 else o
            c1 = c.reshape(1) if c.dim() == 0 else c
            row = torch.zeros_like(o1[:1])
            total = total + (torch.cat([row, o1]) * torch.cat([torch.randn_like(c1[:1]), c1])).sum()
        elif pres == "cot_sum":
            total = total + o.sum()
        elif pres == "cot_transpose":
            o2 = o if o.dim() >= 2 else o.reshape(1, -1)
            c2 = c if c.dim() >= 2 else c.reshape(1, -1)
            total = total + (o2.transpose(0, 1) * c2.transpose(0, 1).contiguous()).sum()
        elif pres == "cot_fp64":
            total = total + (o.double() * c.double()).sum()
        else:
            total = total + (o * c).sum()
    return total


def _run(op, pres, inputs, dev, seed, presented, cots=None):
    """One forward (+ backward) of `op`.  presented = False: the plain counterpart (same grad set, same cotangent values,
    fresh contiguous fp32 tensors, one backward).  Returns outs (detached), grads by input name, aux, cots, leaves."""
    req = _requires(op, pres)
    how = pres if presented else "plain"
    leaves = _leaves(op, {k: bc.present(op, how, k, v, dev) for k, v in inputs.items()}, req)
    if pres == "no_grad_mode":
        with torch.no_grad():
            outs, aux = op.call(leaves)
        assert not any(o.requires_grad for o in outs)
    else:
        outs, aux = op.call(leaves)
    if cots is None:
        cots = _cots(op, outs, pres, seed)
    grads = {}
    if req and pres != "no_grad_mode" and op.diff:
        loss = _loss(op, how, leaves, outs, cots, dev)
        if presented and pres == "twice":
            loss.backward(retain_graph=True)
            loss.backward(retain_graph=True)
        else:
            loss.backward()
        grads = {k: leaves[k].grad for k in req}
    elif pres == "no_grad_inputs":
        assert not any(o.requires_grad for o in outs)
    return [o.detach() for o in outs], grads, aux, cots, leaves


_REF = {}


def _reference(op, inputs, aux, cots, key):
    """float64 outputs and the gradients of sum(out * cot) for every differentiable input, cached per (op, inputs)."""
    if key not in _REF:
        i64 = {k: (v.double().requires_grad_(k in op.diff) if v is not None and v.is_floating_point() else v)
               for k, v in inputs.items()}
        outs = getattr(bc, op.ref)(i64, aux)
        grads = {}
        if op.diff:
            g = torch.autograd.grad(sum((o * c.double()).sum() for o, c in zip(outs, cots)), [i64[k] for k in op.diff],
                                    allow_unused=True)
            grads = {k: (torch.zeros_like(i64[k]) if x is None else x) for k, x in zip(op.diff, g)}
        _REF[key] = ([o.detach() for o in outs], grads)
    return _REF[key]


def _compare(op, pres, inputs, plain, got, seed, factor=1.0):
    outs, grads, aux, cots, leaves = got
    p_outs, p_grads = plain[0], plain[1]
    grads = {k: g for k, g in grads.items() if k in op.diff}
    r_outs, r_grads = _reference(op, inputs, plain[2], cots, (op.name, seed, pres == "expanded", pres == "cot_sum"))
    for o, r in zip(outs, r_outs):
        assert o.dtype == torch.float32 and o.shape == r.shape     # the output stays fp32 whatever the inputs were
    for k, g in grads.items():
        assert g is not None, k
        assert g.dtype == leaves[k].dtype and g.shape == leaves[k].shape, (k, g.dtype, g.shape)  # the input's own dtype
    if op.tol == "crps":
        _check_crps(outs[0], r_outs[0], inputs)
    elif op.tol == "mckl":
        _check_mckl(outs, grads, r_outs, r_grads, inputs, cots, factor)
    else:
        out_checks, grad_check = TOLERANCES[op.tol]
        for n, (o, r, chk) in enumerate(zip(outs, r_outs, out_checks)):
            chk(o.cpu(), r, "out%d" % n)
        for k, g in grads.items():
            grad_check(g.cpu(), r_grads[k] * factor, "grad_" + k)
    if op.name in bc.DETERMINISTIC:
        for n, (o, p) in enumerate(zip(outs, p_outs)):
            assert torch.equal(o, p), ("out%d differs from the plain call" % n, _rel(o, p))
        for k, g in grads.items():
            assert torch.equal(g.to(torch.float32), p_grads[k] * factor), ("grad_%s differs from the plain call" % k,
                                                                           _rel(g, p_grads[k] * factor))


QUEUED_MS_MIN = 5.0


def _queue_work(dev):
    """24 dependent 4096^3 fp32 matmuls queued on the current stream, between two events.  The delay is not tuned to a
    figure: 3.3 TFLOP cannot take less than ~20 ms at the card's fp32 matrix peak, and the side-stream test asserts
    afterwards that the events measured at least QUEUED_MS_MIN, so the case cannot quietly lose its delay."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a = torch.randn(4096, 4096, device=dev) / 64.0
    e0.record()
    for _ in range(24):
        a = (a @ a) / 64.0
    e1.record()
    return a, e0, e1


@pytest.mark.parametrize("name,pres", bc.pairs(), ids=lambda v: v)
def test_binding(name, pres):
    dev = _dev()
    op = bc.OPS[name]
    seed = 1
    inputs = bc.prepare(op, pres, op.build(seed))
    plain = _run(op, pres, inputs, dev, seed, presented=False)
    cots = plain[3]

    if pres == "interleaved":
        inputs_b = op.build(2)
        plain_b = _run(op, pres, inputs_b, dev, 2, presented=False)
        req = _requires(op, pres)
        la = _leaves(op, {k: bc.present(op, "plain", k, v, dev) for k, v in inputs.items()}, req)
        lb = _leaves(op, {k: bc.present(op, "plain", k, v, dev) for k, v in inputs_b.items()}, req)
        oa, aux_a = op.call(la)
        ob, aux_b = op.call(lb)
        _loss(op, "plain", la, oa, cots, dev).backward()
        _loss(op, "plain", lb, ob, plain_b[3], dev).backward()
        _compare(op, pres, inputs, plain, ([o.detach() for o in oa], {k: la[k].grad for k in req}, aux_a, cots, la), seed)
        _compare(op, pres, inputs_b, plain_b, ([o.detach() for o in ob], {k: lb[k].grad for k in req}, aux_b, plain_b[3], lb), 2)
        return

    if pres == "side_stream":
        staged = {k: bc.present(op, "plain", k, v, dev) for k, v in inputs.items()}
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            busy, e0, e1 = _queue_work(dev)
            # produced behind the queued work, on this stream: a binding that launched anywhere else would read them early
            made = {k: (v if v is None or not v.is_floating_point() else v * (1.0 + 0.0 * busy[0, 0])) for k, v in staged.items()}
            req = _requires(op, pres)
            leaves = _leaves(op, made, req)
            outs, aux = op.call(leaves)
            grads = {}
            if req:
                _loss(op, "plain", leaves, outs, cots, dev).backward()
                grads = {k: leaves[k].grad for k in req}
            host = ([o.detach().cpu() for o in outs], {k: g.cpu() for k, g in grads.items()})
        torch.cuda.synchronize()
        assert e0.elapsed_time(e1) >= QUEUED_MS_MIN, e0.elapsed_time(e1)
        got = ([o.to(dev) for o in host[0]], {k: g.to(dev) for k, g in host[1].items()}, aux, cots, leaves)
        _compare(op, pres, inputs, plain, got, seed)
        return

    if pres == "mutated":
        which, rule = op.mutated
        req = _requires(op, pres)
        leaves = _leaves(op, {k: bc.present(op, "plain", k, v, dev) for k, v in inputs.items()}, req)
        outs, aux = op.call(leaves)
        loss = _loss(op, "plain", leaves, outs, cots, dev)
        with torch.no_grad():
            leaves[which].add_(1.0)
        if rule == "raises":
            with pytest.raises(RuntimeError, match="modified by an inplace operation"):
                loss.backward()
        else:  # the binding formed its gradients during the forward: they are those of the forward-time values
            loss.backward()
            _compare(op, pres, inputs, plain, ([o.detach() for o in outs], {k: leaves[k].grad for k in req}, aux, cots, leaves), seed)
        return

    got = _run(op, pres, inputs, dev, seed, presented=True, cots=cots)
    if pres == "nondiff_requires_grad":
        for k in op.nondiff:
            assert got[4][k].requires_grad and got[4][k].grad is None, k   # no gradient: None, not zeros
    _compare(op, pres, inputs, plain, got, seed, factor=2.0 if pres == "twice" else 1.0)


@pytest.mark.parametrize("name", list(bc.OPS))
def test_plain_call_repeats(name, record_property):
    """Two plain runs of every op: equal bit for bit for the ops in DETERMINISTIC; measured and recorded for the others."""
    dev = _dev()
    op = bc.OPS[name]
    inputs = op.build(1)
    a = _run(op, "plain", inputs, dev, 1, presented=False)
    b = _run(op, "plain", inputs, dev, 1, presented=False)
    same = all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    record_property("plain_vs_plain_equal", same)
    print("plain-vs-plain %s: %s" % (name, "equal" if same else "DIFFERENT"))
    if name in bc.DETERMINISTIC:
        assert same
