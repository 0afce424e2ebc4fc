"""Patient isolation of the real-data and recurrent kernels with one value of one patient poisoned (NaN, +inf, -inf).  GPU only.

None of these kernels reports anything (no status word): a non-finite value is silent, and what a caller can rely on is
that it stays inside the patient it came from.  The cases are tests/isolation_cases.py's (tests/test_isolation_cases.py
holds them against the built kernel symbols and pins the expected answer of a poisoned run to each family's float64
reference).  Three cases of a family to a test (the table is long); each case's inputs reach the device once:

a. the clean run is finite (the LSTM, which runs through the descriptor for its cell state and gate cotangents, has the
   bits of its binding call);
b. forward: with one input entry poisoned, every other patient has the BITS of the clean run in every output, at every
   output time; the poisoned patient is non-finite in exactly the output rows in which the float64 reference is, and
   where the reference is finite -- a SATURATING case, or the rows before the poison arrives -- within the family's own
   tolerance of it (LSTM 2e-5 on h, 5e-5 on c; the decoders 2e-5 (1 + max|h|));
c. adjoint, on the clean states with one cotangent entry poisoned: every other patient's own gradient (grad_y0,
   grad_init, the LSTM's gate cotangents) has the bits of the clean run, the poisoned patient's is non-finite, and the
   batch-summed parameter gradients are non-finite whenever a step lies between the cotangent and the inputs (the
   patient's term is summed, not dropped); a cotangent of the start state reaches grad_y0[p] alone and leaves the sums
   their bits (tests/test_hip_failures.py::_check_adjoint's rule; isolation_cases.cot_reaches); and with the clean
   cotangent on the POISONED states every other patient's own gradient still has the bits of the clean run;
d. fenced: every floating-point input inside a larger buffer with 64 floats of NaN on either side (16-byte alignment
   kept; the bindings hand such a view to the kernels as it is) gives the bits of the clean run: nothing past a ragged
   last wave, past row T - 1, past the last action row or past obs on the scalar staging path reaches arithmetic;
f. position: a patient solved alone (B = 1) and the same patient in rows 0, 15, 16 and 49 of a batch of 50 are the same
   bits, forward outputs and the patient's own gradient.

Dead lanes.  tlstm_bwd_kernel, gruode_bwd_kernel, real_mf_kernel and real_dims / real_step / neural_real give a lane past
the batch the data of patient B - 1 and multiply its cotangent by lv = 0.0f: a product, not a select, so with patient
B - 1 poisoned the dead lanes carry NaN into the on-chip weight-gradient sums.  That is harmless: whatever a dead lane
carries is a copy of what patient B - 1's own live lane adds to the same sums, which are non-finite already and have to
be; the per-patient stores of a dead lane are guarded by `live` (a select).  The cases with row = B - 1 hold that: grad_y0
/ grad_init of every other patient keeps its bits, and with a cotangent of the start state (n = 0, reaches grad_y0[p]
alone) the sums keep theirs too.  The code stays as it is."""
import pytest
import torch

import isolation_cases as ic
from reference_checks import LSTM_C_TOL, LSTM_H_TOL, TRAJ_TOL
from test_hip_failures import _guarded

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _map(p, fn, every=False):
    """`fn` on every floating-point tensor of a problem (the weight lists too), on the index tables as well with `every`;
    modules are left out."""
    out = {}
    for k, v in p.items():
        if isinstance(v, torch.Tensor):
            out[k] = fn(v) if every or v.is_floating_point() else v
        elif isinstance(v, list):
            out[k] = [fn(x) for x in v]
    return out


def _on_device(c, dev):
    """The case's clean inputs on the device (copies: the shared ones stay as they are)."""
    return _map(ic.setup(c), lambda v: v.to(dev), every=True)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _n_bad(xs):
    return sum(int((~torch.isfinite(x)).sum()) for x in xs)


def _leaf(x):
    return x.detach().requires_grad_(True)   # the same memory: a fenced view stays the fenced view


# ----------------------------------------------------------------------------------------------------- the families
# run(c, q, cot) -> dict(out = forward outputs by name, pp = the patients' own gradients by name, summed = the batch sums);
# cot = None: forward only.  Patients sit on the axis isolation_cases.out_axis names.
def _run_real(c, q, cot):
    from hode import _lib as L
    from hode.real import _desc, contract_tape, real_solve
    from hode.real_step import real_step_solve
    y0, theta, wflat = _leaf(q["y0"]), _leaf(q["theta"]), _leaf(q["wflat"])
    if c["family"] == "real_step":
        h = real_step_solve(y0, theta, wflat, q["t"], q["act"], c["H"], method=c["method"], perturb=c["perturb"],
                            step_size=1.0 / c["S"], intervals_per_wave=c["C"])
    else:
        h = real_solve(y0, theta, wflat, q["t"], q["act"], c["H"], method=c["method"], perturb=c["perturb"])
    out = dict(out=dict(h=h.detach()))
    if cot is None:
        torch.cuda.synchronize()
        return out
    if c["onchip"]:
        gy0, gth, gw = torch.autograd.grad(h, [y0, theta, wflat], grad_outputs=cot)
    else:
        # the matrix-core backward without grad_w1 (C ABI): it writes the GEMM operand tape instead of folding on chip
        import hode
        lib, hd = hode.lib(), h.detach()
        gy0, gth = torch.empty_like(q["y0"]), torch.zeros(L.N_THETA, device=hd.device)
        d = _desc(hd[0], q["t"], q["act"], q["theta"], q["wflat"], hd, L.METHODS[c["method"]], c["perturb"], c["H"])
        assert cot.is_contiguous() and cot.data_ptr() % 16 == 0
        d.grad_h, d.grad_y0, d.grad_theta = cot.data_ptr(), gy0.data_ptr(), gth.data_ptr()
        n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
        ws = torch.empty(max(n, 4), device=hd.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        L.check(lib.hode_rk_bwd(d, torch.cuda.current_stream().cuda_stream), "hode_rk_bwd[real, tape]")
        gw, gth = contract_tape(ws, c["T"], c["B"], c["D"], c["H"], L.METHODS[c["method"]]), gth[:3].clone()
    torch.cuda.synchronize()
    return dict(out, pp=dict(grad_y0=gy0), summed=[gw, gth])


def _run_neural_real(c, q, cot):
    from hode import neural_real as nr
    y0, w = _leaf(q["y0"]), [_leaf(x) for x in q["w"]]
    h = nr._NeuralRealFixedGrid.apply(y0, *w, q["t"], q["dose"], nr.KINDS[c["kind"]], c["method"])
    out = dict(out=dict(h=h.detach()))
    if cot is not None:
        g = torch.autograd.grad(h, [y0] + w, grad_outputs=cot)
        out.update(pp=dict(grad_y0=g[0]), summed=list(g[1:]))
    torch.cuda.synchronize()
    return out


def _run_seqdec(c, q, cot):
    from hode import seqdec
    init, w = _leaf(q["init"]), [_leaf(x) for x in q["w"]]
    fn = seqdec.tlstm if c["kind"] == "tlstm" else seqdec.gruode
    h = fn(init, q["a"], q["idx"], q["tau"], ic.TA_SEQDEC - 1, *w)
    out = dict(out=dict(h=h.detach()))
    if cot is not None:
        g = torch.autograd.grad(h, [init] + w, grad_outputs=cot)
        out.update(pp=dict(grad_y0=g[0]), summed=list(g[1:]))
    torch.cuda.synchronize()
    return out


def _run_lstm(c, q, cot):
    """hode_lstm_fwd / _bwd / _fill_operand of the case's library through the descriptor -- h, the final c and, per
    patient, the gate cotangents grad_gates (T, B, 4H) -- and the four parameter gradients through the binding."""
    from hode import _lib as L
    from hode import _lstm_seq_lib as SL
    from hode import lstm as hl
    seq = c["lib"] == "seq"
    lib, s = SL.lstm_library(seq), torch.cuda.current_stream().cuda_stream
    x, a, m, w = q["x"], q["a"], q["m"], q["w"]
    T, B, H, dev = c["T"], c["B"], c["H"], x.device
    for v in [x, a, m] + list(w):
        assert v.is_contiguous() and v.dtype == torch.float32 and v.data_ptr() % 16 == 0
    h = torch.full((T, B, H) if seq else (B, H), -7.25, device=dev)
    cn = torch.full((B, H), -7.25, device=dev)
    d = hl._desc(x, a, m, *w, bool(c["reverse"]), c["tape"])
    d.patient_tiles, d.h_out, d.c_out = c["nt"], h.data_ptr(), cn.data_ptr()
    n = lib.hode_lstm_workspace_bytes(d)
    assert n > 0
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    L.check(lib.hode_lstm_fwd(d, s), "hode_lstm_fwd")
    torch.cuda.synchronize()
    out = dict(out=dict(h=h, c=cn))
    if cot is None:
        return out
    assert cot.is_contiguous() and cot.data_ptr() % 16 == 0
    W = (c["obs"] + 1 + H + 1 + 3) // 4 * 4
    dg, hp = torch.full((T, B, 4 * H), -7.25, device=dev), torch.full((T, B, W), -7.25, device=dev)
    d.grad_h_out, d.grad_gates, d.h_prev = cot.data_ptr(), dg.data_ptr(), hp.data_ptr()
    L.check(lib.hode_lstm_fill_operand(d, s), "hode_lstm_fill_operand")
    L.check(lib.hode_lstm_bwd(d, s), "hode_lstm_bwd")
    torch.cuda.synchronize()
    wl = [_leaf(v) for v in w]
    hb = (hl.lstm_sequence if seq else hl.lstm_encode)(x, a, m, *wl, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    assert _same(hb.detach(), h)   # the binding's forward: the same bits
    grads = torch.autograd.grad(hb, wl, grad_outputs=cot)
    torch.cuda.synchronize()
    return dict(out, pp=dict(grad_gates=dg, h_prev=hp), summed=list(grads))


RUN = {"real": _run_real, "real_dims": _run_real, "real_step": _run_real, "neural_real": _run_neural_real, "seqdec": _run_seqdec,
       "lstm": _run_lstm}


def _pp_axis(c, name):
    return 1 if name in ("grad_gates", "h_prev") else ic.out_axis(c, "grad_y0")


def _tolerance(c, name, ref):
    if c["family"] == "lstm":
        return LSTM_C_TOL if name == "c" else LSTM_H_TOL
    return TRAJ_TOL * (1 + ref[torch.isfinite(ref)].abs().max().item())   # the decoders' trajectory bound


def _others(c, dev):
    keep = torch.ones(c["B"], dtype=torch.bool, device=dev)
    keep[c["row"]] = False
    return keep.nonzero().flatten()


def _check_forward(c, clean, bad, others):
    """b (and e): isolation bit for bit; the poisoned patient against the float64 reference on the same poisoned inputs."""
    ref = ic.reference(c, ic.poisoned(c))
    for k, v in bad["out"].items():
        ax = ic.out_axis(c, k)
        assert _same(v.index_select(ax, others), clean["out"][k].index_select(ax, others)), k
        got, want = v.select(ax, c["row"]).double().cpu(), ref[k].select(ax, c["row"])
        if got.dim() == 1:
            got, want = got[None], want[None]
        got_bad, want_bad = ~torch.isfinite(got).all(dim=-1), ~torch.isfinite(want).all(dim=-1)
        print(k, "non-finite rows of the poisoned patient:", got_bad.tolist(), "reference:", want_bad.tolist())
        assert torch.equal(got_bad, want_bad), (k, got_bad.tolist(), want_bad.tolist())
        if bool((~want_bad).any()):
            err = (got[~want_bad] - want[~want_bad]).abs().max().item()
            print(k, "finite rows: max |got - float64| = %.3e (bound %.3e)" % (err, _tolerance(c, k, ref[k])))
            assert err <= _tolerance(c, k, ref[k]), (k, err)
    if c in ic.SATURATING:
        assert _n_bad(bad["out"].values()) == 0


def _check_adjoint(c, clean, got, others):
    reaches = ic.cot_reaches(c)
    for k, g in got["pp"].items():
        ax = _pp_axis(c, k)
        assert _same(g.index_select(ax, others), clean["pp"][k].index_select(ax, others)), k
        if k != "h_prev":   # the LSTM's GEMM operand rows hold inputs and states, no cotangent
            assert bool(torch.isfinite(g.select(ax, c["row"])).all()) == (reaches == "nothing"), k
    if reaches == "steps":
        assert _n_bad(got["summed"]) > 0   # summed, not dropped
        if c["family"] == "lstm":
            assert all(_n_bad([g]) > 0 for g in got["summed"])
    else:
        assert all(_same(a, b) for a, b in zip(got["summed"], clean["summed"]))


def _check_adjoint_of_poisoned_states(c, clean, bad, others):
    """The clean cotangent through the poisoned states: every other patient's own gradient still has the bits of the clean
    run.  Where the forward saturates, the poisoned patient's own gradient is finite exactly when the float64 reference's
    is (tlstm: the saturated gates pass an exact zero back, grad_init stays finite; gruode: dz = (W_n^T dn) x z (1 - z) is
    inf * 0 in the reference too).  The parameter gradients of such a patient are 0 * inf = NaN in the reference as well."""
    for k, g in bad["pp"].items():
        ax = _pp_axis(c, k)
        assert _same(g.index_select(ax, others), clean["pp"][k].index_select(ax, others)), k
    if c in ic.SATURATING and c["family"] != "lstm":
        ref = ic.reference(c, ic.poisoned(c), ic.setup(c)["cot"])
        ax = _pp_axis(c, "grad_y0")
        want = bool(torch.isfinite(ref["pp"].select(ax, c["row"])).all())
        assert bool(torch.isfinite(bad["pp"]["grad_y0"].select(ax, c["row"])).all()) == want, want


def _groups(cases, n=3):
    """Consecutive cases of one family, n to a test: the table is long, and the suite's test count stays moderate."""
    out = []
    for c in cases:
        if out and len(out[-1]) < n and out[-1][0]["family"] == c["family"] and out[-1][0].get("lib") == c.get("lib"):
            out[-1].append(c)
        else:
            out.append([c])
    return out


def _group_id(g):
    return ic.case_id(g[0]) + ("+%d" % (len(g) - 1) if len(g) > 1 else "")


@pytest.mark.parametrize("group", _groups(ic.CASES) + _groups(ic.SATURATING), ids=_group_id)
def test_a_poisoned_patient_stays_alone(group):
    """Every case of the group in turn (its id is printed first: a failure's captured output names the case)."""
    dev = _dev()
    for c in group:
        print("case", ic.case_id(c))
        _a_poisoned_patient_stays_alone(c, dev)


def _a_poisoned_patient_stays_alone(c, dev):
    run = RUN[c["family"]]
    q = _on_device(c, dev)
    has_cot = c["family"] != "lstm" or c["tape"]   # NT = 4 has no tape: forward only
    clean = run(c, q, q["cot"] if has_cot else None)
    assert _n_bad(clean["out"].values()) == 0
    others = _others(c, dev)
    key, idx = ic.forward_target(c)
    bad = run(c, dict(q, **{key: ic.poisoned(c)[key].to(dev)}), q["cot"] if has_cot else None)
    _check_forward(c, clean, bad, others)
    if has_cot:
        _check_adjoint_of_poisoned_states(c, clean, bad, others)
    fenced = _map(q, _guarded)
    got = run(c, fenced, fenced["cot"] if has_cot else None)
    assert all(_same(got["out"][k], v) for k, v in clean["out"].items())
    if has_cot:
        assert _n_bad(clean["pp"].values()) + _n_bad(clean["summed"]) == 0
        assert all(_same(got["pp"][k], v) for k, v in clean["pp"].items())
        assert all(_same(a, b) for a, b in zip(got["summed"], clean["summed"]))
        _check_adjoint(c, clean, run(c, q, ic.poisoned_cot(c).to(dev)), others)


# ------------------------------------------------------------------------------------------------------------ readouts
def _run_readout(c, q):
    from hode import readout as ro
    import kernel_variants as kv
    h, w = _leaf(q["h"]), [_leaf(x) for x in q["w"]]
    if c["family"] == "readout":
        fn = lambda hh, ww: ro.masked_sse_readout(hh, q["x"], q["m"], *ww, variant=kv.READOUT_VARIANT_VALU if c["valu"] else 0)   # noqa: E731
    else:
        fn = lambda hh, ww: ro.masked_sse_readout_mlp(hh, q["x"], q["m"], *ww)   # noqa: E731
    lik = fn(h, w)
    g = torch.autograd.grad(lik, [h] + w)
    with torch.no_grad():
        lik0 = fn(h.detach(), [x.detach() for x in w])   # the GRAD = false instantiation
    torch.cuda.synchronize()
    return dict(lik=lik.detach().reshape(1), lik0=lik0.reshape(1), grad_h=g[0], summed=list(g[1:]))


@pytest.mark.parametrize("group", _groups(ic.READOUT_CASES), ids=_group_id)
def test_a_poisoned_readout_row_stays_alone(group):
    """The loss and the parameter gradients are sums over every (time, patient) row: non-finite, from both instantiations;
    grad_h keeps the bits of the clean run in every other row and is non-finite in the poisoned one.  A NaN behind mask 0
    stays a NaN, as in the reference: (x - x_hat)^2 * mask is a product.  Fenced inputs give the clean bits."""
    dev = _dev()
    for c in group:
        print("case", ic.case_id(c))
        _a_poisoned_readout_row_stays_alone(c, dev)


def _a_poisoned_readout_row_stays_alone(c, dev):
    q = _on_device(c, dev)
    clean = _run_readout(c, q)
    assert _n_bad([clean["lik"], clean["lik0"], clean["grad_h"]] + clean["summed"]) == 0
    key, _ = ic.forward_target(c)
    bad = _run_readout(c, dict(q, **{key: ic.poisoned(c)[key].to(dev)}))
    assert not bool(torch.isfinite(bad["lik"])) and not bool(torch.isfinite(bad["lik0"]))
    assert all(_n_bad([g]) > 0 for g in bad["summed"])
    keep = torch.ones(c["T"], c["B"], dtype=torch.bool, device=dev)
    keep[c["n"], c["row"]] = False
    assert _same(bad["grad_h"][keep], clean["grad_h"][keep])
    assert not bool(torch.isfinite(bad["grad_h"][c["n"], c["row"]]).all())
    got = _run_readout(c, _map(q, _guarded))
    assert all(_same(got[k], clean[k]) for k in ("lik", "lik0", "grad_h")) and all(_same(a, b) for a, b in zip(got["summed"], clean["summed"]))


# ------------------------------------------------------------------------------------------------- position invariance
def _in_axes(c):
    """The patient axis of every per-patient input."""
    f = c["family"]
    if f in ("real", "real_dims", "real_step"):
        return dict(y0=1 if f == "real_step" else 0, act=1, cot=1)
    if f == "neural_real":
        return dict(y0=0, dose=1, cot=1)
    if f == "seqdec":
        return dict(init=0, a=1, cot=1)
    return dict(x=1, a=1, m=1, cot=1 if c["lib"] == "seq" else 0)


PATIENT = 7   # the row of the batch whose data the patient under test is


@pytest.mark.parametrize("group", _groups(ic.POSITION_CASES), ids=_group_id)
def test_a_patient_alone_is_the_same_patient_anywhere_in_the_batch(group):
    """f.  patient_tiles, intervals_per_wave and the layout are the case's in both calls: the same instantiation."""
    dev = _dev()
    for c in group:
        print("case", ic.case_id(c))
        _a_patient_alone(c, dev)


def _a_patient_alone(c, dev):
    run, axes = RUN[c["family"]], _in_axes(c)
    q = _on_device(c, dev)
    has_cot = c["family"] != "lstm" or c["tape"]
    one = dict(q, **{k: q[k].narrow(ax, PATIENT, 1).clone() for k, ax in axes.items() if q[k].numel()})   # a copy: 16-byte aligned
    alone = run(dict(c, B=1), one, one["cot"] if has_cot else None)
    for r in ic.POSITION_ROWS:
        moved = dict(q)
        for k, ax in axes.items():
            if q[k].numel():
                moved[k] = q[k].clone()
                moved[k].select(ax, r).copy_(q[k].select(ax, PATIENT))
        got = run(c, moved, moved["cot"] if has_cot else None)
        for k, v in alone["out"].items():
            ax = ic.out_axis(c, k)
            assert _same(got["out"][k].select(ax, r), v.select(ax, 0)), (r, k)
        for k, v in (alone["pp"] if has_cot else {}).items():
            ax = _pp_axis(c, k)
            assert _same(got["pp"][k].select(ax, r), v.select(ax, 0)), (r, k)


def _readout_grad_h(c, q, scale):
    """hode_readout_sse / hode_readout_mlp_sse through the descriptor with the gradient scale given (the bindings pass
    1 / B, which is another number for a patient alone): grad_h (T, B, D)."""
    import kernel_variants as kv
    from hode import _lib as L
    lib, mlp = L.lib(), c["family"] == "readout_mlp"
    h, x, m, w = q["h"], q["x"], q["m"], q["w"]
    T, B, D = h.shape
    d = L.ReadoutMlpDesc() if mlp else L.ReadoutDesc()
    d.struct_size = L.C.sizeof(type(d))
    d.latent_dim, d.obs_dim, d.scale, d.rows = D, x.shape[-1], scale, T * B
    d.h, d.x, d.mask = h.data_ptr(), x.data_ptr(), m.data_ptr()
    lik, gh = torch.empty(1, device=h.device), torch.full_like(h, -7.25)
    gw = [torch.zeros((v.numel() + 3) // 4 * 4, device=h.device) for v in w]   # every accumulator on a 16-byte boundary
    d.lik, d.grad_h = lik.data_ptr(), gh.data_ptr()
    if mlp:
        d.hidden_dim, d.batch = w[0].shape[0], B
        d.w1, d.b1, d.w2, d.b2 = (v.data_ptr() for v in w)
        d.grad_w1, d.grad_b1, d.grad_w2, d.grad_b2 = (v.data_ptr() for v in gw)
        size, entry, what = lib.hode_readout_mlp_workspace_bytes, lib.hode_readout_mlp_sse, "hode_readout_mlp_sse"
    else:
        d.variant = kv.READOUT_VARIANT_VALU if c["valu"] else 0
        d.w, d.b, d.grad_w, d.grad_b = w[0].data_ptr(), w[1].data_ptr(), gw[0].data_ptr(), gw[1].data_ptr()
        size, entry, what = lib.hode_readout_workspace_bytes, lib.hode_readout_sse, "hode_readout_sse"
    n = size(d)
    ws = torch.empty(max(n, 4), device=h.device, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    L.check(entry(d, torch.cuda.current_stream().cuda_stream), what)
    torch.cuda.synchronize()
    return gh


@pytest.mark.parametrize("c", ic.READOUT_POSITION_CASES, ids=ic.case_id)
def test_a_readout_patient_alone_has_the_same_grad_h_anywhere_in_the_batch(c):
    """f for the readouts: grad_h of a patient's T rows, alone (rows = T) and in rows 0, 15, 16 and 49 of the batch of 50,
    with the same gradient scale in both calls."""
    dev = _dev()
    q = _on_device(c, dev)
    scale = 1.0 / c["B"]
    one = dict(q, **{k: q[k][:, PATIENT:PATIENT + 1].clone() for k in ("h", "x", "m")})
    alone = _readout_grad_h(c, one, scale)
    assert _n_bad([alone]) == 0
    for r in ic.POSITION_ROWS:
        moved = dict(q, **{k: q[k].clone() for k in ("h", "x", "m")})
        for k in ("h", "x", "m"):
            moved[k][:, r] = q[k][:, PATIENT]
        assert _same(_readout_grad_h(c, moved, scale)[:, r], alone[:, 0]), r
