"""The all-steps LSTM kernels of libhode_lstm_seq.so (lstm_seq_fwd_kernel / lstm_seq_bwd_kernel) on the GPU, over the case
table tests/lstm_seq_cases.py: every row of h and the final c against ``torch.nn.LSTM`` in float64 on the masked inputs
(reference_checks.LSTM_H_TOL / LSTM_C_TOL, absolute); the last processed row and the gradients of a last-row cotangent
against libhode.so's final-state kernels bit for bit; parameter gradients against float64 autograd (rel-L2 <= 1e-4, the
bound of tests/test_hip_lstm.py); sentinels around every output; the library's refusals; ``model.LSTMBaseline`` and
``model.EncoderLSTMReal(output_all=True)`` against float64 and against the reference's fixture G17.  GPU only."""
import numpy as np
import pytest
import torch

import lstm_seq_cases as cases
import reference_checks as rc

pytestmark = pytest.mark.gpu

NAMES = ("w_ih", "w_hh", "b_ih", "b_hh")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_PROBLEMS = {}


def _problem(c):
    """Seeded weights (nn.LSTM's init, scaled by 1.5 so that the gates leave their linear range), inputs, a cotangent on
    every row -- and the float64 reference, computed once per case and shared by the tests that need it."""
    key = cases.case_id(c) + str(c["tape"])
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    T, B, obs, H, ad = c["T"], c["B"], c["obs"], c["H"], 1 if c["a"] else 0
    gen = torch.Generator().manual_seed(1000 * H + 10 * obs + B + T)
    torch.manual_seed(H + obs + T)
    lstm = torch.nn.LSTM(obs + ad, H)
    with torch.no_grad():
        for prm in lstm.parameters():
            prm.mul_(1.5)
    x = torch.randn(T, B, obs, generator=gen)
    a = torch.rand(T, B, 1, generator=gen) * (torch.rand(T, B, 1, generator=gen) < 0.3).float() if ad else None
    m = (torch.rand(T, B, obs, generator=gen) < 0.5).float() if c["mask"] else None
    cot = torch.randn(T, B, H, generator=gen)
    w = [p.detach().clone() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
    out = dict(x=x, a=a, m=m, w=w, cot=cot)
    _PROBLEMS[key] = out
    return out


def _ref(c, p, cot=None):
    """float64 nn.LSTM on the masked inputs; rows in input order whichever way the window is walked.  With `cot`: also the
    four parameter gradients of sum(h * cot)."""
    T, obs, H = c["T"], c["obs"], c["H"]
    ref = torch.nn.LSTM(p["w"][0].shape[1], H).double()
    with torch.no_grad():
        for q, v in zip((ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0), p["w"]):
            q.copy_(v.double())
    xm = p["x"].double() * (p["m"].double() if p["m"] is not None else 1.0)
    seq = torch.cat([xm, p["a"].double()], dim=-1) if p["a"] is not None else xm
    out, (_, cn) = ref(seq.flip(0) if c["reverse"] else seq)
    h = out.flip(0) if c["reverse"] else out
    if cot is None:
        return h.detach(), cn[0].detach()
    (h * cot.double()).sum().backward()
    return h.detach(), cn[0].detach(), [q.grad for q in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)]


def _to(p, dev):
    g = lambda v: None if v is None else v.to(dev)   # noqa: E731
    return g(p["x"]), g(p["a"]), g(p["m"]), [v.to(dev) for v in p["w"]]


def _entry_fwd(x, a, m, w, reverse, nt, tape, h=None):
    """hode_lstm_seq_fwd through the C entry: (h_all, c, workspace, descriptor)."""
    from hode import _lstm_seq_lib as SL
    from hode.lstm import _desc
    lib = SL.lib()
    T, B, H = x.shape[0], x.shape[1], w[1].shape[1]
    h = torch.full((T, B, H), float("nan"), device=x.device) if h is None else h
    c = torch.full((B, H), float("nan"), device=x.device)
    d = _desc(x, a, m, *w, reverse, tape)
    d.patient_tiles, d.h_out, d.c_out = nt, h.data_ptr(), c.data_ptr()
    n = lib.hode_lstm_seq_workspace_bytes(d)
    assert n > 0
    ws = torch.empty(n, device=x.device, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    SL.check(lib.hode_lstm_seq_fwd(d, torch.cuda.current_stream().cuda_stream), "hode_lstm_seq_fwd")
    torch.cuda.synchronize()
    return h, c, ws, d


def _rel(got, want):
    return float((got.detach().cpu().double() - want.double()).norm() / want.double().norm())


# ------------------------------------------------------------------------------------------------ forward vs float64
@pytest.mark.parametrize("c", cases.FWD_CASES + cases.BWD_CASES, ids=cases.case_id)
def test_every_row_and_the_final_cell_state_match_float64(c):
    _rows_and_cell_state_match_float64(c, _dev())


@pytest.mark.parametrize("tpw", cases.TPWS)
def test_every_row_and_the_final_cell_state_match_float64_with_the_other_hidden_size(tpw):
    """PAD_FWD_CASES: the forward cases of one padded size again with the other H of each (padded units on / off)."""
    dev = _dev()
    mine = [c for c in cases.PAD_FWD_CASES if -(-c["H"] // 16) == tpw]
    assert len(mine) == 8
    for c in mine:
        print("case", cases.case_id(c))
        _rows_and_cell_state_match_float64(c, dev)


def _rows_and_cell_state_match_float64(c, dev):
    p = _problem(c)
    h_ref, c_ref = _ref(c, p)
    x, a, m, w = _to(p, dev)
    h, cn, _, _ = _entry_fwd(x, a, m, w, c["reverse"], c["nt"], c["tape"])
    eh = (h.cpu().double() - h_ref).abs().amax(dim=(1, 2))
    ec = (cn.cpu().double() - c_ref).abs().max().item()
    print("max |h - h64| per row", eh.tolist(), "max |c - c64|", ec)
    assert not torch.isnan(h).any() and not torch.isnan(cn).any()
    assert eh.max().item() <= rc.LSTM_H_TOL and ec <= rc.LSTM_C_TOL


# ------------------------------------------------------------------------------------- differential, no tolerance
@pytest.mark.parametrize("c", cases.DIFF_CASES, ids=cases.case_id)
def test_the_last_processed_row_is_the_final_state_kernel_s_bit_for_bit(c):
    from hode.lstm import lstm_encode, lstm_final_state, lstm_sequence
    dev = _dev()
    p = _problem(c)
    x, a, m, w = _to(p, dev)
    last = 0 if c["reverse"] else c["T"] - 1
    h_all, cn, _, _ = _entry_fwd(x, a, m, w, c["reverse"], c["nt"], False)
    h_fin, c_fin = lstm_final_state(x, a, m, *w, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    assert torch.equal(h_all[last], h_fin) and torch.equal(cn, c_fin)
    # a cotangent that is zero except on the last processed row: the four gradients are lstm_encode's
    cot = torch.zeros_like(p["cot"])
    cot[last] = p["cot"][last]
    ws = [v.clone().requires_grad_(True) for v in w]
    hs = lstm_sequence(x, a, m, *ws, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    assert torch.equal(hs.detach(), h_all)
    (hs * cot.to(dev)).sum().backward()
    we = [v.clone().requires_grad_(True) for v in w]
    he = lstm_encode(x, a, m, *we, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    (he * cot[last].to(dev)).sum().backward()
    for n, q, r in zip(NAMES, ws, we):
        assert torch.equal(q.grad, r.grad), (n, (q.grad - r.grad).abs().max().item())


# ------------------------------------------------------------------------------------- backward vs float64 autograd
def _check_grads(c, p, cot, dev):
    from hode.lstm import lstm_sequence
    h_ref, _, g_ref = _ref(c, p, cot)
    x, a, m, w = _to(p, dev)
    ws = [v.clone().requires_grad_(True) for v in w]
    xg = x.clone().requires_grad_(True)
    h = lstm_sequence(xg, a, m, *ws, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    assert h.shape == (c["T"], c["B"], c["H"])
    assert (h.detach().cpu().double() - h_ref).abs().max().item() <= rc.LSTM_H_TOL
    (h * cot.to(dev)).sum().backward()
    assert xg.grad is None
    errs = {n: _rel(q.grad, r) for n, q, r in zip(NAMES, ws, g_ref)}
    print("rel-L2 of the parameter gradients", errs)
    assert max(errs.values()) <= cases.GRAD_TOL, errs


@pytest.mark.parametrize("c", cases.BWD_CASES, ids=cases.case_id)
def test_parameter_gradients_of_a_cotangent_on_every_row_match_float64(c):
    p = _problem(c)
    _check_grads(c, p, p["cot"], _dev())


@pytest.mark.parametrize("c", cases.MIDDLE_CASES, ids=cases.case_id)
def test_a_cotangent_on_one_middle_row_is_added_at_its_step(c):
    p = _problem(c)
    cot = torch.zeros_like(p["cot"])
    cot[c["row"]] = p["cot"][c["row"]]
    _check_grads(c, p, cot, _dev())


@pytest.mark.parametrize("how", ["all_but_the_last_row", "sum"])
def test_the_cotangents_autograd_really_hands_over(how):
    """h[:-1] reaches the backward as a zero-padded contiguous tensor, h.sum() as an expanded one (stride 0)."""
    from hode.lstm import lstm_sequence
    dev = _dev()
    c = cases.AUTOGRAD_CASE
    p = _problem(c)
    cot = p["cot"].clone()
    if how == "sum":
        cot.fill_(1.0)
    else:
        cot[-1] = 0.0
    _, _, g_ref = _ref(c, p, cot)
    x, a, m, w = _to(p, dev)
    ws = [v.clone().requires_grad_(True) for v in w]
    h = lstm_sequence(x, a, m, *ws, reverse=bool(c["reverse"]), patient_tiles=c["nt"])
    (h.sum() if how == "sum" else (h[:-1] * p["cot"][:-1].to(dev)).sum()).backward()
    errs = {n: _rel(q.grad, r) for n, q, r in zip(NAMES, ws, g_ref)}
    assert max(errs.values()) <= cases.GRAD_TOL, errs


def test_no_tape_is_written_when_nothing_needs_a_gradient():
    from hode import _lstm_seq_lib as SL
    from hode.lstm import lstm_sequence
    dev = _dev()
    c = cases.AUTOGRAD_CASE
    x, a, m, w = _to(_problem(c), dev)
    ws = [v.clone().requires_grad_(True) for v in w]
    seen = []
    side = SL.side_library()
    plain = side.hode_lstm_fwd
    side.hode_lstm_fwd = lambda d, s: (seen.append(int(d.save_tape)), plain(d, s))[1]
    try:
        h_grad = lstm_sequence(x, a, m, *ws)
        with torch.no_grad():
            h_none = lstm_sequence(x, a, m, *ws)
        h_const = lstm_sequence(x, a, m, *w)
    finally:
        side.hode_lstm_fwd = plain
    assert seen == [1, 0, 0]
    assert h_grad.requires_grad and not h_none.requires_grad and not h_const.requires_grad
    assert torch.equal(h_grad.detach(), h_none) and torch.equal(h_none, h_const)


# -------------------------------------------------------------------------------------------------------- sentinels
def test_nothing_outside_the_outputs_is_written():
    """h_all, grad_gates and h_prev each inside a larger buffer of NaNs (B = 21, H = 13): every element of the output is
    written, nothing around it changes."""
    from hode import _lstm_seq_lib as SL
    dev = _dev()
    c = cases.SENTINEL_CASE
    p = _problem(c)
    x, a, m, w = _to(p, dev)
    T, B, H, obs = c["T"], c["B"], c["H"], c["obs"]
    W = (obs + 1 + H + 1 + 3) // 4 * 4
    pad = 256   # floats on either side: 1 KiB, keeps the 16-byte alignment
    nan = float("nan")
    big_h, big_g, big_p = (torch.full((2 * pad + n,), nan, device=dev) for n in (T * B * H, T * B * 4 * H, T * B * W))
    h = big_h[pad:pad + T * B * H].view(T, B, H)
    h, cn, ws, d = _entry_fwd(x, a, m, w, c["reverse"], c["nt"], True, h=h)
    gh = p["cot"].to(dev)
    dg, hp = big_g[pad:pad + T * B * 4 * H].view(T, B, 4 * H), big_p[pad:pad + T * B * W].view(T, B, W)
    d.grad_h_out, d.grad_gates, d.h_prev = gh.data_ptr(), dg.data_ptr(), hp.data_ptr()
    lib, s = SL.lib(), torch.cuda.current_stream().cuda_stream
    SL.check(lib.hode_lstm_seq_fill_operand(d, s), "hode_lstm_seq_fill_operand")
    SL.check(lib.hode_lstm_seq_bwd(d, s), "hode_lstm_seq_bwd")
    torch.cuda.synchronize()
    for name, big, n in (("h_all", big_h, T * B * H), ("grad_gates", big_g, T * B * 4 * H), ("h_prev", big_p, T * B * W)):
        assert torch.isnan(big[:pad]).all() and torch.isnan(big[pad + n:]).all(), name
        assert not torch.isnan(big[pad:pad + n]).any(), name
    assert not torch.isnan(cn).any()
    h_ref, _ = _ref(c, p)
    assert (h.cpu().double() - h_ref).abs().max().item() <= rc.LSTM_H_TOL
    assert torch.equal(hp[..., :obs], x * m) and torch.equal(hp[..., obs:obs + 1], a)
    assert torch.equal(hp[..., obs + 1 + H], torch.ones(T, B, device=dev)) and not hp[..., obs + 2 + H:].any()


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    import hode
    from hode import _lstm_seq_lib as SL
    from hode.lstm import _desc, lstm_sequence
    dev = _dev()
    lib, s = SL.lib(), torch.cuda.current_stream().cuda_stream
    T, B, obs = 3, 21, 20
    x = torch.randn(T, B, obs, device=dev)
    nan = float("nan")
    # hidden_dim 161
    w = [torch.zeros(4 * 161, obs, device=dev), torch.zeros(4 * 161, 161, device=dev), torch.zeros(4 * 161, device=dev), torch.zeros(4 * 161, device=dev)]
    with pytest.raises(hode.HodeConfigError, match="hidden_dim 161 exceeds the largest compiled kernel"):
        lstm_sequence(x, None, None, *w)
    # a workspace one byte short, a NULL grad_h_out
    H = 13
    w = [torch.randn(4 * H, obs, device=dev) * 0.3, torch.randn(4 * H, H, device=dev) * 0.3, torch.zeros(4 * H, device=dev), torch.zeros(4 * H, device=dev)]
    h, c = torch.full((T, B, H), nan, device=dev), torch.full((B, H), nan, device=dev)
    d = _desc(x, None, None, *w, False, True)
    d.h_out, d.c_out = h.data_ptr(), c.data_ptr()
    n = lib.hode_lstm_seq_workspace_bytes(d)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n - 1
    assert lib.hode_lstm_seq_fwd(d, s) == -4 and b"workspace %d B < required %d B" % (n - 1, n) in lib.hode_lstm_seq_last_error_string()
    d.workspace_bytes = n
    dg, hp = torch.full((T, B, 4 * H), nan, device=dev), torch.full((T, B, 36), nan, device=dev)
    d.grad_gates, d.h_prev, d.grad_h_out = dg.data_ptr(), hp.data_ptr(), None
    assert lib.hode_lstm_seq_bwd(d, s) == -1 and b"grad_h_out / grad_gates / h_prev must be non-NULL" in lib.hode_lstm_seq_last_error_string()
    torch.cuda.synchronize()
    for buf in (h, c, dg, hp):
        assert torch.isnan(buf).all()   # nothing ran


# ------------------------------------------------------------------------------------------------------ model level
def _model_batch(gen, T, B, obs, action, statics):
    return {"measurements": torch.randn(T, B, obs, generator=gen), "actions": (torch.rand(T, B, action, generator=gen) < 0.3).float(),
            "masks": (torch.rand(T, B, obs, generator=gen) < 0.7).float(),
            "statics": torch.randn(1, B, statics, generator=gen).expand(T, B, statics).contiguous()}


def test_lstm_baseline_loss_and_gradients_match_float64_and_adam_lowers_the_loss():
    import model
    dev = _dev()
    s = cases.MODEL_SHAPE
    data = _model_batch(torch.Generator().manual_seed(77), s["T"], s["B"], s["obs"], s["action"], s["statics"])
    torch.manual_seed(7)
    ref = model.LSTMBaseline(s["obs"] + s["action"] + s["statics"], s["H"], s["obs"], device=torch.device("cpu"))
    base = model.LSTMBaseline(s["obs"] + s["action"] + s["statics"], s["H"], s["obs"], device=dev)
    base.load_state_dict(ref.state_dict())
    ref = ref.double()
    want = ref.loss({k: v.double() for k, v in data.items()})
    want.backward()
    ddev = {k: v.to(dev) for k, v in data.items()}
    loss = base.loss(ddev)
    loss.backward()
    assert abs(loss.item() - want.item()) <= 2e-5 * abs(want.item()), (loss.item(), want.item())
    for (n, q), (_, r) in zip(base.named_parameters(), ref.named_parameters()):
        assert _rel(q.grad, r.grad) <= cases.GRAD_TOL, (n, _rel(q.grad, r.grad))
    assert all(v.grad is None for v in ddev.values())
    opt = torch.optim.Adam(base.parameters(), lr=1e-2)
    first = loss.item()
    for _ in range(2):
        opt.step()
        opt.zero_grad()
        loss = base.loss(ddev)
        loss.backward()
    assert loss.item() < first, (first, loss.item())


def test_the_reference_s_fixture_on_the_device(golden_dir):
    import os
    import test_lstm_baseline as tb
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g17_lstm_seq.npz"), allow_pickle=False)
    tb.check_baseline(g, dev)
    for reverse in (False, True):
        tb.check_encoder(g, reverse, dev)


def test_a_hidden_size_above_160_is_refused_by_the_model():
    import hode
    import model
    dev = _dev()
    base = model.LSTMBaseline(8, 161, 6, device=dev)
    with pytest.raises(hode.HodeConfigError, match="hidden_dim 161"):
        base(torch.zeros(3, 4, 6, device=dev), torch.zeros(3, 4, 2, device=dev), torch.ones(3, 4, 6, device=dev))
