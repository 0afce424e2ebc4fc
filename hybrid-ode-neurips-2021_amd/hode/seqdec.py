"""Real-data recurrent baseline decoders (reference ``DecoderRealBenchmark``, ``model.py:889-966``) on the gfx950 kernels of
``csrc/hode_seqdec.hip``: one launch per direction instead of the reference's Python loop over the steps (one host sync,
then one ``nn.LSTM`` call or a handful of small eager ops per step).

``tlstm``: LSTM(2, D) with h0 = c0 = init; the forward tapes the cell state, the BPTT kernel recomputes the gates from it.
``gruode``: ``GRUODECell`` as the reference calls it -- the hidden state handed to the cell stays ``init`` at every step,
so every row is independent (no recurrence).  Both return gradients for ``init`` and every parameter; ``a``, ``idx`` and
``tau`` take none (their ``.grad`` stays None).  ``idx`` may be any integer tensor and ``tau`` any float tensor."""

from __future__ import annotations

import torch

from . import _lib as L
from .solver import _f32c, _i32c, _require_gpu, _stream


def step_tables(t, t_max, device):
    """(step_index int32 [T'], step_time fp32 [T'], largest index) as the reference forms them per step: the action row is
    ``int(t_k.item())`` and the time feature ``torch.ones_like(obs) * t / t_max`` in fp32.  Reads ``t`` back to the host:
    build once per grid and keep it (``DecoderRealBenchmark`` caches it per ``self.t``)."""
    rows = [int(v) for v in t.detach().cpu().tolist()]
    idx = torch.tensor(rows, dtype=torch.int32, device=device)
    tau = torch.ones(len(rows), device=device, dtype=torch.float32) * idx.to(torch.float32) / t_max
    return idx, tau, max(rows) if rows else -1


def _check(init, a, idx, max_row):
    B, D = init.shape
    if not 1 <= D <= L.SEQDEC_MAX_LATENT:
        raise L.HodeConfigError("hode: DecoderRealBenchmark kernels cover latent_dim 1..%d (got %d)" % (L.SEQDEC_MAX_LATENT, D))
    if a.dim() != 3 or a.shape[1] != B or a.shape[2] != 1:
        raise L.HodeConfigError("hode: DecoderRealBenchmark kernels take a (T, B, 1) action (got %s for batch %d)" % (tuple(a.shape), B))
    if idx.numel() == 0 or max_row >= a.shape[0] or max_row < 0:
        raise L.HodeConfigError("hode: decoder steps read action rows up to %d but a has %d rows" % (max_row, a.shape[0]))


def _desc(kind, init, a, idx, tau, w0, w1, b0, b1, h):
    B, D = init.shape
    d = L.SeqdecDesc()
    d.struct_size = L.C.sizeof(L.SeqdecDesc)
    d.kind, d.n_steps, d.n_action_times, d.batch, d.latent_dim, d.action_dim = kind, idx.numel(), a.shape[0], B, D, 1
    d.step_index, d.step_time, d.a, d.init = idx.data_ptr(), tau.data_ptr(), a.data_ptr(), init.data_ptr()
    d.w0, d.w1 = w0.data_ptr(), w1.data_ptr()
    d.b0, d.b1 = (0 if b0 is None else b0.data_ptr()), (0 if b1 is None else b1.data_ptr())
    d.h = h.data_ptr()
    return d


def _forward(ctx, kind, init, a, idx, tau, w0, w1, b0, b1, tape):
    lib = L.lib()
    initc, ac = _f32c(init), _f32c(a)
    idx, tau = _i32c(idx, "step index table"), _f32c(tau)   # the kernels read int32 rows and fp32 times, whatever came in
    w0c, w1c = _f32c(w0), _f32c(w1)
    b0c = None if b0 is None else _f32c(b0)
    b1c = None if b1 is None else _f32c(b1)
    B, D = initc.shape
    h = torch.empty((idx.numel(), B, D), device=init.device, dtype=torch.float32)
    d = _desc(kind, initc, ac, idx, tau, w0c, w1c, b0c, b1c, h)
    c = None
    if kind == L.SEQDEC_TLSTM and tape:
        c = torch.empty_like(h)  # cell-state tape for the BPTT kernel
        d.c = c.data_ptr()
    with torch.cuda.device(init.device):
        L.check(lib.hode_seqdec_fwd(d, _stream()), "hode_seqdec_fwd")
    ctx.save_for_backward(initc, ac, idx, tau, w0c, w1c, b0c, b1c, h, c)
    ctx.kind = kind
    return h


def _backward(ctx, grad_h):
    initc, ac, idx, tau, w0c, w1c, b0c, b1c, h, c = ctx.saved_tensors
    lib = L.lib()
    gh = _f32c(grad_h)
    d = _desc(ctx.kind, initc, ac, idx, tau, w0c, w1c, b0c, b1c, h)
    d.c = 0 if c is None else c.data_ptr()
    ginit, gw0, gw1 = torch.empty_like(initc), torch.empty_like(w0c), torch.empty_like(w1c)
    gb0 = None if b0c is None else torch.empty_like(b0c)
    gb1 = None if b1c is None else torch.empty_like(b1c)
    d.grad_h, d.grad_init, d.grad_w0, d.grad_w1 = gh.data_ptr(), ginit.data_ptr(), gw0.data_ptr(), gw1.data_ptr()
    d.grad_b0, d.grad_b1 = (0 if gb0 is None else gb0.data_ptr()), (0 if gb1 is None else gb1.data_ptr())
    n = lib.hode_seqdec_workspace_bytes(d)
    ws = torch.empty(max(n, 4), device=h.device, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    with torch.cuda.device(h.device):
        L.check(lib.hode_seqdec_bwd(d, _stream()), "hode_seqdec_bwd")
    return ginit, gw0, gw1, gb0, gb1


class _Tlstm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, init, w_ih, w_hh, b_ih, b_hh, a, idx, tau, tape):
        return _forward(ctx, L.SEQDEC_TLSTM, init, a, idx, tau, w_ih, w_hh, b_ih, b_hh, tape)

    @staticmethod
    def backward(ctx, grad_h):
        ginit, gw_ih, gw_hh, gb_ih, gb_hh = _backward(ctx, grad_h)
        return ginit, gw_ih, gw_hh, gb_ih, gb_hh, None, None, None, None


class _GruOde(torch.autograd.Function):
    @staticmethod
    def forward(ctx, init, w_z, w_n, a, idx, tau):
        return _forward(ctx, L.SEQDEC_GRUODE, init, a, idx, tau, w_z, w_n, None, None, False)

    @staticmethod
    def backward(ctx, grad_h):
        ginit, gw_z, gw_n, _, _ = _backward(ctx, grad_h)
        return ginit, gw_z, gw_n, None, None, None


def tlstm(init, a, idx, tau, max_row, w_ih, w_hh, b_ih, b_hh):
    """h (T', B, D): the hidden states of nn.LSTM(2, D) after steps k = 0 .. T'-1, h0 = c0 = init, input
    [a[idx[k]], tau[k]] (``step_tables``)."""
    _require_gpu(init, a, idx, tau, w_ih, w_hh, b_ih, b_hh)
    _check(init, a, idx, max_row)
    D = init.shape[1]
    if tuple(w_ih.shape) != (4 * D, 2) or tuple(w_hh.shape) != (4 * D, D):
        raise L.HodeConfigError("hode: tlstm expects nn.LSTM(2, %d) weights (got %s, %s)" % (D, tuple(w_ih.shape), tuple(w_hh.shape)))
    # the cell-state tape only when a backward can follow (needs_input_grad mirrors requires_grad, not the grad mode)
    tape = torch.is_grad_enabled() and any(x.requires_grad for x in (init, w_ih, w_hh, b_ih, b_hh))
    return _Tlstm.apply(init, w_ih, w_hh, b_ih, b_hh, a, idx, tau, tape)


def gruode(init, a, idx, tau, max_row, w_z, w_n):
    """h (T', B, D): h[k] = (1 - z[:D]) * (tanh(W_n (z * x_k)) - init), z = sigmoid(W_z x_k), x_k = [init, a[idx[k]], tau[k]]
    -- GRUODECell as the reference's decoder loop calls it (the hidden state it is handed is always ``init``)."""
    _require_gpu(init, a, idx, tau, w_z, w_n)
    _check(init, a, idx, max_row)
    D = init.shape[1]
    if tuple(w_z.shape) != (D + 2, D + 2) or tuple(w_n.shape) != (D, D + 2):
        raise L.HodeConfigError("hode: gruode expects GRUODECell(%d) weights (got %s, %s)" % (D, tuple(w_z.shape), tuple(w_n.shape)))
    return _GruOde.apply(init, w_z, w_n, a, idx, tau)
