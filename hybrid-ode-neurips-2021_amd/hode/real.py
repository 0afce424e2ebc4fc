"""Fixed-grid solve of the real-data hybrid ODE (reference ``RocheODEReal``, ``model.py:570-657``) on the gfx950 kernels:
libhode.so at the latent sizes 4 and 20, libhode_real_dims.so (matrix cores, on-chip weight gradients) at 5 .. 19; the
one-step-ahead solve (``hode.real_step``: a start state per interval) runs through the same autograd function on
libhode_real_step.so.

The backward kernel returns ``grad_y0`` and the gradients of the three scalars, and tapes the operands of every linear
layer's weight gradient; they are contracted here with batched BLAS GEMMs and returned as one flat gradient matching
the flat weight buffer (parameter creation order of the reference)."""

from __future__ import annotations

import torch

from . import _lib as L
from . import _real_dims_lib as RD
from . import _real_step_lib as RS
from .solver import _f32c, _require_gpu, _stream

_STAGES = {L.METHOD_EULER: 1, L.METHOD_MIDPOINT: 2, L.METHOD_RK4_38: 4}


def _desc(y0, t, act, theta, wflat, h, method, perturb, hidden):
    B, D = y0.shape[-2:]
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.perturb = L.RHS_ROCHE_REAL, method, int(perturb)
    d.batch, d.latent_dim, d.n_times, d.hidden_dim, d.n_action_times = B, D, t.numel(), hidden, act.shape[0]
    d.t, d.y0, d.dosage, d.theta, d.w1, d.h = t.data_ptr(), y0.data_ptr(), act.data_ptr(), theta.data_ptr(), wflat.data_ptr(), h.data_ptr()
    return d


class _RealFixedGrid(torch.autograd.Function):
    """Gradients for y0, theta, wflat; none for t and the action table act (their .grad stays None).

    A 3-D ``y0`` (N, B, D) with a 2-D ``t`` (N, S + 1) is the one-step-ahead solve (``lib`` is then the step library of
    ``hode._real_step_lib``): interval i starts from ``y0[i]`` and runs over the S solver steps of ``t[i]``; ``h`` is
    (N + 1, B, D) with the zero row first, ``grad_y0`` has ``y0``'s shape."""

    @staticmethod
    def forward(ctx, y0, theta, wflat, t, act, method, perturb, hidden, lanes, lib):
        _require_gpu(y0, theta, wflat, t, act)
        y0c, thc, wc, tc, ac = _f32c(y0), _f32c(theta), _f32c(wflat), _f32c(t), _f32c(act)
        B, D = y0c.shape[-2:]
        M = D - 4
        assert wc.numel() == 9 * hidden + 2 + 3 * M * M, "flat weight buffer has the wrong length"
        step = y0c.dim() == 3
        assert not step or (RS.is_step_library(lib) and tc.dim() == 2 and tc.shape[0] == y0c.shape[0]), "step solve: t is (N, S + 1)"
        h = torch.empty((y0c.shape[0] + 1 if step else tc.numel(), B, D), device=y0.device, dtype=torch.float32)
        d = _desc(y0c, tc, ac, thc, wc, h, method, perturb, hidden)
        d.lanes_per_patient = lanes
        n = lib.hode_workspace_bytes(d, L.WS_RK_FWD)  # the per-patient dose table
        ws = torch.empty(max(n, 4), device=y0.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        with torch.cuda.device(y0.device):
            L.check(lib.hode_rk_fwd(d, _stream()), "hode_rk_fwd[real]")
        if step:  # h[0] is the zero row there: the start states are the input
            ctx.save_for_backward(y0c, h, thc, wc, tc, ac)
        else:
            ctx.save_for_backward(h, thc, wc, tc, ac)
        ctx.meta = (method, int(perturb), int(hidden), lanes, lib)
        return h

    @staticmethod
    def backward(ctx, grad_h):
        method, perturb, H, lanes, lib = ctx.meta
        if RS.is_step_library(lib):
            y0c, h, thc, wc, tc, ac = ctx.saved_tensors
        else:
            h, thc, wc, tc, ac = ctx.saved_tensors
            y0c = h[0]
        T, B, D = h.shape
        gh = _f32c(grad_h)
        gy0 = torch.empty(y0c.shape, device=h.device, dtype=torch.float32)
        gth = torch.zeros(L.N_THETA, device=h.device, dtype=torch.float32)
        d = _desc(y0c, tc, ac, thc, wc, h, method, perturb, H)
        d.lanes_per_patient = lanes
        d.grad_h, d.grad_y0, d.grad_theta = gh.data_ptr(), gy0.data_ptr(), gth.data_ptr()
        # matrix-core kernels (D = 20, hidden <= 64; the side library at every size it serves): the weight gradients are
        # accumulated on chip into this flat buffer; the lane-per-patient kernels (lanes_per_patient = 1, D = 4,
        # hidden > 64) tape the GEMM operands for contract_tape
        onchip = RD.is_side_library(lib) or RS.is_step_library(lib) or (D == 20 and H <= 64 and lanes != 1)
        if onchip:
            gw = torch.zeros_like(wc)
            d.grad_w1 = gw.data_ptr()
        n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
        ws = torch.empty(max(n, 4), device=h.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        with torch.cuda.device(h.device):
            L.check(lib.hode_rk_bwd(d, _stream()), "hode_rk_bwd[real]")
        if onchip:
            return gy0, gth[:3].clone(), gw, None, None, None, None, None, None, None
        return gy0, gth[:3].clone(), contract_tape(ws, T, B, D, H, method), None, None, None, None, None, None, None


def contract_tape(ws, T, B, D, H, method):
    """Flat weight gradient (creation order of the flat weight buffer) from the GEMM operands a tape-writing backward left
    at offset 0 of its workspace ``ws``: per stage instance, rows [y3 | a11 | u11 | u12 | a21 | u21 | u22 | hh rh ur uz uh]
    of ``B`` floats each (the lane-per-patient kernels, and the matrix-core backward when the caller passes no grad_w1)."""
    M = D - 4
    inst = (T - 1) * _STAGES[method]
    rows = 5 + 4 * H + 5 * M
    if inst == 0:
        return torch.zeros(9 * H + 2 + 3 * M * M, device=ws.device, dtype=torch.float32)
    tape = ws[: inst * rows * B * 4].view(torch.float32).view(inst, rows, B)
    o = 0

    def take(k):
        nonlocal o
        v = tape[:, o:o + k]
        o += k
        return v

    y3, a11, u11, u12, a21, u21, u22 = take(3), take(H), take(H), take(1), take(H), take(H), take(1)
    hh, rh, ur, uz, uh = (take(M) for _ in range(5)) if M > 0 else (None,) * 5

    # sums over instances are (1 x inst) GEMMs: torch's strided sum over these shapes runs at a fraction of HBM speed
    ones_i = torch.ones((1, inst), device=ws.device, dtype=torch.float32)
    ones_b = torch.ones((B, 1), device=ws.device, dtype=torch.float32)

    def fold(part):  # (inst, m, n) -> (m, n)
        return (ones_i @ part.reshape(inst, -1)).view(part.shape[1], part.shape[2])

    def outer(u, x):  # sum over instances and patients of u x^T
        return fold(torch.bmm(u, x.transpose(1, 2)))

    def colsum(u):   # (inst, k, B) -> (k,)
        return fold(u @ ones_b).reshape(-1)

    parts = [outer(u11, y3).reshape(-1), colsum(u11), outer(u12, a11).reshape(-1), colsum(u12),
             outer(u21, y3[:, :2]).reshape(-1), colsum(u21), outer(u22, a21).reshape(-1), colsum(u22)]
    if M > 0:
        parts += [outer(uh, rh).reshape(-1), outer(uz, hh).reshape(-1), outer(ur, hh).reshape(-1)]
    return torch.cat(parts)


def real_solve(y0, theta, wflat, t, act, hidden, method="midpoint", perturb=True, lanes_per_patient=0, library=None):
    """h (T, B, D).  ``theta`` = (k_immunity, kel, kel2); ``wflat`` = all weights in creation order; ``act`` (Ta, B) doses.
    ``lanes_per_patient`` forces a kernel family (tuning / tests): 1 = one patient per lane, 16 = matrix cores where they
    exist; 0 = the library chooses.  ``library`` is the kernel library to call; None chooses by latent size
    (``real_solver_library``: libhode_real_dims.so for D = 5 .. 19, libhode.so otherwise)."""
    if method not in L.METHODS:
        raise L.HodeConfigError("hode: the real-data rhs is built for the fixed-grid methods (euler, midpoint, rk4); got %r" % (method,))
    D, hidden, lanes = int(y0.shape[-1]), int(hidden), int(lanes_per_patient)
    if library is None and D in RD.DIMS and (not 1 <= hidden <= RD.MAX_HIDDEN or lanes == 1):
        # refused here, before a library is loaded or anything is launched, with the sizes of both libraries
        raise L.HodeConfigError("hode: the real-data hybrid rhs has no kernel for latent_dim %d with hidden_dim %d, lanes_per_patient %d; "
                                "have %s" % (D, hidden, lanes, RD.sizes_text()))
    if library is None:
        library = RD.real_solver_library(D)
    return _RealFixedGrid.apply(y0, theta, wflat, t, act, L.METHODS[method], bool(perturb), hidden, lanes, library)
