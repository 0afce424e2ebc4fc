"""Neural ODE baselines of the real-data experiment (reference ``NeuralODEReal`` / ``NeuralODEReal2nd``,
``model.py:660-769``) on the gfx950 kernels of ``csrc/hode_neural_real_mf.hip``.

The reference's rhs reads ``dose(t) = cumsum(a, 0)[int(t)]`` (zeros once ``int(t) >= Ta``) at every stage, which costs a
host sync and a cumsum over the whole action per call.  Which row a stage reads depends only on the grid, the method and
``perturb``, so it is worked out once per grid on the host (``stage_rows``) and the dose of every (interval, stage) is
gathered into one table [T-1][stages][B] on the device; the kernels never see a stage time.  The backward returns
``grad_y0`` and the four ``ml_net`` gradients (accumulated on chip, fixed-order fold); the action takes none."""

from __future__ import annotations

import torch

from . import _lib as L
from .solver import _f32c, _require_gpu, _stream

KINDS = {"neural": L.RHS_NEURAL_REAL, "2nd": L.RHS_NEURAL_REAL_2ND}
MAX_LATENT = {"neural": 30, "2nd": 60}
MAX_HIDDEN = 64
_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def check_config(kind, latent_dim, hidden_dim, action_dim, method=None):
    """HodeConfigError unless the kernels cover this decoder: ``neural`` D 1..30, ``2nd`` even D 2..60, hidden 1..64,
    action_dim 1, a fixed-grid method."""
    D, H = int(latent_dim), int(hidden_dim)
    if kind not in KINDS:
        raise L.HodeConfigError("hode: neural-real kinds are 'neural' and '2nd' (got %r)" % (kind,))
    if kind == "2nd" and D % 2 != 0:
        raise L.HodeConfigError("hode: NeuralODEReal2nd needs an even latent_dim (got %d): [m(y), y[:D//2]] has D - 1 "
                                "columns otherwise, which the reference cannot integrate either" % D)
    if not 1 <= D <= MAX_LATENT[kind]:
        raise L.HodeConfigError("hode: %s decoder kernels cover latent_dim 1..%d (got %d)" % (kind, MAX_LATENT[kind], D))
    if not 1 <= H <= MAX_HIDDEN:
        raise L.HodeConfigError("hode: neural-real kernels cover hidden_dim 1..%d (got %d)" % (MAX_HIDDEN, H))
    if int(action_dim) != 1:
        raise L.HodeConfigError("hode: neural-real kernels take action_dim 1 (got %d)" % int(action_dim))
    if method is not None and method not in _STAGES:
        raise L.HodeConfigError("hode: NeuralODEReal* are built for the fixed-grid methods (euler, midpoint, rk4); got %r. "
                                "dopri5 with DecoderReal's options['step_t'] is not supported" % (method,))


def stage_times(grid, method, perturb):
    """fp32 time of every rhs call of the fixed-grid solve over ``grid``, (T-1, stages), in call order: the same torch
    ops as torchdiffeq's fixed-grid steps (oracle/solvers.py), applied to the whole grid at once."""
    g = grid.detach().to(torch.float32).cpu()
    t0, t1 = g[:-1], g[1:]
    dt = t1 - t0
    first = torch.nextafter(t0, t0 + 1) if perturb else t0
    if method == "euler":
        cols = [first]
    elif method == "midpoint":
        cols = [first, t0 + 0.5 * dt]
    elif method == "rk4":
        last = torch.nextafter(t1, t1 - 1) if perturb else t1
        cols = [first, t0 + dt * (1 / 3), t0 + dt * (2 / 3), last]
    else:
        raise L.HodeConfigError("hode: no stage times for method %r" % (method,))
    return torch.stack(cols, dim=1)


def stage_rows(grid, method, perturb, Ta):
    """The action row ``int(t)`` the reference's ``dose_at_time`` uses at every stage, (T-1, stages) int64 on the CPU
    (``int`` truncates toward zero; rows >= ``Ta`` read zeros, negative rows index from the end).  One host read-back:
    cache the result per grid (``NeuralODEReal`` does)."""
    rows = torch.trunc(stage_times(grid, method, perturb)).to(torch.int64)
    if rows.numel() and int(rows.min()) < -int(Ta):
        raise L.HodeConfigError("hode: a stage reads action row %d, outside an action of %d rows" % (int(rows.min()), Ta))
    return rows


def table_index(rows, Ta):
    """Row of ``cat([cumsum(a, 0), 0])`` every stage reads: Python indexing for negative rows, the zero row ``Ta`` for
    rows past the end."""
    idx = torch.where(rows < 0, rows + Ta, rows)
    return torch.where(rows >= Ta, torch.full_like(rows, Ta), idx)


def dose_table(a, index):
    """(T-1, stages, B) doses from the action (Ta, B, 1) and the flat ``table_index`` (on a's device)."""
    cs = torch.cumsum(a[..., 0].detach().to(torch.float32), dim=0)
    cs = torch.cat([cs, cs.new_zeros(1, cs.shape[1])], dim=0)
    return cs.index_select(0, index)


def _desc(kind, y0, t, dose, w1, b1, w2, b2, h, method):
    B, D = y0.shape
    d = L.new_solve_desc()
    d.rhs_kind, d.method = kind, L.METHODS[method]
    d.batch, d.latent_dim, d.n_times, d.hidden_dim = B, D, t.numel(), w1.shape[0]
    d.t, d.y0, d.dosage = t.data_ptr(), y0.data_ptr(), dose.data_ptr() if dose.numel() else 0
    d.w1, d.b1, d.w2, d.b2, d.h = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), h.data_ptr()
    return d


class _NeuralRealFixedGrid(torch.autograd.Function):
    """Gradients for y0 and the four weights; none for t and the dose table gathered from the action a (their .grad
    stays None)."""

    @staticmethod
    def forward(ctx, y0, w1, b1, w2, b2, t, dose, kind, method):
        lib = L.lib()
        y0c, tc, dc = _f32c(y0), _f32c(t), _f32c(dose)
        w1c, b1c, w2c, b2c = _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2)
        B, D = y0c.shape
        h = torch.empty((tc.numel(), B, D), device=y0.device, dtype=torch.float32)
        d = _desc(kind, y0c, tc, dc, w1c, b1c, w2c, b2c, h, method)
        with torch.cuda.device(y0.device):
            L.check(lib.hode_rk_fwd(d, _stream()), "hode_rk_fwd[neural-real]")
        ctx.save_for_backward(h, tc, dc, w1c, b1c, w2c, b2c)
        ctx.meta = (kind, method)
        return h

    @staticmethod
    def backward(ctx, grad_h):
        h, tc, dc, w1c, b1c, w2c, b2c = ctx.saved_tensors
        kind, method = ctx.meta
        lib = L.lib()
        T, B, D = h.shape
        gh = _f32c(grad_h)
        gy0 = torch.empty((B, D), device=h.device, dtype=torch.float32)
        gw1, gb1, gw2, gb2 = (torch.zeros_like(x) for x in (w1c, b1c, w2c, b2c))
        d = _desc(kind, h[0], tc, dc, w1c, b1c, w2c, b2c, h, method)
        d.grad_h, d.grad_y0 = gh.data_ptr(), gy0.data_ptr()
        d.grad_w1, d.grad_b1, d.grad_w2, d.grad_b2 = gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(), gb2.data_ptr()
        n = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
        ws = torch.empty(max(n, 4), device=h.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        with torch.cuda.device(h.device):
            L.check(lib.hode_rk_bwd(d, _stream()), "hode_rk_bwd[neural-real]")
        return gy0, gw1, gb1, gw2, gb2, None, None, None, None


def neural_real_solve(kind, y0, w1, b1, w2, b2, grid, a, index, method):
    """h (len(grid), B, D) of dy/dt = m([y, dose]) (``neural``) or [m([y, dose]), y[:D//2]] (``2nd``) on ``grid``;
    ``index`` = the flat ``table_index`` of ``stage_rows(grid, method, ...)`` on a's device."""
    check_config(kind, y0.shape[1], w1.shape[0], a.shape[2] if a.dim() == 3 else 0, method)
    _require_gpu(y0, w1, b1, w2, b2, grid, a)
    dose = dose_table(a, index)
    return _NeuralRealFixedGrid.apply(y0, w1, b1, w2, b2, grid, dose, KINDS[kind], method)
