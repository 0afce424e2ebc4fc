"""One-step-ahead ("step") solve of the real-data hybrid ODE (reference ``DecoderReal.forward`` with a 3-D ``init``,
``model.py:838-856``) on libhode_real_step.so: interval ``i`` of the grid ``t`` is integrated on its own from ``init[i]``, all
``(len(t) - 1) * B`` of them in one launch per direction.

The solver grid of an interval is torchdiffeq's: ``t[i] + k * step_size`` with the last point clipped to ``t[i + 1]``
(``hode.substep.fixed_grid`` over ``t[i : i + 2]``, in ``t``'s dtype), so the end point is always a grid point and nothing
is interpolated.  Served: every grid on which all intervals get the same number S of solver steps, 1 <= S <= 8.  The
autograd function is ``hode.real._RealFixedGrid``, the one of the chained solve, handed a 3-D ``y0`` and the (N, S + 1)
grid table."""

from __future__ import annotations

import torch

from . import _lib as L
from . import _real_step_lib as RS
from . import substep
from .real import _RealFixedGrid
from .solver import _require_gpu

_grid_cache = {}


def interval_grids(t, step_size=None):
    """The solver grids of the ``len(t) - 1`` intervals as one (N, S + 1) CPU table in ``t``'s dtype: row ``i`` is
    ``substep.fixed_grid(t[i : i + 2], step_size)`` (``t[i : i + 2]`` itself without a step size).  Raises
    ``HodeConfigError`` when the intervals do not all get the same number of solver steps, or more than eight."""
    tc = t.detach().cpu()
    rows = [tc[i:i + 2] if step_size is None else substep.fixed_grid(tc[i:i + 2], step_size) for i in range(tc.numel() - 1)]
    counts = sorted({r.numel() - 1 for r in rows})
    if len(counts) != 1:
        raise L.HodeConfigError("hode: the one-step-ahead solve needs the same number of solver steps in every interval; step_size %r "
                                "gives %s on this grid; have %s" % (step_size, " and ".join(map(str, counts)), RS.sizes_text()))
    if not 1 <= counts[0] <= RS.MAX_SUBSTEPS:
        raise L.HodeConfigError("hode: the one-step-ahead solve has no kernel for %d solver steps per interval (step_size %r); have %s"
                                % (counts[0], step_size, RS.sizes_text()))
    return torch.stack(rows)


def _grid_table(t, step_size):
    """``interval_grids`` on ``t``'s device as fp32: one host read-back per grid tensor (cached on its identity and version,
    like ``_uniform_grid_cache``), so a training step that hands over the same ``t`` has no sync."""
    key = (t._version, None if step_size is None else float(step_size), t.device)
    hit = _grid_cache.get(id(t))
    if hit is None or hit[0] is not t or hit[1] != key:
        if len(_grid_cache) >= 16:
            _grid_cache.clear()
        hit = (t, key, interval_grids(t, step_size).to(torch.float32).to(t.device))
        _grid_cache[id(t)] = hit
    return hit[2]


def real_step_solve(init, theta, wflat, t, act, hidden, method="midpoint", perturb=True, step_size=None, intervals_per_wave=0):
    """h (N + 1, B, D) for ``init`` (>= N, B, D) and the grid ``t`` of N + 1 points: ``h[0] = 0`` and ``h[i + 1]`` is the state
    at ``t[i + 1]`` of the solve that starts from ``init[i]`` at ``t[i]``.  Rows of ``init`` beyond N are not read (their
    gradient is the zero autograd gives an unused slice).  ``theta``, ``wflat``, ``act``, ``hidden``, ``method`` and
    ``perturb`` as in ``hode.real.real_solve``; ``step_size`` is torchdiffeq's ``options["step_size"]``;
    ``intervals_per_wave`` forces the run length C of the launch (tuning / tests), 0 = the library chooses."""
    if method not in L.METHODS:
        raise L.HodeConfigError("hode: the real-data rhs is built for the fixed-grid methods (euler, midpoint, rk4); got %r" % (method,))
    if init.dim() != 3:
        raise L.HodeConfigError("hode: the one-step-ahead solve takes per-interval start states (N, B, D); got %d-D" % init.dim())
    D, hidden, N = int(init.shape[-1]), int(hidden), int(t.numel()) - 1
    # refused here, before a library is loaded or anything is launched
    if not RS.MIN_LATENT <= D <= RS.MAX_LATENT or not 1 <= hidden <= RS.MAX_HIDDEN:
        raise L.HodeConfigError("hode: the one-step-ahead solve has no kernel for latent_dim %d with hidden_dim %d; have %s"
                                % (D, hidden, RS.sizes_text()))
    if N < 1 or int(init.shape[0]) < N:
        raise L.HodeConfigError("hode: the one-step-ahead solve over a grid of %d points needs %d start states (one per interval); "
                                "init has %d rows" % (N + 1, max(N, 1), int(init.shape[0])))
    if int(intervals_per_wave) < 0:
        raise L.HodeConfigError("hode: intervals_per_wave %d (0 = the library chooses)" % int(intervals_per_wave))
    grids = _grid_table(t, step_size)
    _require_gpu(init, theta, wflat, t, act)   # before the library is loaded: there is no CPU path
    library = RS.step_library(N, grids.shape[1] - 1, int(intervals_per_wave))
    return _RealFixedGrid.apply(init[:N], theta, wflat, grids, act, L.METHODS[method], bool(perturb), hidden, 0, library)
