"""A chain of Sylvester normalizing flows over the draws of a patient (``hode_sylvester_fwd`` / ``hode_sylvester_bwd``,
libhode_sylvester.so): reference ``Sylvester._forward`` (``flow.py:86-134``) and ``TriangularSylvester._forward``
(``flow.py:160-215``) as one forward and one backward launch instead of four ``bmm`` calls and a dozen element-wise
launches per flow and draw plus their autograd graph.  Two plain launch functions; the ``torch.autograd.Function`` that
joins them lives next to the modules it serves, in the package-root ``flow.py``."""

from __future__ import annotations

import torch

from . import _sylvester_lib as SL
from ._lib import HodeConfigError
from .solver import _f32c, _i32c, _ptr, _require_gpu, _stream


def check_domain(B, D, M, K, S, dense=True):
    """Raise HodeConfigError outside the kernels' domain (include/hode_sylvester.h); there is no fallback."""
    if B < 1:
        raise HodeConfigError("hode.sylvester: batch %d must be >= 1" % B)
    if not 1 <= D <= SL.MAX_LATENT:
        raise HodeConfigError("hode.sylvester: latent_dim %d outside 1..%d" % (D, SL.MAX_LATENT))
    if not 1 <= M <= SL.MAX_ORTHO:
        raise HodeConfigError("hode.sylvester: n_ortho %d outside 1..%d" % (M, SL.MAX_ORTHO))
    if not 1 <= K <= SL.MAX_FLOWS:
        raise HodeConfigError("hode.sylvester: n_flows %d outside 1..%d" % (K, SL.MAX_FLOWS))
    if not 1 <= S <= SL.MAX_SAMPLES:
        raise HodeConfigError("hode.sylvester: n_samples %d outside 1..%d" % (S, SL.MAX_SAMPLES))
    if not dense and M != D:
        raise HodeConfigError("hode.sylvester: triangular mode (no q) needs n_ortho %d == latent_dim %d" % (M, D))


def _shapes(z0, r1, r2, b, q, perm):
    if z0.dim() != 3 or r1.dim() != 4:
        raise HodeConfigError("hode.sylvester: shapes z0 (S, B, D), r1/r2 (B, K, M, M), b (B, K, M), q (B, K, D, M) expected")
    S, B, D = z0.shape
    K, M = r1.shape[1], r1.shape[2]
    check_domain(B, D, M, K, S, dense=q is not None)
    if r1.shape != (B, K, M, M) or r2.shape != (B, K, M, M) or b.shape != (B, K, M) or (q is not None and q.shape != (B, K, D, M)):
        raise HodeConfigError("hode.sylvester: shapes z0 (S, B, D), r1/r2 (B, K, M, M), b (B, K, M), q (B, K, D, M) expected")
    if perm is not None:
        if q is not None:
            raise HodeConfigError("hode.sylvester: perm belongs to triangular mode (q must be None)")
        if perm.shape != (K, D):
            raise HodeConfigError("hode.sylvester: perm (K, D) = (%d, %d) expected, got %s" % (K, D, tuple(perm.shape)))
    return S, B, D, M, K


def sylvester_forward(z0, r1, r2, b, q=None, perm=None, want_log_diag=False, save_tape=True):
    """The forward launch.  z0 (S, B, D); r1, r2 (B, K, M, M); b (B, K, M); q (B, K, D, M) or None (triangular mode, M == D);
    perm (K, D) integer index or None.  Returns ``(z_K (S, B, D), logdet (S, B), log_diag (S, B, K, M) or None, tape)``:
    ``tape`` is the float32 workspace holding z_1 .. z_{K-1} that ``sylvester_backward`` reads (None when ``save_tape`` is
    False or K == 1).  A ``perm`` entry outside 0 .. D-1 is refused (one read-back of the (K, D) table per call)."""
    _require_gpu(z0, r1, r2, b, q, perm)
    lib = SL.lib()
    z0c, r1c, r2c, bc = _f32c(z0), _f32c(r1), _f32c(r2), _f32c(b)
    qc = _f32c(q) if q is not None else None
    pc = _i32c(perm, "perm") if perm is not None else None
    S, B, D, M, K = _shapes(z0c, r1c, r2c, bc, qc, pc)
    if pc is not None and (int(pc.min()) < 0 or int(pc.max()) >= D):
        raise HodeConfigError("hode.sylvester: perm entries must lie in 0..%d" % (D - 1))
    d = SL.new_desc()
    d.batch, d.latent_dim, d.n_ortho, d.n_flows, d.n_samples = B, D, M, K, S
    d.z0, d.r1, d.r2, d.b, d.q, d.perm = z0c.data_ptr(), r1c.data_ptr(), r2c.data_ptr(), bc.data_ptr(), _ptr(qc), _ptr(pc)
    z_out = torch.empty((S, B, D), device=z0c.device, dtype=torch.float32)
    logdet = torch.empty((S, B), device=z0c.device, dtype=torch.float32)
    log_diag = torch.empty((S, B, K, M), device=z0c.device, dtype=torch.float32) if want_log_diag else None
    tape = None
    if save_tape and K > 1:
        tape = torch.empty((lib.hode_sylvester_workspace_bytes(d) // 4,), device=z0c.device, dtype=torch.float32)
        d.workspace_bytes = tape.numel() * 4
    d.z_out, d.logdet, d.log_diag, d.workspace = z_out.data_ptr(), logdet.data_ptr(), _ptr(log_diag), _ptr(tape)
    with torch.cuda.device(z0c.device):
        SL.check(lib.hode_sylvester_fwd(d, _stream()), "hode_sylvester_fwd")
    return z_out, logdet, log_diag, tape


def sylvester_backward(z0, r1, r2, b, q, perm, tape, grad_z=None, grad_logdet=None, grad_log_diag=None):
    """The backward launch for the inputs of a ``sylvester_forward`` call and the ``tape`` it returned.  Cotangents
    ``grad_z`` (S, B, D), ``grad_logdet`` (S, B), ``grad_log_diag`` (S, B, K, M), each or None (zero).  Returns
    ``(grad_z0, grad_r1, grad_r2, grad_b, grad_q or None)``; the parameter gradients are sums over the S draws, formed in
    a fixed order (bit-identical repeats)."""
    _require_gpu(z0, r1, r2, b, q, perm, tape, grad_z, grad_logdet, grad_log_diag)
    lib = SL.lib()
    z0c, r1c, r2c, bc = _f32c(z0), _f32c(r1), _f32c(r2), _f32c(b)
    qc = _f32c(q) if q is not None else None
    pc = _i32c(perm, "perm") if perm is not None else None
    ws = _f32c(tape) if tape is not None else None
    gz = _f32c(grad_z) if grad_z is not None else None
    gl = _f32c(grad_logdet) if grad_logdet is not None else None
    gd = _f32c(grad_log_diag) if grad_log_diag is not None else None
    S, B, D, M, K = _shapes(z0c, r1c, r2c, bc, qc, pc)
    if (gz is not None and gz.shape != (S, B, D)) or (gl is not None and gl.shape != (S, B)) \
            or (gd is not None and gd.shape != (S, B, K, M)):
        raise HodeConfigError("hode.sylvester: cotangents grad_z (S, B, D), grad_logdet (S, B), grad_log_diag (S, B, K, M) expected")
    d = SL.new_desc()
    d.batch, d.latent_dim, d.n_ortho, d.n_flows, d.n_samples = B, D, M, K, S
    d.z0, d.r1, d.r2, d.b, d.q, d.perm = z0c.data_ptr(), r1c.data_ptr(), r2c.data_ptr(), bc.data_ptr(), _ptr(qc), _ptr(pc)
    d.workspace, d.workspace_bytes = _ptr(ws), (ws.numel() * 4 if ws is not None else 0)
    d.grad_z_out, d.grad_logdet, d.grad_log_diag = _ptr(gz), _ptr(gl), _ptr(gd)
    g_z0, g_r1, g_r2, g_b = torch.empty_like(z0c), torch.empty_like(r1c), torch.empty_like(r2c), torch.empty_like(bc)
    g_q = torch.empty_like(qc) if qc is not None else None
    d.grad_z0, d.grad_r1, d.grad_r2, d.grad_b, d.grad_q = g_z0.data_ptr(), g_r1.data_ptr(), g_r2.data_ptr(), g_b.data_ptr(), _ptr(g_q)
    with torch.cuda.device(z0c.device):
        SL.check(lib.hode_sylvester_bwd(d, _stream()), "hode_sylvester_bwd")
    return g_z0, g_r1, g_r2, g_b, g_q
