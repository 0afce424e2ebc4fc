"""ctypes binding of libhode_roche_dims.so (C ABI: include/hode_roche_dims.h): the hybrid Roche kernels at the latent sizes
5 .. 16 that libhode.so does not hold, and ``roche_solver_library`` -- the one place that says which library serves the
Roche rhs at a latent size.  Fails loudly when the library is missing, stale or of another ABI version -- at the first call
that needs it, never at import and never for a size libhode.so serves."""

from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._loader import HodeConfigError, Library  # noqa: F401

HODE_ROCHE_DIMS_ABI_VERSION = 1
#: latent sizes this library is compiled for (build_hip.ROCHE_DIMS), fixed grid and dopri5 alike
DIMS = (5, 7, 9, 10, 11, 13, 14, 15, 16)
#: libhode.so's own: fixed grid (build_hip.RK_DIMS) and dopri5 (build_hip.DP_DIMS)
LIBHODE_RK_DIMS = (4, 6, 8, 12, 20)
LIBHODE_DP_DIMS = (4, 6, 8, 12)

_desc_p, _size_p = C.POINTER(L.SolveDesc), C.POINTER(C.c_size_t)
#: the entries that stand in for their hode_* namesakes of libhode.so: (suffix, restype, argtypes)
SOLVER_ENTRIES = (
    ("workspace_bytes", C.c_size_t, (_desc_p, C.c_int)),
    ("rk_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("rk_bwd", C.c_int, (_desc_p, C.c_void_p)),
    ("dopri5_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("dopri5_bwd", C.c_int, (_desc_p, C.c_void_p)),
    ("dopri5_tape_offsets", C.c_int, (_desc_p, _size_p)),
)
#: every symbol include/hode_roche_dims.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_roche_dims_version", C.c_int, ()),
    ("hode_roche_dims_last_error_string", C.c_char_p, ()),
) + tuple(("hode_roche_dims_" + n, r, a) for n, r, a in SOLVER_ENTRIES)

LIBRARY = Library("libhode_roche_dims.so", "HODE_ROCHE_DIMS_LIBRARY", EXPORTS, "hode_roche_dims_version",
                   "hode_roche_dims_last_error_string", HODE_ROCHE_DIMS_ABI_VERSION,
                   "the hybrid Roche rhs at a latent size libhode.so does not hold", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


class _AsLibhode:
    """The side library under libhode.so's names: ``hode_rk_fwd`` is ``hode_roche_dims_rk_fwd`` and so on, so that the
    bindings written against ``L.lib()`` call it unchanged.  A status-returning entry that fails raises here, with THIS
    library's error text; the caller's ``L.check`` then sees 0 and never asks libhode.so for a message it does not have."""

    def __init__(self, handle):
        for name, restype, _ in SOLVER_ENTRIES:
            fn = getattr(handle, "hode_roche_dims_" + name)
            setattr(self, "hode_" + name, fn if restype is C.c_size_t else self._checked(fn, "hode_roche_dims_" + name))

    @staticmethod
    def _checked(fn, what):
        def call(*args):
            check(fn(*args), what)
            return 0
        return call


_as_libhode = None


def roche_solver_library(latent_dim):
    """The library whose ``hode_workspace_bytes / hode_rk_fwd / hode_rk_bwd / hode_dopri5_fwd / hode_dopri5_bwd /
    hode_dopri5_tape_offsets`` serve ``HODE_RHS_ROCHE`` and ``HODE_RHS_ROCHE_ABLATE`` at ``latent_dim``:
    libhode_roche_dims.so for ``DIMS`` and libhode.so for everything else (which refuses what it has no kernel for).
    ``hode.roche_solve`` and ``hode.adaptive.roche_dopri5`` take the answer as ``library=``."""
    global _as_libhode
    if int(latent_dim) not in DIMS:
        return L.lib()
    handle = lib()
    if _as_libhode is None or _as_libhode[0] is not handle:
        _as_libhode = (handle, _AsLibhode(handle))
    return _as_libhode[1]


def sizes_text(dopri5=False):
    """The sizes both libraries hold, for error messages."""
    own = LIBHODE_DP_DIMS if dopri5 else LIBHODE_RK_DIMS
    return "%s (libhode.so) and %s (libhode_roche_dims.so)" % (", ".join(map(str, own)), ", ".join(map(str, DIMS)))
