"""ctypes binding of libhode_neural_odd.so (C ABI: include/hode_neural_odd.h): the NeuralODE kernels at the odd latent
dimensions 5 .. 15, and ``neural_solver_library`` -- the one place that says which library serves the NeuralODE rhs at a
latent dimension.  Fails loudly when the library is missing, stale or of another ABI version -- at the first call that
needs it, never at import and never for a dimension libhode.so serves."""

from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._loader import HodeConfigError, Library  # noqa: F401

HODE_NEURAL_ODD_ABI_VERSION = 1
#: latent dimensions this library is compiled for (build_hip.NEURAL_ODD_DIMS); libhode.so has hode.adaptive.NEURAL_DIMS
DIMS = (5, 7, 9, 11, 13, 15)

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
#: every symbol include/hode_neural_odd.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_neural_odd_version", C.c_int, ()),
    ("hode_neural_odd_last_error_string", C.c_char_p, ()),
) + tuple(("hode_neural_odd_" + n, r, a) for n, r, a in SOLVER_ENTRIES)

LIBRARY = Library("libhode_neural_odd.so", "HODE_NEURAL_ODD_LIBRARY", EXPORTS, "hode_neural_odd_version",
                   "hode_neural_odd_last_error_string", HODE_NEURAL_ODD_ABI_VERSION,
                   "the NeuralODE rhs at an odd latent dimension", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


class _AsLibhode:
    """The side library under libhode.so's names: ``hode_rk_fwd`` is ``hode_neural_odd_rk_fwd`` and so on, so that the
    bindings written against ``L.lib()`` call it unchanged.  A status-returning entry that fails raises here, with THIS
    library's error text; the caller's ``L.check`` then sees 0 and never asks libhode.so for a message it does not have."""

    def __init__(self, handle):
        for name, restype, _ in SOLVER_ENTRIES:
            fn = getattr(handle, "hode_neural_odd_" + name)
            setattr(self, "hode_" + name, fn if restype is C.c_size_t else self._checked(fn, "hode_neural_odd_" + name))

    @staticmethod
    def _checked(fn, what):
        def call(*args):
            check(fn(*args), what)
            return 0
        return call


_as_libhode = None


def neural_solver_library(latent_dim):
    """The library whose ``hode_workspace_bytes / hode_rk_fwd / hode_rk_bwd / hode_dopri5_fwd / hode_dopri5_bwd /
    hode_dopri5_tape_offsets`` serve ``HODE_RHS_NEURAL`` at ``latent_dim``: libhode_neural_odd.so for 5, 7, ..., 15 and
    libhode.so for everything else (which refuses what it has no kernel for)."""
    global _as_libhode
    if int(latent_dim) not in DIMS:
        return L.lib()
    handle = lib()
    if _as_libhode is None or _as_libhode[0] is not handle:
        _as_libhode = (handle, _AsLibhode(handle))
    return _as_libhode[1]
