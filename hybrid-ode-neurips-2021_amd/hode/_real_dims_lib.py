"""ctypes binding of libhode_real_dims.so (C ABI: include/hode_real_dims.h): the real-data hybrid rhs on the matrix cores at
the latent sizes 5 .. 20, and ``real_solver_library`` -- the one place that says which library serves
``HODE_RHS_ROCHE_REAL`` at a latent size.  Fails loudly when the library is missing, stale or of another ABI version -- at
the first call that needs it, never at import and never for a size libhode.so serves."""

from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._loader import HodeConfigError, Library  # noqa: F401

HODE_REAL_DIMS_ABI_VERSION = 1
#: latent sizes the library accepts; 20 only so that it can be held against libhode.so, which serves it by default
MIN_LATENT, MAX_LATENT = 5, 20
#: the sizes ``real_solver_library`` gives to this library
DIMS = tuple(range(5, 20))
#: hidden sizes (one to four tiles of 16)
MAX_HIDDEN = 64
#: libhode.so's own latent sizes for this rhs (csrc/hode_real.hip check_real)
LIBHODE_DIMS = (4, 20)

_desc_p = C.POINTER(L.SolveDesc)
#: the entries that stand in for their hode_* namesakes of libhode.so: (suffix, restype, argtypes)
SOLVER_ENTRIES = (
    ("workspace_bytes", C.c_size_t, (_desc_p, C.c_int)),
    ("rk_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("rk_bwd", C.c_int, (_desc_p, C.c_void_p)),
)
#: every symbol include/hode_real_dims.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_real_dims_version", C.c_int, ()),
    ("hode_real_dims_last_error_string", C.c_char_p, ()),
) + tuple(("hode_real_dims_" + n, r, a) for n, r, a in SOLVER_ENTRIES)

LIBRARY = Library("libhode_real_dims.so", "HODE_REAL_DIMS_LIBRARY", EXPORTS, "hode_real_dims_version",
                   "hode_real_dims_last_error_string", HODE_REAL_DIMS_ABI_VERSION,
                   "the real-data hybrid rhs at a latent size libhode.so does not hold", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


class _AsLibhode:
    """The side library under libhode.so's names: ``hode_rk_fwd`` is ``hode_real_dims_rk_fwd`` and so on, so that
    ``hode.real`` calls it unchanged.  A status-returning entry that fails raises here, with THIS library's error text; the
    caller's ``L.check`` then sees 0 and never asks libhode.so for a message it does not have."""

    def __init__(self, handle):
        for name, restype, _ in SOLVER_ENTRIES:
            fn = getattr(handle, "hode_real_dims_" + name)
            setattr(self, "hode_" + name, fn if restype is C.c_size_t else self._checked(fn, "hode_real_dims_" + name))

    @staticmethod
    def _checked(fn, what):
        def call(*args):
            check(fn(*args), what)
            return 0
        return call


_as_libhode = None


def side_library():
    """libhode_real_dims.so under libhode.so's entry names (loads it on first use)."""
    global _as_libhode
    handle = lib()
    if _as_libhode is None or _as_libhode[0] is not handle:
        _as_libhode = (handle, _AsLibhode(handle))
    return _as_libhode[1]


def is_side_library(library):
    return isinstance(library, _AsLibhode)


def real_solver_library(latent_dim):
    """The library whose ``hode_workspace_bytes / hode_rk_fwd / hode_rk_bwd`` serve ``HODE_RHS_ROCHE_REAL`` at
    ``latent_dim``: libhode_real_dims.so for 5 .. 19 and libhode.so for everything else (which refuses what it has no
    kernel for).  ``hode.real.real_solve`` asks here when it is given no ``library=``."""
    if int(latent_dim) not in DIMS:
        return L.lib()
    return side_library()


def sizes_text():
    """The sizes both libraries hold, for error messages."""
    return ("latent_dim %s at any hidden_dim (libhode.so; matrix cores at 20 with hidden_dim <= %d, one patient per lane otherwise) "
            "and latent_dim %d .. %d with hidden_dim 1 .. %d on the matrix cores only (libhode_real_dims.so)"
            % (", ".join(map(str, LIBHODE_DIMS)), MAX_HIDDEN, DIMS[0], DIMS[-1], MAX_HIDDEN))
