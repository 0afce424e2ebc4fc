"""ctypes binding of libhode_real_step.so (C ABI: include/hode_real_step.h): the one-step-ahead solve of the real-data
hybrid rhs on the matrix cores at the latent sizes 5 .. 20, and ``step_library`` -- the library under libhode.so's
``hode_workspace_bytes / hode_rk_fwd / hode_rk_bwd`` names for ONE call, so that ``hode.real._RealFixedGrid`` drives it
with the code of the chained solve.  Fails loudly when the library is missing, stale or of another ABI version -- at the
first call that needs it, never at import."""

from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._loader import HodeConfigError, Library  # noqa: F401

HODE_REAL_STEP_ABI_VERSION = 1
#: latent sizes, hidden sizes (one to four tiles of 16) and solver steps per interval the library serves
MIN_LATENT, MAX_LATENT = 5, 20
MAX_HIDDEN = 64
MAX_SUBSTEPS = 8

_desc_p = C.POINTER(L.SolveDesc)
#: the entries that stand in for their hode_* namesakes of libhode.so: (suffix, restype, argtypes)
SOLVER_ENTRIES = (
    ("workspace_bytes", C.c_size_t, (_desc_p, C.c_int)),
    ("rk_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("rk_bwd", C.c_int, (_desc_p, C.c_void_p)),
)
#: every symbol include/hode_real_step.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_real_step_version", C.c_int, ()),
    ("hode_real_step_last_error_string", C.c_char_p, ()),
    ("hode_real_step_intervals_per_wave", C.c_int, (_desc_p,)),
) + tuple(("hode_real_step_" + n, r, a) for n, r, a in SOLVER_ENTRIES)

LIBRARY = Library("libhode_real_step.so", "HODE_REAL_STEP_LIBRARY", EXPORTS, "hode_real_step_version",
                  "hode_real_step_last_error_string", HODE_REAL_STEP_ABI_VERSION,
                  "the one-step-ahead solve of the real-data hybrid rhs", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


class _AsLibhode:
    """The step library under libhode.so's names for one solve of ``intervals`` intervals with ``substeps`` solver steps
    each: ``hode_rk_fwd`` is ``hode_real_step_rk_fwd`` and so on.  ``hode_solve_desc`` has no field of its own for the three
    numbers; every entry writes them into the fields include/hode_real_step.h names for them (``n_times`` = intervals,
    ``n_dose`` = solver steps per interval, ``max_steps`` = intervals per wave, 0 = the library chooses) before it calls.
    A status-returning entry that fails raises here, with THIS library's error text; the caller's ``L.check`` then sees
    0 and never asks libhode.so for a message it does not have."""

    def __init__(self, handle, intervals, substeps, intervals_per_wave=0):
        self.intervals, self.substeps, self.intervals_per_wave = int(intervals), int(substeps), int(intervals_per_wave)
        for name, restype, _ in SOLVER_ENTRIES:
            fn = getattr(handle, "hode_real_step_" + name)
            setattr(self, "hode_" + name, self._sized(fn) if restype is C.c_size_t else self._checked(fn, "hode_real_step_" + name))
        self.chosen_intervals_per_wave = self._sized(handle.hode_real_step_intervals_per_wave)

    def describe(self, d):
        d.n_times, d.n_dose, d.max_steps = self.intervals, self.substeps, self.intervals_per_wave
        return d

    def _sized(self, fn):
        def call(d, *args):
            return fn(self.describe(d), *args)
        return call

    def _checked(self, fn, what):
        def call(d, *args):
            check(fn(self.describe(d), *args), what)
            return 0
        return call


def step_library(intervals, substeps, intervals_per_wave=0):
    """libhode_real_step.so under libhode.so's entry names for one call (loads it on first use)."""
    return _AsLibhode(lib(), intervals, substeps, intervals_per_wave)


def is_step_library(library):
    return isinstance(library, _AsLibhode)


def sizes_text():
    """What the library serves, for error messages."""
    return ("latent_dim %d .. %d with hidden_dim 1 .. %d, euler / midpoint / rk4 and the same 1 .. %d solver steps in every "
            "interval (libhode_real_step.so)" % (MIN_LATENT, MAX_LATENT, MAX_HIDDEN, MAX_SUBSTEPS))
