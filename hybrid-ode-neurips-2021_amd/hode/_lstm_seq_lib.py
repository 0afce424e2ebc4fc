"""ctypes binding of libhode_lstm_seq.so (C ABI: include/hode_lstm_seq.h): the masked LSTM window kernels with the hidden
state of every step as output, and ``side_library`` -- the library under libhode.so's ``hode_lstm_*`` names, so that
``hode.lstm._LstmEncode`` calls either with the same code.  Fails loudly when the library is missing, stale or of another ABI
version -- at the first call that needs it, never at import and never for a call libhode.so serves."""

from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._loader import HodeConfigError, Library  # noqa: F401

HODE_LSTM_SEQ_ABI_VERSION = 1
#: largest hidden size (csrc/hode_lstm.hip lstm_geom: the padded sizes 16 .. 160)
MAX_HIDDEN = 160

_desc_p = C.POINTER(L.LstmDesc)
#: the entries that stand in for their hode_lstm_* namesakes of libhode.so: (suffix, restype, argtypes)
LSTM_ENTRIES = (
    ("workspace_bytes", C.c_size_t, (_desc_p,)),
    ("fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("bwd", C.c_int, (_desc_p, C.c_void_p)),
    ("fill_operand", C.c_int, (_desc_p, C.c_void_p)),
)
#: every symbol include/hode_lstm_seq.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_lstm_seq_version", C.c_int, ()),
    ("hode_lstm_seq_last_error_string", C.c_char_p, ()),
) + tuple(("hode_lstm_seq_" + n, r, a) for n, r, a in LSTM_ENTRIES)

LIBRARY = Library("libhode_lstm_seq.so", "HODE_LSTM_SEQ_LIBRARY", EXPORTS, "hode_lstm_seq_version",
                  "hode_lstm_seq_last_error_string", HODE_LSTM_SEQ_ABI_VERSION,
                  "the LSTM with the hidden state of every step as output", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


class _AsLibhode:
    """The side library under libhode.so's names: ``hode_lstm_fwd`` is ``hode_lstm_seq_fwd`` and so on.  A status-returning
    entry that fails raises here, with THIS library's error text; the caller's ``L.check`` then sees 0 and never asks
    libhode.so for a message it does not have."""

    def __init__(self, handle):
        for name, restype, _ in LSTM_ENTRIES:
            fn = getattr(handle, "hode_lstm_seq_" + name)
            setattr(self, "hode_lstm_" + name, fn if restype is C.c_size_t else self._checked(fn, "hode_lstm_seq_" + name))

    @staticmethod
    def _checked(fn, what):
        def call(*args):
            check(fn(*args), what)
            return 0
        return call


_as_libhode = None


def side_library():
    """libhode_lstm_seq.so under libhode.so's entry names (loads it on first use)."""
    global _as_libhode
    handle = lib()
    if _as_libhode is None or _as_libhode[0] is not handle:
        _as_libhode = (handle, _AsLibhode(handle))
    return _as_libhode[1]


def is_side_library(library):
    return isinstance(library, _AsLibhode)


def lstm_library(all_steps):
    """The library whose ``hode_lstm_*`` entries serve a call: libhode_lstm_seq.so when every step's hidden state is the
    output, libhode.so for the final state."""
    return side_library() if all_steps else L.lib()
