"""ctypes binding of libhode_real_pp.so (C ABI: include/hode_real_pp.h), dopri5 with per-patient step control for the
real-data hybrid rhs, forward and discrete adjoint.  Fails loudly when the library is missing, stale or of another ABI
version; nothing is loaded before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_REAL_PP_ABI_VERSION = 1
#: latent sizes this library accepts (M = latent_dim - 4 GRU states in one ragged 16-row tile)
MIN_LATENT, MAX_LATENT = 5, 20
#: hidden sizes (one to four tiles of 16; build_hip.REAL_PP_HTS)
MAX_HIDDEN = 64

_fp = C.c_void_p  # device pointers travel as integers


class RealPpDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("latent_dim", C.c_int32), ("hidden_dim", C.c_int32),
        ("n_times", C.c_int32), ("n_action_times", C.c_int32), ("max_steps", C.c_int32), ("max_attempts", C.c_int32),
        ("flags", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
        ("t", _fp), ("y0", _fp), ("act", _fp), ("theta", _fp), ("wflat", _fp), ("h", _fp),
        ("status", _fp), ("n_accepted", _fp), ("n_rejected", _fp), ("patient_status", _fp),
        ("grad_h", _fp), ("grad_y0", _fp), ("grad_wflat", _fp), ("grad_theta", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_size_t),
    ]


_desc_p = C.POINTER(RealPpDesc)
#: every symbol include/hode_real_pp.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_real_pp_version", C.c_int, ()),
    ("hode_real_pp_last_error_string", C.c_char_p, ()),
    ("hode_real_pp_workspace_bytes", C.c_size_t, (_desc_p,)),
    ("hode_real_pp_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("hode_real_pp_bwd", C.c_int, (_desc_p, C.c_void_p)),
    ("hode_real_pp_tape_offsets", C.c_int, (_desc_p, C.POINTER(C.c_size_t))),
)

LIBRARY = Library("libhode_real_pp.so", "HODE_REAL_PP_LIBRARY", EXPORTS, "hode_real_pp_version",
                  "hode_real_pp_last_error_string", HODE_REAL_PP_ABI_VERSION,
                  "dopri5 of the real-data hybrid rhs with per-patient step control", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> RealPpDesc:
    d = RealPpDesc()
    d.struct_size = C.sizeof(RealPpDesc)
    return d


def sizes_text():
    """What this library holds, for error messages."""
    return "the real-data hybrid rhs (RocheODEReal) at latent dimensions %d .. %d with hidden_dim 1 .. %d and method dopri5 " \
           "with per-patient step control (libhode_real_pp.so)" % (MIN_LATENT, MAX_LATENT, MAX_HIDDEN)
