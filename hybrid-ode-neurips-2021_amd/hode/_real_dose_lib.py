"""ctypes binding of libhode_real_dose.so (C ABI: include/hode_real_dose.h), the fixed-grid adjoint of the real-data hybrid
rhs that also gives the gradient of the table of hourly doses.  Fails loudly when the library is missing, stale or of another
ABI version; nothing is loaded before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_REAL_DOSE_ABI_VERSION = 1
#: latent sizes this library accepts (M = latent_dim - 4 GRU states in one ragged 16-row tile)
MIN_LATENT, MAX_LATENT = 5, 20
#: hidden sizes (one to four tiles of 16; build_hip.REAL_DOSE_HTS)
MAX_HIDDEN = 64
#: the fixed-grid methods it holds
METHODS = ("euler", "midpoint", "rk4")

_fp = C.c_void_p  # device pointers travel as integers


class RealDoseDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("method", C.c_int32), ("perturb", C.c_int32), ("batch", C.c_int32),
        ("latent_dim", C.c_int32), ("hidden_dim", C.c_int32), ("n_times", C.c_int32), ("n_action_times", C.c_int32),
        ("flags", C.c_int32),
        ("t", _fp), ("h", _fp), ("act", _fp), ("theta", _fp), ("wflat", _fp), ("grad_h", _fp),
        ("grad_y0", _fp), ("grad_act", _fp), ("grad_wflat", _fp), ("grad_theta", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_size_t),
    ]


_desc_p = C.POINTER(RealDoseDesc)
#: every symbol include/hode_real_dose.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_real_dose_version", C.c_int, ()),
    ("hode_real_dose_last_error_string", C.c_char_p, ()),
    ("hode_real_dose_workspace_bytes", C.c_size_t, (_desc_p,)),
    ("hode_real_dose_bwd", C.c_int, (_desc_p, C.c_void_p)),
)

LIBRARY = Library("libhode_real_dose.so", "HODE_REAL_DOSE_LIBRARY", EXPORTS, "hode_real_dose_version",
                  "hode_real_dose_last_error_string", HODE_REAL_DOSE_ABI_VERSION,
                  "the real-data fixed-grid adjoint with dose-table gradients", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> RealDoseDesc:
    d = RealDoseDesc()
    d.struct_size = C.sizeof(RealDoseDesc)
    return d


def sizes_text():
    """What this library holds, for error messages."""
    return "the real-data hybrid rhs (RocheODEReal) at latent dimensions %d .. %d with hidden_dim 1 .. %d and the methods " \
           "euler / midpoint / rk4 (libhode_real_dose.so)" % (MIN_LATENT, MAX_LATENT, MAX_HIDDEN)
