"""ctypes binding of libhode_dose.so (C ABI: include/hode_dose.h), the fixed-grid adjoint of the hybrid Roche rhs that also
gives the gradient of every patient's dosage.  Fails loudly when the library is missing, stale or of another ABI version;
nothing is loaded before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_DOSE_ABI_VERSION = 1
#: latent sizes this library is compiled for (build_hip.DP_DIMS)
DIMS = (4, 6, 8, 12)
#: the fixed-grid methods it holds
METHODS = ("euler", "midpoint", "rk4")

_fp = C.c_void_p  # device pointers travel as integers


class DoseDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("rhs_kind", C.c_int32), ("method", C.c_int32), ("perturb", C.c_int32),
        ("batch", C.c_int32), ("latent_dim", C.c_int32), ("n_times", C.c_int32), ("n_dose", C.c_int32),
        ("need_theta_grad", C.c_int32), ("flags", C.c_int32),
        ("t", _fp), ("h", _fp), ("dosage", _fp), ("dose_times", _fp), ("theta", _fp), ("w1", _fp), ("b1", _fp), ("grad_h", _fp),
        ("grad_y0", _fp), ("grad_dosage", _fp), ("grad_w1", _fp), ("grad_b1", _fp), ("grad_theta", _fp), ("status", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_size_t),
    ]


_desc_p = C.POINTER(DoseDesc)
#: every symbol include/hode_dose.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_dose_version", C.c_int, ()),
    ("hode_dose_last_error_string", C.c_char_p, ()),
    ("hode_dose_workspace_bytes", C.c_size_t, (_desc_p,)),
    ("hode_dose_bwd", C.c_int, (_desc_p, C.c_void_p)),
)

LIBRARY = Library("libhode_dose.so", "HODE_DOSE_LIBRARY", EXPORTS, "hode_dose_version", "hode_dose_last_error_string",
                  HODE_DOSE_ABI_VERSION, "the fixed-grid adjoint with dose gradients", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> DoseDesc:
    d = DoseDesc()
    d.struct_size = C.sizeof(DoseDesc)
    return d


def sizes_text():
    """What this library holds, for error messages."""
    return "the hybrid Roche rhs (RocheODE, ablate or not) at latent dimensions %s with the methods euler / midpoint / rk4 " \
           "(libhode_dose.so)" % ", ".join(map(str, DIMS))
