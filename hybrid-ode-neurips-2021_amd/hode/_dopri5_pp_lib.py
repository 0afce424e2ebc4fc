"""ctypes binding of libhode_dopri5_pp.so (C ABI: include/hode_dopri5_pp.h), the dopri5 solve of the hybrid Roche rhs with
per-patient step control.  Fails loudly when the library is missing, stale or of another ABI version; nothing is loaded
before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_DOPRI5_PP_ABI_VERSION = 1
#: latent sizes this library is compiled for (build_hip.DP_DIMS)
DIMS = (4, 6, 8, 12)

_fp = C.c_void_p  # device pointers travel as integers


class PpDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("rhs_kind", C.c_int32), ("batch", C.c_int32), ("latent_dim", C.c_int32),
        ("n_times", C.c_int32), ("n_dose", C.c_int32), ("need_theta_grad", C.c_int32), ("max_steps", C.c_int32),
        ("max_attempts", C.c_int32), ("flags", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
        ("t", _fp), ("y0", _fp), ("dosage", _fp), ("dose_times", _fp), ("theta", _fp), ("w1", _fp), ("b1", _fp), ("h", _fp),
        ("status", _fp), ("n_accepted", _fp), ("n_rejected", _fp), ("patient_status", _fp),
        ("grad_h", _fp), ("grad_y0", _fp), ("grad_w1", _fp), ("grad_b1", _fp), ("grad_theta", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_size_t),
    ]


_desc_p = C.POINTER(PpDesc)
#: every symbol include/hode_dopri5_pp.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_dopri5_pp_version", C.c_int, ()),
    ("hode_dopri5_pp_last_error_string", C.c_char_p, ()),
    ("hode_dopri5_pp_workspace_bytes", C.c_size_t, (_desc_p,)),
    ("hode_dopri5_pp_fwd", C.c_int, (_desc_p, C.c_void_p)),
    ("hode_dopri5_pp_bwd", C.c_int, (_desc_p, C.c_void_p)),
    ("hode_dopri5_pp_tape_offsets", C.c_int, (_desc_p, C.POINTER(C.c_size_t))),
)

LIBRARY = Library("libhode_dopri5_pp.so", "HODE_DOPRI5_PP_LIBRARY", EXPORTS, "hode_dopri5_pp_version",
                  "hode_dopri5_pp_last_error_string", HODE_DOPRI5_PP_ABI_VERSION,
                  "the dopri5 solve with per-patient step control", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> PpDesc:
    d = PpDesc()
    d.struct_size = C.sizeof(PpDesc)
    return d


def sizes_text():
    """What this library holds, for error messages."""
    return "the hybrid Roche rhs (RocheODE, ablate or not) at latent dimensions %s (libhode_dopri5_pp.so)" % ", ".join(map(str, DIMS))
