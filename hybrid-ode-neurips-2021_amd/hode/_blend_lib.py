"""ctypes binding of libhode_blend.so (C ABI: include/hode_blend.h), the real-data two-model scoring kernels' own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_BLEND_ABI_VERSION = 1
MAX_OBS, MAX_HORIZONS = 128, 8
E_NULL, E_SIZE = -1, -2

_fp = C.c_void_p  # device pointers travel as integers


class Nnls2Desc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32), ("rows", C.c_int64),
        ("step_stride_e", C.c_int64), ("step_stride_m", C.c_int64), ("step_stride_b", C.c_int64),
        ("x_e", _fp), ("x_m", _fp), ("truth", _fp), ("w", _fp),
    ]


class HorizonDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_times", C.c_int32), ("batch", C.c_int32), ("obs_dim", C.c_int32),
        ("n_horizons", C.c_int32), ("reserved", C.c_int32), ("horizons", C.c_int32 * MAX_HORIZONS),
        ("time_stride", C.c_int64), ("patient_stride", C.c_int64),
        ("x_e", _fp), ("x_m", _fp), ("w_e", _fp), ("w_m", _fp), ("truth", _fp), ("mask", _fp), ("sse", _fp), ("cnt", _fp),
    ]


#: every symbol include/hode_blend.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_blend_version", C.c_int, ()),
    ("hode_blend_last_error_string", C.c_char_p, ()),
    ("hode_blend_nnls2", C.c_int, (C.POINTER(Nnls2Desc), C.c_void_p)),
    ("hode_blend_horizon_sse", C.c_int, (C.POINTER(HorizonDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_blend.so", "HODE_BLEND_LIBRARY", EXPORTS, "hode_blend_version", "hode_blend_last_error_string",
                   HODE_BLEND_ABI_VERSION, "the blend kernels on the device", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc(cls):
    """A zeroed descriptor of class ``cls`` (Nnls2Desc, HorizonDesc) with its struct_size set."""
    d = cls()
    d.struct_size = C.sizeof(cls)
    return d
