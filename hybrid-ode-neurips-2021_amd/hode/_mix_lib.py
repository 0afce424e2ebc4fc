"""ctypes binding of libhode_mix.so (C ABI: include/hode_mix.h), the two-model mixture CRPS's own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_MIX_ABI_VERSION = 1
MAX_DIM = 128
E_NULL, E_SIZE, E_UNSUPPORTED = -1, -2, -3

_fp = C.c_void_p  # device pointers travel as integers


class MixCrpsDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_times", C.c_int32), ("batch", C.c_int32), ("n_members", C.c_int32),
        ("obs_dim", C.c_int32), ("latent_dim_e", C.c_int32), ("latent_dim_m", C.c_int32), ("reserved", C.c_int32),
        ("time_stride_e", C.c_int64), ("member_stride_e", C.c_int64), ("patient_stride_e", C.c_int64),
        ("time_stride_m", C.c_int64), ("member_stride_m", C.c_int64), ("patient_stride_m", C.c_int64),
        ("h_e", _fp), ("h_m", _fp), ("w_e", _fp), ("b_e", _fp), ("w_m", _fp), ("b_m", _fp), ("mix_e", _fp), ("mix_m", _fp),
        ("truth", _fp), ("crps", _fp), ("crps_sum", _fp),
    ]


#: every symbol include/hode_mix.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_mix_version", C.c_int, ()),
    ("hode_mix_last_error_string", C.c_char_p, ()),
    ("hode_mix_crps", C.c_int, (C.POINTER(MixCrpsDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_mix.so", "HODE_MIX_LIBRARY", EXPORTS, "hode_mix_version", "hode_mix_last_error_string",
                   HODE_MIX_ABI_VERSION, "the mixture CRPS on the device", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> MixCrpsDesc:
    d = MixCrpsDesc()
    d.struct_size = C.sizeof(MixCrpsDesc)
    return d
