"""ctypes binding of libhode_datagen.so (C ABI: include/hode_datagen.h), the synthetic data generator's own library.  Fails
loudly when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_DATAGEN_ABI_VERSION = 1
MAX_OBS, MAX_DOSES, N_THETA = 128, 8, 13
DIMS = (4, 6, 8, 12, 20)
E_NULL, E_SIZE, E_UNSUPPORTED = -1, -2, -3

_fp = C.c_void_p  # device pointers travel as integers


class DatagenDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_patients", C.c_int32), ("n_times", C.c_int32), ("latent_dim", C.c_int32),
        ("obs_dim", C.c_int32), ("n_dose", C.c_int32), ("max_steps", C.c_int32), ("flags", C.c_uint32),
        ("seed", C.c_uint64), ("step", C.c_double), ("rtol", C.c_double), ("atol", C.c_double), ("sigma", C.c_double),
        ("p_remove", C.c_double), ("theta", C.c_double * N_THETA),
        ("init", _fp), ("dose_times", _fp), ("dose_amount", _fp), ("ml_coef", _fp), ("output_coef", _fp), ("noise", _fp),
        ("latents", _fp), ("actions", _fp), ("measurements", _fp), ("masks", _fp), ("noise_out", _fp), ("status", _fp),
        ("steps", _fp), ("workspace", _fp), ("workspace_bytes", C.c_uint64),
    ]


#: every symbol include/hode_datagen.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_datagen_version", C.c_int, ()),
    ("hode_datagen_last_error_string", C.c_char_p, ()),
    ("hode_datagen_workspace_bytes", C.c_uint64, (C.c_int32, C.c_int32)),
    ("hode_datagen_generate", C.c_int, (C.POINTER(DatagenDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_datagen.so", "HODE_DATAGEN_LIBRARY", EXPORTS, "hode_datagen_version",
                  "hode_datagen_last_error_string", HODE_DATAGEN_ABI_VERSION, "the data generator on the device", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc():
    """A zeroed DatagenDesc with its struct_size set."""
    d = DatagenDesc()
    d.struct_size = C.sizeof(DatagenDesc)
    return d
