"""ctypes binding of libhode_sylvester.so (C ABI: include/hode_sylvester.h), the Sylvester flows' own library.  Fails
loudly when the library is missing, stale or of another ABI version; nothing is loaded before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_SYLVESTER_ABI_VERSION = 1
MAX_LATENT, MAX_ORTHO, MAX_FLOWS, MAX_SAMPLES = 32, 32, 16, 256
E_NULL, E_SIZE, E_WORKSPACE = -1, -2, -3

_fp = C.c_void_p  # device pointers travel as integers


class SylvesterDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("latent_dim", C.c_int32), ("n_ortho", C.c_int32),
        ("n_flows", C.c_int32), ("n_samples", C.c_int32),
        ("z0", _fp), ("r1", _fp), ("r2", _fp), ("b", _fp), ("q", _fp), ("perm", _fp),
        ("z_out", _fp), ("logdet", _fp), ("log_diag", _fp), ("workspace", _fp), ("workspace_bytes", C.c_size_t),
        ("grad_z_out", _fp), ("grad_logdet", _fp), ("grad_log_diag", _fp),
        ("grad_z0", _fp), ("grad_r1", _fp), ("grad_r2", _fp), ("grad_b", _fp), ("grad_q", _fp),
    ]


#: every symbol include/hode_sylvester.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_sylvester_version", C.c_int, ()),
    ("hode_sylvester_last_error_string", C.c_char_p, ()),
    ("hode_sylvester_workspace_bytes", C.c_size_t, (C.POINTER(SylvesterDesc),)),
    ("hode_sylvester_fwd", C.c_int, (C.POINTER(SylvesterDesc), C.c_void_p)),
    ("hode_sylvester_bwd", C.c_int, (C.POINTER(SylvesterDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_sylvester.so", "HODE_SYLVESTER_LIBRARY", EXPORTS, "hode_sylvester_version",
                  "hode_sylvester_last_error_string", HODE_SYLVESTER_ABI_VERSION, "the Sylvester flows on the device",
                  check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> SylvesterDesc:
    d = SylvesterDesc()
    d.struct_size = C.sizeof(SylvesterDesc)
    return d
