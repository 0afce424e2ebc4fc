"""ctypes binding of libhode_snf.so (C ABI: include/hode_snf.h), the Sylvester-flow posterior's own library.  Fails loudly
when the library is missing, stale or of another ABI version; nothing is loaded before the first use."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_SNF_ABI_VERSION = 1
MAX_LATENT, MAX_FLOWS, MAX_SAMPLES, MAX_HOUSEHOLDER = 32, 16, 256, 8
E_NULL, E_SIZE, E_WORKSPACE = -1, -2, -3

_fp = C.c_void_p  # device pointers travel as integers


class SnfDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("latent_dim", C.c_int32), ("n_flows", C.c_int32),
        ("n_samples", C.c_int32), ("s_kl", C.c_int32), ("n_householder", C.c_int32),
        ("mu", _fp), ("log_var", _fp), ("full_d", _fp), ("diag1", _fp), ("diag2", _fp), ("bias", _fp), ("v", _fp),
        ("noise", _fp), ("z_out", _fp), ("kl", _fp), ("workspace", _fp), ("workspace_bytes", C.c_size_t),
        ("grad_z_out", _fp), ("grad_kl", _fp),
        ("grad_mu", _fp), ("grad_log_var", _fp), ("grad_full_d", _fp), ("grad_diag1", _fp), ("grad_diag2", _fp),
        ("grad_bias", _fp), ("grad_v", _fp),
    ]


#: every symbol include/hode_snf.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_snf_version", C.c_int, ()),
    ("hode_snf_last_error_string", C.c_char_p, ()),
    ("hode_snf_workspace_bytes", C.c_size_t, (C.POINTER(SnfDesc),)),
    ("hode_snf_fwd", C.c_int, (C.POINTER(SnfDesc), C.c_void_p)),
    ("hode_snf_bwd", C.c_int, (C.POINTER(SnfDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_snf.so", "HODE_SNF_LIBRARY", EXPORTS, "hode_snf_version", "hode_snf_last_error_string",
                  HODE_SNF_ABI_VERSION, "the Sylvester-flow posterior on the device", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> SnfDesc:
    d = SnfDesc()
    d.struct_size = C.sizeof(SnfDesc)
    return d
