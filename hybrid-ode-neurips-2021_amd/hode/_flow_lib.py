"""ctypes binding of libhode_flow.so (C ABI: include/hode_flow.h), the planar-flow posterior's own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C

from ._loader import HodeConfigError, Library  # noqa: F401

HODE_FLOW_ABI_VERSION = 1
MAX_LATENT, MAX_FLOWS, MAX_SAMPLES = 32, 16, 256

_fp = C.c_void_p  # device pointers travel as integers


class FlowDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("latent_dim", C.c_int32), ("n_flows", C.c_int32),
        ("n_samples", C.c_int32), ("s_kl", C.c_int32),
        ("mu", _fp), ("log_var", _fp), ("u", _fp), ("w", _fp), ("b", _fp), ("noise", _fp), ("z_out", _fp), ("kl", _fp),
        ("grad_z_out", _fp), ("grad_kl", _fp), ("grad_mu", _fp), ("grad_log_var", _fp), ("grad_u", _fp),
        ("grad_w", _fp), ("grad_b", _fp),
    ]


#: every symbol include/hode_flow.h declares: (name, restype, argtypes)
EXPORTS = (
    ("hode_flow_version", C.c_int, ()),
    ("hode_flow_last_error_string", C.c_char_p, ()),
    ("hode_flow_fwd", C.c_int, (C.POINTER(FlowDesc), C.c_void_p)),
    ("hode_flow_bwd", C.c_int, (C.POINTER(FlowDesc), C.c_void_p)),
)

LIBRARY = Library("libhode_flow.so", "HODE_FLOW_LIBRARY", EXPORTS, "hode_flow_version", "hode_flow_last_error_string",
                   HODE_FLOW_ABI_VERSION, "the flow posterior on the device", check_digest=True)
lib, library_path, check = LIBRARY.load, LIBRARY.path, LIBRARY.check


def new_desc() -> FlowDesc:
    d = FlowDesc()
    d.struct_size = C.sizeof(FlowDesc)
    return d
