"""ctypes binding of libhode_flow.so (C ABI: include/hode_flow.h), the planar-flow posterior's own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C
import os

from ._lib import HodeConfigError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libhode_flow.so"

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

_lib = None


def library_path() -> str:
    return os.environ.get("HODE_FLOW_LIBRARY", os.path.join(_HERE, _LIB_NAME))


def lib():
    """Load (once) and return the ctypes handle; raises HodeConfigError if the library is absent or of another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise HodeConfigError(
            "hode: %s not found -- build it with `python build_hip.py` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the flow posterior on the device." % path
        )
    handle = C.CDLL(path)
    for name, restype, argtypes in EXPORTS:
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)
    if handle.hode_flow_version() != HODE_FLOW_ABI_VERSION:
        raise HodeConfigError("hode: flow ABI version %d != expected %d" % (handle.hode_flow_version(), HODE_FLOW_ABI_VERSION))
    _lib = handle
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().hode_flow_last_error_string().decode("utf-8", "replace")
        raise HodeConfigError("%s failed (code %d): %s" % (what, code, msg))


def new_desc() -> FlowDesc:
    d = FlowDesc()
    d.struct_size = C.sizeof(FlowDesc)
    return d
