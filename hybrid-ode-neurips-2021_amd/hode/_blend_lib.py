"""ctypes binding of libhode_blend.so (C ABI: include/hode_blend.h), the real-data two-model scoring kernels' own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C
import os

from ._lib import HodeConfigError

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB_NAME = "libhode_blend.so"

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

_lib = None


def library_path() -> str:
    return os.environ.get("HODE_BLEND_LIBRARY", os.path.join(_HERE, _LIB_NAME))


def _check_digest(path):
    """A library left over from other sources (e.g. after `git checkout`) is refused when the sources are there to compare."""
    stamp = path + ".digest"
    if "HODE_BLEND_LIBRARY" in os.environ or not os.path.exists(stamp) or not os.path.exists(os.path.join(_ROOT, "build_hip.py")):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("_hode_build_hip", os.path.join(_ROOT, "build_hip.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
        want = mod.blend_source_digest()
    except OSError:
        return  # sources not shipped with the package
    if open(stamp).read().strip() != want:
        raise HodeConfigError("hode: %s is stale (its digest does not match csrc/blend/ and include/hode_blend.h) -- "
                              "rebuild with `python build_hip.py`" % path)


def lib():
    """Load (once) and return the ctypes handle; raises HodeConfigError if the library is absent, stale or of another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise HodeConfigError(
            "hode: %s not found -- build it with `python build_hip.py` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the blend kernels on the device." % path
        )
    _check_digest(path)
    handle = C.CDLL(path)
    for name, restype, argtypes in EXPORTS:
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)
    if handle.hode_blend_version() != HODE_BLEND_ABI_VERSION:
        raise HodeConfigError("hode: blend ABI version %d != expected %d" % (handle.hode_blend_version(), HODE_BLEND_ABI_VERSION))
    _lib = handle
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().hode_blend_last_error_string().decode("utf-8", "replace")
        raise HodeConfigError("%s failed (code %d): %s" % (what, code, msg))


def new_desc(cls):
    """A zeroed descriptor of class ``cls`` (Nnls2Desc, HorizonDesc) with its struct_size set."""
    d = cls()
    d.struct_size = C.sizeof(cls)
    return d
