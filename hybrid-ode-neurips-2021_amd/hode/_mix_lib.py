"""ctypes binding of libhode_mix.so (C ABI: include/hode_mix.h), the two-model mixture CRPS's own library.  Fails loudly
when the library is missing, stale or of another ABI version."""

from __future__ import annotations

import ctypes as C
import os

from ._lib import HodeConfigError

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB_NAME = "libhode_mix.so"

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

_lib = None


def library_path() -> str:
    return os.environ.get("HODE_MIX_LIBRARY", os.path.join(_HERE, _LIB_NAME))


def _check_digest(path):
    """A library left over from other sources (e.g. after `git checkout`) is refused when the sources are there to compare."""
    stamp = path + ".digest"
    if "HODE_MIX_LIBRARY" in os.environ or not os.path.exists(stamp) or not os.path.exists(os.path.join(_ROOT, "build_hip.py")):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("_hode_build_hip", os.path.join(_ROOT, "build_hip.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
        want = mod.mix_source_digest()
    except OSError:
        return  # sources not shipped with the package
    if open(stamp).read().strip() != want:
        raise HodeConfigError("hode: %s is stale (its digest does not match csrc/mix/ and include/hode_mix.h) -- "
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
            "There is no CPU fallback for the mixture CRPS on the device." % path
        )
    _check_digest(path)
    handle = C.CDLL(path)
    for name, restype, argtypes in EXPORTS:
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)
    if handle.hode_mix_version() != HODE_MIX_ABI_VERSION:
        raise HodeConfigError("hode: mix ABI version %d != expected %d" % (handle.hode_mix_version(), HODE_MIX_ABI_VERSION))
    _lib = handle
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().hode_mix_last_error_string().decode("utf-8", "replace")
        raise HodeConfigError("%s failed (code %d): %s" % (what, code, msg))


def new_desc() -> MixCrpsDesc:
    d = MixCrpsDesc()
    d.struct_size = C.sizeof(MixCrpsDesc)
    return d
