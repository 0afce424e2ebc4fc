"""The one loader of the ctypes-bound kernel libraries (libhode.so and the side libraries built by build_hip.py): find the
file, refuse a stale one, bind the exports, compare the ABI version.  Fails loudly: a missing kernel library is an error."""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD_HIP = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "build_hip.py")
_build_hip = None  # build_hip.py as a module, executed at most once per process


class HodeConfigError(Exception):
    """Everything that is NOT the numerics' fault: a kernel library missing / stale / ABI mismatch, an argument error or
    unsupported shape reported by an entry point (HODE_E_*), a HIP launch error, CPU tensors handed to the GPU-only
    path.  Deliberately not a RuntimeError: the mirrored training loop must not mistake it for solver divergence,
    print it, save the untrained model and carry on."""


def _tree_digest(file_name):
    """build_hip.digest of the library as the sources in the tree would build it; None when they are not shipped."""
    global _build_hip
    if not os.path.exists(_BUILD_HIP):
        return None
    if _build_hip is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location("_hode_build_hip", _BUILD_HIP)
        _build_hip = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_build_hip)
    try:
        return _build_hip.digest(file_name)
    except OSError:
        return None


class Library:
    """One kernel library.  ``directory`` (where ``file_name`` is looked for unless the ``env`` variable names a file) and
    ``handle`` (the cached ctypes handle, None until loaded) are plain attributes: a test may point them elsewhere."""

    def __init__(self, file_name, env, exports, version_fn, error_fn, abi_version, noun, check_digest):
        self.file_name, self.env, self.exports = file_name, env, exports
        self.version_fn, self.error_fn, self.abi_version = version_fn, error_fn, abi_version
        self.noun, self.check_digest = noun, check_digest
        self.directory, self.handle = _HERE, None

    def path(self) -> str:
        return os.environ.get(self.env, os.path.join(self.directory, self.file_name))

    def _refuse_stale(self, path):
        """A library left over from other sources (e.g. after `git checkout`) is refused when it carries a stamp and the
        sources are there to compare.  A library named through the override variable is taken as it is."""
        stamp = path + ".digest"
        if self.env in os.environ or not os.path.exists(stamp):
            return
        want = _tree_digest(self.file_name)
        if want is not None and open(stamp).read().strip() != want:
            raise HodeConfigError("hode: %s is stale (its digest does not match the sources in the tree) -- "
                                  "rebuild with `python build_hip.py`" % path)

    def load(self):
        """Load (once) and return the ctypes handle; raises HodeConfigError if the library is absent, stale or of another ABI."""
        if self.handle is not None:
            return self.handle
        path = self.path()
        if not os.path.exists(path):
            raise HodeConfigError(
                "hode: %s not found -- build it with `python build_hip.py` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for %s." % (path, self.noun)
            )
        if self.check_digest:
            self._refuse_stale(path)
        handle = C.CDLL(path)
        for name, restype, argtypes in self.exports:
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype = restype
            fn.argtypes = list(argtypes)
        version = getattr(handle, self.version_fn)()
        if version != self.abi_version:
            raise HodeConfigError("hode: %s ABI version %d != expected %d" % (self.file_name, version, self.abi_version))
        self.handle = handle
        return handle

    def check(self, code: int, what: str):
        if code != 0:
            msg = getattr(self.load(), self.error_fn)().decode("utf-8", "replace")
            raise HodeConfigError("%s failed (code %d): %s" % (what, code, msg))
