"""ctypes binding of the test-only libhode_probe.so (include/hode_probe.h, csrc/probe/hode_probe.hip): each call runs one
shared device helper on torch tensors of the GPU and returns the result as a numpy array.  The op ids are read out of the
header, so the table here and the switch in the probe cannot drift apart unnoticed."""
import ctypes as C
import os
import re

import numpy as np

from hode._loader import Library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hode_probe.h")
FILE_NAME = "libhode_probe.so"


def header_defines(path=HEADER):
    """{name: int} of every `#define HODE_PROBE_<name> <int>` of the header."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define HODE_PROBE_(\w+) (-?\d+)\b", open(path).read(), flags=re.M)}


DEFINES = header_defines()
#: op name (lower case, without the prefix) -> id
OPS = {k[3:].lower(): v for k, v in DEFINES.items() if k.startswith("OP_")}

_fp, _ip = C.c_void_p, C.c_void_p
EXPORTS = (
    ("hode_probe_version", C.c_int, ()),
    ("hode_probe_last_error_string", C.c_char_p, ()),
    ("hode_probe_map", C.c_int, (C.c_int32, _fp, _fp, _fp, _fp, C.c_int64, C.c_void_p)),
    ("hode_probe_wave", C.c_int, (C.c_int32, _fp, _fp, C.c_int64, C.c_int32, C.c_void_p)),
    ("hode_probe_lanemap", C.c_int, (C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, C.c_void_p)),
    ("hode_probe_roundtrip", C.c_int, (C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_void_p)),
)
LIBRARY = Library(FILE_NAME, "HODE_PROBE_LIBRARY", EXPORTS, "hode_probe_version", "hode_probe_last_error_string",
                  DEFINES["ABI_VERSION"], "the device-helper probe", check_digest=True)


class Probe:
    """The loaded library and a device.  Inputs are numpy arrays; maps pad to a multiple of 64 with 1.0 and cut the result."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device, self.lib = torch, torch.device(device), LIBRARY.load()

    def _dev(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def map(self, op, a, b=None, c=None):
        n = len(a)
        pad = (-n) % 64
        ins = [None if v is None else self._dev(np.concatenate([np.asarray(v, np.float32), np.ones(pad, np.float32)])) for v in (a, b, c)]
        y = self.torch.empty(n + pad, dtype=self.torch.float32, device=self.device)
        ptrs = [None if t is None else t.data_ptr() for t in ins]
        LIBRARY.check(self.lib.hode_probe_map(OPS[op], ptrs[0], ptrs[1], ptrs[2], y.data_ptr(), n + pad, self._stream()), "hode_probe_map(%s)" % op)
        return y.cpu().numpy()[:n]

    def wave(self, op, x, block):
        xs = self._dev(x)
        y = self.torch.empty_like(xs)
        LIBRARY.check(self.lib.hode_probe_wave(OPS[op], xs.data_ptr(), y.data_ptr(), xs.numel(), block, self._stream()), "hode_probe_wave(%s)" % op)
        return y.cpu().numpy()

    def lanemap(self, lpp, B, ppw, block, n_blocks):
        out = self.torch.full((n_blocks * block, 3), -7, dtype=self.torch.int32, device=self.device)
        LIBRARY.check(self.lib.hode_probe_lanemap(lpp, B, ppw, block, n_blocks, out.data_ptr(), self._stream()), "hode_probe_lanemap")
        return out.cpu().numpy()

    def roundtrip(self, D, lpp, B, ppw, block, src, sentinel, guard=64):
        """dst is [guard | B * D | guard] floats pre-filled with `sentinel`; returns the whole buffer."""
        s = self._dev(src)
        buf = self.torch.full((2 * guard + B * D,), float(sentinel), dtype=self.torch.float32, device=self.device)
        dst = buf[guard:guard + B * D]
        LIBRARY.check(self.lib.hode_probe_roundtrip(D, lpp, B, ppw, block, s.data_ptr(), dst.data_ptr(), self._stream()), "hode_probe_roundtrip")
        return buf.cpu().numpy()
