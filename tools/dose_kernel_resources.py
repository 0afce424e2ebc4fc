"""VGPR allocation, scratch and LDS of every dose_bwd_kernel instantiation of libhode_dose.so, read from the kernel
descriptors of the objects build_hip.py left in csrc/dose/build: python tools/dose_kernel_resources.py
Writes profiles/dose_kernel_resources.txt.  No GPU."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import build_hip  # noqa: E402
from kernel_descriptor import kernel_descriptors  # noqa: E402

METHODS = {0: "euler", 1: "midpoint", 2: "rk4"}


def rows():
    lib = build_hip.library("libhode_dose.so")
    out = []
    for unit, _, _ in lib.units():
        for name, kd in kernel_descriptors(os.path.join(lib.obj, unit + ".o")):
            lds, scratch = struct.unpack_from("<II", kd, 0)
            rsrc1 = struct.unpack_from("<I", kd, 48)[0]
            vgpr = ((rsrc1 & 63) + 1) * 8
            out.append((name.replace("void ", "").replace("(hode::DoseArgs)", ""), vgpr, min(8, 512 // vgpr), scratch, lds))
    return sorted(set(out), key=lambda r: [int(x) if x.isdigit() else x for x in r[0].replace("<", ",").replace(">", "").replace(" ", "").split(",")])


def main():
    lines = ["# libhode_dose.so: registers, scratch and LDS of every compiled kernel, from the kernel descriptors of the build",
             "# (hipcc --offload-arch=gfx950 -O3).  dose_bwd_kernel<D, METHOD (0 euler, 1 midpoint, 2 rk4), ABLATE, NEED_TH>.",
             "# vgpr = granulated allocation (arch + accumulation registers, 512 per SIMD lane); scratch = bytes per lane",
             "# (non-zero: the instantiation spills); lds = bytes per workgroup.",
             "%-58s %5s %11s %8s %5s" % ("kernel", "vgpr", "waves/SIMD", "scratch", "lds")]
    for name, vgpr, waves, scratch, lds in rows():
        lines.append("%-58s %5d %11d %8d %5d" % (name, vgpr, waves, scratch, lds))
    spills = [r for r in rows() if r[3]]
    lines.append("# %d kernels, %d with scratch%s" % (len(rows()), len(spills), ": " + ", ".join(r[0] for r in spills) if spills else ""))
    path = os.path.join(ROOT, "profiles", "dose_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
