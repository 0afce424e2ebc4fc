"""Registers, scratch and LDS of the twelve real_dose_bwd_kernel instantiations of libhode_real_dose.so and, beside each, of
the plain backward real_dims_kernel<HT, METHOD, true> of libhode_real_dims.so, read from the kernel descriptors of the
objects build_hip.py left in csrc/real_dose/build and csrc/real_dims/build: python tools/real_dose_kernel_resources.py
Writes profiles/real_dose_kernel_resources.txt.  No GPU."""
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import build_hip  # noqa: E402
from kernel_descriptor import kernel_descriptors  # noqa: E402


def rows(library, pattern):
    """{(HT, METHOD): (name, vgpr, agpr, scratch, lds)} of the kernels of `library` whose demangled name matches."""
    lib = build_hip.library(library)
    out = {}
    for unit, _, _ in lib.units():
        for name, kd in kernel_descriptors(os.path.join(lib.obj, unit + ".o")):
            m = re.search(pattern, name)
            if not m:
                continue
            lds, scratch = struct.unpack_from("<II", kd, 0)
            rsrc3, rsrc1 = struct.unpack_from("<II", kd, 44)
            total = ((rsrc1 & 63) + 1) * 8          # granulated allocation, arch + accumulation registers
            arch = ((rsrc3 & 63) + 1) * 4           # accum_offset: where the accumulation registers start
            out[(int(m.group(1)), int(m.group(2)))] = (m.group(0), arch, total - arch, scratch, lds)
    return out


def main():
    dose = rows("libhode_real_dose.so", r"hode::real_dose_bwd_kernel<(\d), (\d)>")
    plain = rows("libhode_real_dims.so", r"hode::real_dims_kernel<(\d), (\d), true>")
    assert len(dose) == len(plain) == 12
    lines = ["# libhode_real_dose.so: registers, scratch and LDS of the twelve backward instantiations, from the kernel descriptors",
             "# of the build (hipcc --offload-arch=gfx950 -O3); beside each, the plain backward of libhode_real_dims.so.",
             "# <HT, METHOD (0 euler, 1 midpoint, 2 rk4)>.  vgpr = arch registers up to the accumulation offset, agpr = the rest of",
             "# the granulated allocation (512 per SIMD lane; both kernels run one wave per SIMD); scratch = bytes per lane",
             "# (non-zero: the instantiation spills); lds = bytes per workgroup.",
             "%-36s %5s %5s %8s %6s   %-40s %5s %5s %8s %6s" % ("kernel", "vgpr", "agpr", "scratch", "lds", "plain backward", "vgpr", "agpr", "scratch", "lds")]
    for key in sorted(dose):
        lines.append("%-36s %5d %5d %8d %6d   %-40s %5d %5d %8d %6d" % (dose[key] + plain[key]))
    for what, table in (("real_dose_bwd_kernel", dose), ("real_dims_kernel<.., true>", plain)):
        spills = [r[0] for _, r in sorted(table.items()) if r[3]]
        lines.append("# %s: %d of 12 with scratch%s" % (what, len(spills), ": " + ", ".join(spills) if spills else ""))
    path = os.path.join(ROOT, "profiles", "real_dose_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
