"""VGPR allocation the kernel descriptors of an object's gfx950 code object REQUEST (granulated count, which the backend pads
to enforce `amdgpu_waves_per_eu`'s upper bound) next to what the code uses: python tools/kernel_descriptor.py <obj.o> <substr>

Importable: `kernel_descriptors(obj)` returns [(demangled kernel name, 64-byte kernel descriptor)] of the object's gfx950
code object; tests/test_kernel_variant_coverage.py reads the compiled template instantiations from it."""
import os, re, struct, subprocess, sys, tempfile
B = "/opt/rocm/lib/llvm/bin/"


def code_object(obj, tmp):
    """Path of the object's gfx950 code object, extracted into directory `tmp`; None for a host-only unit."""
    fb, co = os.path.join(tmp, "fb.bin"), os.path.join(tmp, "k.co")
    r = subprocess.run([B + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "fb_dummy.o")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if "not found" in r.stderr:
            return None  # no device code
        raise RuntimeError("llvm-objcopy %s: %s" % (obj, r.stderr))
    subprocess.run([B + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    return co


def kernel_descriptors(obj):
    with tempfile.TemporaryDirectory(prefix="hode_kd_") as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return []
        sec = subprocess.run([B + "llvm-readelf", "-S", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([B + "llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
        data = open(co, "rb").read()
    kd_syms = [(f[-1][:-3], int(f[1], 16)) for f in (line.split() for line in syms.splitlines())
               if len(f) >= 8 and f[-1].endswith(".kd")]
    if not kd_syms:
        return []  # device code without kernels (no descriptors, possibly no .rodata)
    m = re.search(r"\.rodata\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    kds = [(name, data[off + v - addr: off + v - addr + 64]) for name, v in kd_syms]
    names = subprocess.run(["c++filt"], input="\n".join(k for k, _ in kds) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    return list(zip(names, (kd for _, kd in kds)))


if __name__ == "__main__":
    obj, pat = sys.argv[1], sys.argv[2]
    for name, kd in kernel_descriptors(obj):
        if pat not in name:
            continue
        rsrc1 = struct.unpack_from("<I", kd, 48)[0]
        rsrc3 = struct.unpack_from("<I", kd, 44)[0]
        print("%-80s granulated vgpr alloc %3d (waves/SIMD <= %d), accum_offset %d" % (name[:80], ((rsrc1 & 63) + 1) * 8, min(8, 512 // (((rsrc1 & 63) + 1) * 8)), ((rsrc3 & 63) + 1) * 4))
