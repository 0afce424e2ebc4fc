"""Is the device code of two built trees the same?  python tools/device_code_diff.py <tree A> <tree B>

For every object under csrc/**/build/ of both trees (experiment objects `<unit>__<tag>.o` aside): the .text bytes of its
gfx950 code object and every kernel descriptor.  Prints one row per unit and exits 1 on any difference or a unit that only
tree A has; a unit that only tree B has is listed as added.  Symbol names are
not compared (the compilation-unit id in them follows the source path).  A unit whose .text differs is looked at kernel by
kernel: if both trees hold the same kernels (by demangled name) with the same bytes and the same descriptors up to the
offset of the code, only their order in the section changed (the order in which the host code first names them; the
padding between them may change the section's length); the row
says so and the unit does not count as different."""
import glob, hashlib, os, struct, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_descriptor import B, code_object, kernel_descriptors

CSRC = os.path.join("hybrid-ode-neurips-2021_amd", "csrc")


def objects(tree):
    found = glob.glob(os.path.join(tree, CSRC, "build", "*.o")) + glob.glob(os.path.join(tree, CSRC, "*", "build", "*.o"))
    return {os.path.relpath(o, os.path.join(tree, CSRC)): o for o in found if "__" not in os.path.basename(o)}


def text_bytes(obj):
    """The .text section of the object's gfx950 code object; None for a host-only unit."""
    with tempfile.TemporaryDirectory(prefix="hode_dcd_") as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return None
        text = os.path.join(tmp, "text.bin")
        subprocess.run([B + "llvm-objcopy", "--dump-section", ".text=" + text, co, os.path.join(tmp, "dummy.co")], check=True)
        return open(text, "rb").read()


def kernels(obj):
    """{demangled kernel name: (code bytes, descriptor without kernel_code_entry_byte_offset)} of the object's code object."""
    with tempfile.TemporaryDirectory(prefix="hode_dcd_") as tmp:
        co = code_object(obj, tmp)
        syms = subprocess.run([B + "llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
        sec = subprocess.run([B + "llvm-readelf", "-S", "-W", co], capture_output=True, text=True, check=True).stdout
        data = open(co, "rb").read()
    f = [l.split("]", 1)[1].split() for l in sec.splitlines() if "] .text " in l][0]
    addr, off = int(f[2], 16), int(f[3], 16)
    code = {}
    for g in (l.split() for l in syms.splitlines()):
        if len(g) >= 8 and g[3] == "FUNC" and g[6] != "UND":
            v, n = int(g[1], 16), int(g[2])
            code[g[-1]] = data[off + v - addr: off + v - addr + n]
    names = subprocess.run(["c++filt"], input="\n".join(code) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    demangled = dict(zip(names, code.values()))
    out = {}
    for name, kd in kernel_descriptors(obj):
        out[name] = (demangled[name], kd[:16] + kd[24:])
    return out


if __name__ == "__main__":
    a, b = objects(sys.argv[1]), objects(sys.argv[2])
    bad = sorted(set(a) - set(b))   # a unit that is gone; units only tree B has are listed as added
    reordered = []
    print("%-40s %10s %8s  %-12s %s" % ("unit", ".text B", "kernels", ".text sha256", "result"))
    for unit in sorted(set(a) & set(b)):
        ta, tb = text_bytes(a[unit]), text_bytes(b[unit])
        ka, kb = sorted(kernel_descriptors(a[unit])), sorted(kernel_descriptors(b[unit]))
        same = ta == tb and ka == kb
        moved = not same and ta is not None and tb is not None and kernels(a[unit]) == kernels(b[unit])
        bad += [] if same or moved else [unit]
        reordered += [unit] if moved else []
        print("%-40s %10d %8d  %-12s %s" % (unit, len(ta or b""), len(ka), hashlib.sha256(ta or b"").hexdigest()[:12],
                                            "identical" if same else "same kernels, byte for byte, in another order" if moved
                                            else "DIFFERENT (text %s, descriptors %s)" % (ta == tb, ka == kb)))
    for unit in sorted(set(b) - set(a)):
        tb = text_bytes(b[unit])
        print("%-40s %10d %8d  %-12s %s" % (unit, len(tb or b""), len(kernel_descriptors(b[unit])),
                                            hashlib.sha256(tb or b"").hexdigest()[:12], "added"))
    ok = "all identical" if not reordered else "identical except for the order of the kernels in %s" % reordered
    print("%d units compared; %s" % (len(set(a) & set(b)), ok if not bad else "DIFFERENT or unmatched: %s" % bad))
    sys.exit(1 if bad else 0)
