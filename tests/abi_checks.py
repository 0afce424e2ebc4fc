"""What the host tests of every kernel library check about its C ABI and its build stamp, once: the functions a header
declares, a struct's C layout against its ctypes mirror, the digest stamp against the tree, the loader's
missing -> stale -> current behaviour, the compiler's depfiles against the digest, and that importing loads nothing.
`library` arguments are hode._loader.Library instances (hode._mix_lib.LIBRARY, ...); tests/test_build_hip.py runs the
checks that are the same for every library over BINDINGS."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: every library of build_hip.LIBRARIES -> the module that binds it (its LIBRARY is the hode._loader.Library)
BINDINGS = {
    "libhode.so": "hode._lib",
    "libhode_flow.so": "hode._flow_lib",
    "libhode_mix.so": "hode._mix_lib",
    "libhode_blend.so": "hode._blend_lib",
    "libhode_datagen.so": "hode._datagen_lib",
    "libhode_probe.so": "device_probe",
    "libhode_neural_odd.so": "hode._neural_odd_lib",
    "libhode_roche_dims.so": "hode._roche_dims_lib",
    "libhode_real_dims.so": "hode._real_dims_lib",
    "libhode_lstm_seq.so": "hode._lstm_seq_lib",
    "libhode_real_step.so": "hode._real_step_lib",
    "libhode_sylvester.so": "hode._sylvester_lib",
    "libhode_snf.so": "hode._snf_lib",
    "libhode_dopri5_pp.so": "hode._dopri5_pp_lib",
}


def binding(file_name):
    """The hode._loader.Library that binds `file_name`."""
    return importlib.import_module(BINDINGS[file_name]).LIBRARY


def header_text(header):
    """include/<header> without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def declared_functions(header, prefix):
    """The names starting with `prefix` that include/<header> declares as functions."""
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % re.escape(prefix), header_text(header)))


def built(library):
    """The loaded handle of `library`, after building everything if its file is not there."""
    if not os.path.exists(library.path()):
        build_hip.build(verbose=False)
    return library.load()


def assert_c_layout(header, c_type, mirror, tmp_path):
    """sizeof(c_type) and the offset of EVERY field, as gcc lays include/<header> out, against the ctypes class `mirror`."""
    fields = [n for n, _ in mirror._fields_]
    src = tmp_path / ("layout_%s.c" % c_type)
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(%s));\n%s\nreturn 0;}\n'
                   % (os.path.join(ROOT, "include", header), c_type,
                      "\n".join('printf(" %%zu", offsetof(%s, %s));' % (c_type, f) for f in fields)))
    exe = tmp_path / ("layout_%s" % c_type)
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    nums = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert ctypes.sizeof(mirror) == nums[0], c_type
    assert [getattr(mirror, f).offset for f in fields] == nums[1:], c_type


def assert_digest_current(file_name):
    """The stamp build_hip.py wrote next to the library equals the digest of the sources in the tree."""
    out = build_hip.LIBRARIES[file_name].out
    if not os.path.exists(out):
        build_hip.build(verbose=False)
    assert os.path.exists(out + ".digest"), "%s has no source digest: rebuild with `python build_hip.py`" % file_name
    assert open(out + ".digest").read().strip() == build_hip.digest(file_name), "%s is stale: run `python build_hip.py`" % file_name


def assert_stale_library_is_refused(library, tmp_path, monkeypatch):
    """In an empty directory the library is "not found"; a copy with a foreign stamp is "stale"; with its own stamp it loads.
    Both messages name the file and the way out, the first also what has no CPU fallback."""
    from hode import HodeConfigError
    out = build_hip.LIBRARIES[library.file_name].out
    if not os.path.exists(out):
        build_hip.build(verbose=False)
    assert library.check_digest
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "directory", str(tmp_path))
    name = re.escape(library.file_name)
    with pytest.raises(HodeConfigError, match=r"%s not found -- build it with `python build_hip\.py`.*no CPU fallback for %s"
                       % (name, re.escape(library.noun))):
        library.load()
    shutil.copy(out, tmp_path / library.file_name)
    (tmp_path / (library.file_name + ".digest")).write_text("0" * 64 + "\n")
    with pytest.raises(HodeConfigError, match=r"%s is stale .*rebuild with `python build_hip\.py`" % name):
        library.load()
    shutil.copy(out + ".digest", tmp_path / (library.file_name + ".digest"))
    assert getattr(library.load(), library.version_fn)() == library.abi_version


def assert_depfiles_are_hashed(file_name):
    """The depfile hipcc left next to each object lists what the unit really included: all of it that lies in the
    repository must be in digest_files(), so that a new #include cannot escape the stamp.  A unit compiled while the tree
    lived elsewhere is checked too: the depfile's own entry of the unit's source tells where the tree was.  Returns the
    number of units checked: all of them, or none where no depfile is there (library shipped pre-built)."""
    lib = build_hip.LIBRARIES[file_name]
    hashed = set(build_hip.digest_files(file_name))
    checked = 0
    for unit, src, _ in lib.units():
        dfile = os.path.join(lib.obj, unit + ".d")
        if not os.path.exists(dfile):
            continue
        deps = {os.path.normpath(x) for x in open(dfile).read().replace("\\\n", " ").split() if not x.endswith(":")}
        tail = os.sep + os.path.relpath(src, ROOT)
        roots = {d[:-len(tail)] for d in deps if d.endswith(tail)}
        assert len(roots) == 1, (file_name, unit, sorted(roots))  # the unit's own source is among its dependencies, once
        root = roots.pop()
        inside = {os.path.relpath(d, root).replace(os.sep, "/") for d in deps if d.startswith(root + os.sep)}
        assert inside and inside <= hashed, (file_name, unit, sorted(inside - hashed))
        checked += 1
    assert checked in (0, len(lib.units())), (file_name, checked)
    return checked


def assert_import_does_not_load(binding_module_names, modules=("hode", "model", "flow")):
    """A fresh interpreter imports `modules`, every module of the hode package and the binding modules: no LIBRARY of the
    latter has a handle afterwards (a library is loaded at the first call that needs it)."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import importlib, os\n"
            "for m in %r: importlib.import_module(m)\n"
            "import hode\n"
            "for f in sorted(os.listdir(hode.__path__[0])):\n"
            "    if f.endswith('.py') and f != '__init__.py': importlib.import_module('hode.' + f[:-3])\n"
            "loaded = [b for b in %r if importlib.import_module(b).LIBRARY.handle is not None]\n"
            "assert not loaded, loaded\n"
            "print('ok')" % ([ROOT, os.path.join(ROOT, build_hip.PKG), os.path.join(ROOT, "tests")], tuple(modules),
                             tuple(binding_module_names)))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr[-2000:]
