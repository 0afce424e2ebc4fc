"""What the host tests of every kernel library check about its C ABI and its build stamp, once: the functions a header
declares, a struct's C layout against its ctypes mirror, the digest stamp against the tree, and the loader's
missing -> stale -> current behaviour.  `library` arguments are hode._loader.Library instances (hode._mix_lib.LIBRARY, ...)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """In an empty directory the library is "not found"; a copy with a foreign stamp is "stale"; with its own stamp it loads."""
    from hode import HodeConfigError
    out = build_hip.LIBRARIES[library.file_name].out
    if not os.path.exists(out):
        build_hip.build(verbose=False)
    monkeypatch.setattr(library, "handle", None)
    monkeypatch.setattr(library, "directory", str(tmp_path))
    with pytest.raises(HodeConfigError, match="not found"):
        library.load()
    shutil.copy(out, tmp_path / library.file_name)
    (tmp_path / (library.file_name + ".digest")).write_text("0" * 64 + "\n")
    with pytest.raises(HodeConfigError, match="stale"):
        library.load()
    shutil.copy(out + ".digest", tmp_path / (library.file_name + ".digest"))
    assert getattr(library.load(), library.version_fn)() == library.abi_version
