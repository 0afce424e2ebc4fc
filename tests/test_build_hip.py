"""CPU checks of build_hip.py's digests (no GPU, no compiler): they do not depend on where the tree lives, and they cover
every file of the repository that a unit was compiled from."""
import importlib.util
import os
import shutil

import pytest

import build_hip

ROOT = build_hip.ROOT


def test_digests_do_not_depend_on_the_location_of_the_tree(tmp_path):
    """A library is built in one place and checked in another: a copy of the sources elsewhere has the same four digests."""
    shutil.copy(os.path.join(ROOT, "build_hip.py"), tmp_path / "build_hip.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    shutil.copytree(build_hip.CSRC, tmp_path / build_hip.PKG / "csrc", ignore=shutil.ignore_patterns("build"))
    spec = importlib.util.spec_from_file_location("_build_hip_copy", str(tmp_path / "build_hip.py"))
    copy = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(copy)
    assert copy.ROOT == str(tmp_path) != ROOT
    assert sorted(copy.LIBRARIES) == sorted(build_hip.LIBRARIES) == ["libhode.so", "libhode_blend.so", "libhode_flow.so", "libhode_mix.so"]
    for name in build_hip.LIBRARIES:
        assert copy.digest(name) == build_hip.digest(name), name
    assert copy.source_digest() == build_hip.digest("libhode.so")


def test_every_compiled_file_of_the_repository_is_in_its_library_digest():
    """The depfile hipcc left next to each object lists what the unit really included: all of it that lies in the
    repository must be hashed, so that a new #include cannot escape the stamp.  A unit compiled while the tree lived
    elsewhere is checked too: the depfile's own entry of the unit's source tells where the tree was."""
    checked = 0
    for name, lib in build_hip.LIBRARIES.items():
        hashed = set(build_hip.digest_files(name))
        for unit, src, _ in lib.units():
            dfile = os.path.join(lib.obj, unit + ".d")
            if not os.path.exists(dfile):
                continue
            deps = {os.path.normpath(x) for x in open(dfile).read().replace("\\\n", " ").split() if not x.endswith(":")}
            tail = os.sep + os.path.relpath(src, ROOT)
            roots = {d[:-len(tail)] for d in deps if d.endswith(tail)}
            assert len(roots) == 1, (name, unit, sorted(roots))  # the unit's own source is among its dependencies, once
            root = roots.pop()
            inside = {os.path.relpath(d, root).replace(os.sep, "/") for d in deps if d.startswith(root + os.sep)}
            assert inside and inside <= hashed, (name, unit, sorted(inside - hashed))
            checked += 1
    if not checked:
        pytest.skip("no depfile is there (library shipped pre-built)")
