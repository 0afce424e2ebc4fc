"""CPU checks of build_hip.py that are the same for every library (no GPU, no compiler): the table and its rows, the
digests (they do not depend on where the tree lives, they cover every file a unit was compiled from, they follow an edit of
any of those files and of no other), the stamp next to each library and the loader's refusal of a missing or stale copy, and
that importing the package loads nothing.  What is particular to one library is in its own tests/test_*_host.py."""
import importlib.util
import os
import shutil

import pytest

import abi_checks
import build_hip

ROOT = build_hip.ROOT
CSRC = build_hip.PKG + "/csrc/"
LIBS = list(build_hip.LIBRARIES)
#: shared sources whose edit a library's digest was already known to follow, by name (each is asserted to be in
#: digest_files(), and test_digest_follows_an_edit_of_each_of_its_files_and_of_no_other edits every file of that list)
FOLLOWED = {
    "libhode_roche_dims.so": ["hode_roche.hpp", "hode_rk_host.hpp", "hode_rk_kernels.hpp", "hode_dopri5.hip",
                              "roche_dims/hode_roche_dims.hpp"],
    "libhode_real_dims.so": ["hode_real_mf.hpp", "hode_real_args.hpp", "hode_common.hpp", "real_dims/hode_real_dims.hpp"],
    "libhode_lstm_seq.so": ["hode_lstm_kernels.hpp", "hode_lstm_bwd_body.hpp", "hode_lstm_fwd_body.hpp", "hode_lstm.hip",
                            "hode_lstm_tpw.hip", "lstm_seq/hode_lstm_seq.hip"],
}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def copy(tmp_path_factory):
    """build_hip.py of a copy of the sources elsewhere.  A test that edits a file of the copy puts it back."""
    tmp = tmp_path_factory.mktemp("tree")
    shutil.copy(os.path.join(ROOT, "build_hip.py"), tmp / "build_hip.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp / "include")
    shutil.copytree(build_hip.CSRC, tmp / build_hip.PKG / "csrc", ignore=shutil.ignore_patterns("build"))
    module = _load(str(tmp / "build_hip.py"), "_build_hip_copy")
    assert module.ROOT == str(tmp) != ROOT
    return module


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_holds_these_libraries():
    assert sorted(build_hip.LIBRARIES) == [
        "libhode.so", "libhode_blend.so", "libhode_datagen.so", "libhode_dopri5_pp.so", "libhode_flow.so", "libhode_lstm_seq.so",
        "libhode_mix.so", "libhode_neural_odd.so", "libhode_probe.so", "libhode_real_dims.so", "libhode_real_step.so",
        "libhode_roche_dims.so", "libhode_snf.so", "libhode_sylvester.so"]
    assert LIBS[0] == "libhode.so" and (build_hip.OUT, build_hip.OBJ) == (build_hip.LIBRARIES["libhode.so"].out, build_hip.LIBRARIES["libhode.so"].obj)


def test_every_library_has_a_binding_module():
    """A library added to the table without a line in abi_checks.BINDINGS gets none of the checks below: it fails here."""
    assert set(abi_checks.BINDINGS) == set(build_hip.LIBRARIES)
    for name in LIBS:
        assert abi_checks.binding(name).file_name == name
        assert abi_checks.binding(name).env == name[3:-3].upper() + "_LIBRARY"   # HODE_LIBRARY, HODE_FLOW_LIBRARY, ...
    # libhode.so is checked by tests/test_abi.py and loaded with HODE_LIBRARY variants; every other library refuses a stale copy
    assert [name for name in LIBS if not abi_checks.binding(name).check_digest] == ["libhode.so"]


@pytest.mark.parametrize("name", LIBS)
def test_row_shape(name):
    row = build_hip.LIBRARIES[name]
    assert row.name == name and row.out == os.path.join(ROOT, build_hip.PKG, "hode", name)
    assert row.obj == os.path.join(ROOT, row.src_dir, "build") and os.path.isdir(os.path.join(ROOT, row.src_dir))
    assert row.header.startswith("include/") and os.path.isfile(os.path.join(ROOT, row.header))
    units = row.units()
    assert units and len({n for n, _, _ in units}) == len(units)   # objects are <obj>/<unit name>.o
    for _, src, flags in units:
        assert os.path.isfile(src) and src.startswith(build_hip.CSRC + os.sep) and isinstance(flags, list)


# ------------------------------------------------------------------------------------------------------ the digests
@pytest.mark.parametrize("name", LIBS)
def test_digest_does_not_depend_on_the_location_of_the_tree(copy, name):
    """A library is built in one place and checked in another: a copy of the sources elsewhere has the same digest."""
    assert list(copy.LIBRARIES) == LIBS
    assert copy.digest_files(name) == build_hip.digest_files(name) == sorted(build_hip.digest_files(name))
    assert copy.digest(name) == build_hip.digest(name)
    assert copy.source_digest() == build_hip.digest("libhode.so")


@pytest.mark.parametrize("name", LIBS)
def test_every_compiled_file_of_the_repository_is_in_the_library_digest(name):
    """The compiler's own list against digest_files(): the evidence that the scan of the #include lines misses nothing."""
    if not abi_checks.assert_depfiles_are_hashed(name):
        pytest.skip("no depfile is there (library shipped pre-built)")


@pytest.mark.parametrize("name", LIBS)
def test_digest_follows_an_edit_of_each_of_its_files_and_of_no_other(copy, name):
    files = copy.digest_files(name)
    row = copy.LIBRARIES[name]
    sources = {os.path.relpath(s, copy.ROOT).replace(os.sep, "/") for _, s, _ in row.units()}
    assert {row.header} | sources <= set(files)
    for f in FOLLOWED.get(name, ()):
        assert CSRC + f in files, f
    before = copy.digest(name)
    assert before == build_hip.digest(name)

    def edited(paths):
        kept = {p: open(os.path.join(copy.ROOT, p), "rb").read() for p in paths}
        try:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text + b"\n")
            return copy.digest(name)
        finally:
            for p, text in kept.items():
                open(os.path.join(copy.ROOT, p), "wb").write(text)

    for f in files:
        assert edited([f]) != before, f
    others = [os.path.relpath(os.path.join(d, f), copy.ROOT).replace(os.sep, "/")
              for top in ("include", build_hip.PKG) for d, _, fs in os.walk(os.path.join(copy.ROOT, top)) for f in fs]
    others = sorted(set(others) - set(files))
    assert others and edited(others) == before, name
    assert copy.digest(name) == before   # the copy is as it was


# ------------------------------------------------------------------------------------ the stamp, the loader, the import
@pytest.mark.parametrize("name", LIBS)
def test_library_digest_matches_sources(name):
    abi_checks.assert_digest_current(name)


@pytest.mark.parametrize("name", LIBS[1:])
def test_a_missing_and_a_stale_library_are_refused_with_a_message(name, tmp_path, monkeypatch):
    abi_checks.assert_stale_library_is_refused(abi_checks.binding(name), tmp_path, monkeypatch)


def test_importing_the_package_does_not_load_a_library():
    abi_checks.assert_import_does_not_load(abi_checks.BINDINGS.values())
