#!/usr/bin/env python
"""Build the gfx950 kernel libraries in-tree with hipcc: `python build_hip.py [-j N] [--force]`.

LIBRARIES has one row per library: its file name in hode/, the directory of its sources, its C ABI header and its compile
units; MORE_LIBRARIES, LATER_LIBRARIES and PATIENT_LIBRARIES hold further rows of the same type, and library(name) looks a row up in all four.
build() compiles the units of every row (built_libraries()) in one thread pool (a unit is recompiled when a file of its depfile, its flags
or this script changed), links each library whose objects are newer than it, and writes digest(<library>) next to it as
<library>.so.digest; tests and hode/_loader.py compare that stamp with the tree.  The digest covers the header, every source
of the row's directory, the units' sources and everything they include from inside the tree, the flags and the units."""
import argparse
import concurrent.futures as cf
import hashlib
import os
import posixpath
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = "hybrid-ode-neurips-2021_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-variable",
         "-Wno-unused-but-set-variable"]
RK_DIMS = (4, 6, 8, 12, 20)
DP_DIMS = (4, 6, 8, 12)
NEURAL_ODD_DIMS = (5, 7, 9, 11, 13, 15)  # csrc/neural_odd/hode_neural_odd_dim.hip; the even ones are in libhode.so
ROCHE_DIMS = (5, 7, 9, 10, 11, 13, 14, 15, 16)  # csrc/roche_dims/: the hybrid decoder beside RK_DIMS / DP_DIMS
REAL_DIMS_HTS = (1, 2, 3, 4)  # csrc/real_dims/hode_real_dims_ht.hip: hidden tiles of 16 (hidden_dim 1 .. 64)
REAL_STEP_HTS = (1, 2, 3, 4)  # csrc/real_step/hode_real_step_ht.hip: the same tiles for the one-step-ahead solve
REAL_DOSE_HTS = (1, 2, 3, 4)  # csrc/real_dose/hode_real_dose_ht.hip: the same tiles for the adjoint with dose-table gradients
REAL_PP_HTS = (1, 2, 3, 4)  # csrc/real_pp/hode_real_pp_ht.hip: the same tiles for dopri5 with per-patient step control
LSTM_TPWS = (1, 2, 3, 4, 5, 6, 8, 10)   # padded hidden sizes 16 * TPW (csrc/hode_lstm_tpw.hip)
# per-unit flags (measured on MI355X)
# -fno-slp-vectorize on the split kernels: packed-fp32 pairing costs more v_mov than it saves (step 0.228 -> 0.207 ms)
EXTRA_FLAGS = {"hode_rk_split": os.environ.get("HODE_SPLIT_FLAGS", "-fno-slp-vectorize").split()}
DP_FLAGS = os.environ.get("HODE_DP_FLAGS", "").split()  # experiments on the dopri5 units only; product builds: empty
EXTRA_FLAGS["hode_dopri5"] = DP_FLAGS
EXTRA_FLAGS["hode_lstm"] = os.environ.get("HODE_LSTM_FLAGS", "").split()  # diagnostics (-DHODE_LSTM_STAMPS); product builds: empty


def units():
    u = [("hode_api", os.path.join(CSRC, "hode_api.hip"), [])]
    for d in RK_DIMS:
        u.append(("hode_rk_d%d" % d, os.path.join(CSRC, "hode_rk_dim.hip"), ["-DHODE_DIM=%d" % d]))
    for d in DP_DIMS:
        u.append(("hode_dp_d%d" % d, os.path.join(CSRC, "hode_dopri5_dim.hip"), ["-DHODE_DIM=%d" % d] + DP_FLAGS))
    for n in LSTM_TPWS:
        u.append(("hode_lstm_tpw%d" % n, os.path.join(CSRC, "hode_lstm_tpw.hip"), ["-DHODE_LSTM_TPW=%d" % n] + EXTRA_FLAGS["hode_lstm"]))
    for name in ("hode_dopri5", "hode_lstm", "hode_neural", "hode_real", "hode_rk_mf", "hode_readout", "hode_rk_split", "hode_crps", "hode_mckl", "hode_neural_mf", "hode_real_mf", "hode_neural_dopri5", "hode_readout_mlp", "hode_seqdec", "hode_neural_real_mf"):
        u.append((name, os.path.join(CSRC, name + ".hip"), EXTRA_FLAGS.get(name, [])))
    return u


def _neural_odd_units():
    d = os.path.join(CSRC, "neural_odd")
    return [("hode_neural_odd", os.path.join(d, "hode_neural_odd.hip"), [])] + \
        [("hode_neural_odd_d%d" % n, os.path.join(d, "hode_neural_odd_dim.hip"), ["-DHODE_DIM=%d" % n]) for n in NEURAL_ODD_DIMS]


def _roche_dims_units():
    d = os.path.join(CSRC, "roche_dims")
    return [("hode_roche_dims", os.path.join(d, "hode_roche_dims.hip"), []),
            # the dopri5 entries: libhode.so's unit compiled for this library (its checks, layout and attempt loop, once)
            ("hode_roche_dims_dopri5", os.path.join(CSRC, "hode_dopri5.hip"), ["-DHODE_ROCHE_DIMS_UNIT"])] + \
        [("hode_roche_dims_rk_d%d" % n, os.path.join(d, "hode_roche_dims_rk_dim.hip"), ["-DHODE_DIM=%d" % n]) for n in ROCHE_DIMS] + \
        [("hode_roche_dims_dp_d%d" % n, os.path.join(d, "hode_roche_dims_dp_dim.hip"), ["-DHODE_DIM=%d" % n]) for n in ROCHE_DIMS]


def _lstm_seq_units():
    # libhode.so's LSTM units compiled for this library (its checks, geometry, packing and launch code, once)
    seq = ["-DHODE_LSTM_SEQ_UNIT"]
    return [("hode_lstm_seq", os.path.join(CSRC, "lstm_seq", "hode_lstm_seq.hip"), []),
            ("hode_lstm_seq_host", os.path.join(CSRC, "hode_lstm.hip"), seq)] + \
        [("hode_lstm_seq_tpw%d" % n, os.path.join(CSRC, "hode_lstm_tpw.hip"), seq + ["-DHODE_LSTM_TPW=%d" % n]) for n in LSTM_TPWS]


def _dose_units():
    d = os.path.join(CSRC, "dose")
    # -Wno-unused-function: hode_rk_host.hpp is included for the grid shape and the partial fold; its argument helpers are not called here
    return [("hode_dose", os.path.join(d, "hode_dose.hip"), ["-Wno-unused-function"])] + \
        [("hode_dose_d%d" % n, os.path.join(d, "hode_dose_dim.hip"), ["-DHODE_DIM=%d" % n]) for n in DP_DIMS]


def _dopri5_pp_units():
    d = os.path.join(CSRC, "dopri5_pp")
    # -Wno-unused-function: hode_rk_host.hpp is included for the partial fold; its Roche argument helpers are not called here
    return [("hode_dopri5_pp", os.path.join(d, "hode_dopri5_pp.hip"), ["-Wno-unused-function"])] + \
        [("hode_dopri5_pp_d%d" % n, os.path.join(d, "hode_dopri5_pp_dim.hip"), ["-DHODE_DIM=%d" % n]) for n in DP_DIMS]


class Library:
    """One row of LIBRARIES: the file name of the library in hode/ and what it is built from.  `src_dir` and `header` are
    relative to the repository root and use "/", so that digest() is the same wherever the tree lives; `units` is a callable
    returning [(unit name, absolute source path, extra flags)]; objects go to <src_dir>/build."""

    def __init__(self, name, src_dir, header, units):
        self.name, self.src_dir, self.header, self.units = name, src_dir, header, units
        self.out = os.path.join(ROOT, PKG, "hode", name)
        self.obj = os.path.join(ROOT, src_dir, "build")


def _side(name):
    """A side library of one unit: csrc/<name>/hode_<name>.hip, with the C ABI header include/hode_<name>.h."""
    d = PKG + "/csrc/" + name
    unit = ("hode_" + name, os.path.join(ROOT, d, "hode_%s.hip" % name), [])
    return Library("libhode_%s.so" % name, d, "include/hode_%s.h" % name, lambda: [unit])


def _multi(name, units):
    """A library of several units: sources in csrc/<name>/ (and what `units` names elsewhere), header include/hode_<name>.h."""
    return Library("libhode_%s.so" % name, PKG + "/csrc/" + name, "include/hode_%s.h" % name, units)


def _real_side(name, hts):
    """A side library of the real-data hybrid rhs (csrc/hode_real_side_host.hpp): csrc/<name>/ with the entry points in
    hode_<name>.hip and hode_<name>_ht.hip compiled once per hidden-tile count of `hts`."""
    d = os.path.join(CSRC, name)

    def units():
        # -Wno-unused-function: hode_rk_host.hpp is included for the partial fold; its Roche argument helpers are not called here
        return [("hode_" + name, os.path.join(d, "hode_%s.hip" % name), ["-Wno-unused-function"])] + \
            [("hode_%s_ht%d" % (name, n), os.path.join(d, "hode_%s_ht.hip" % name), ["-DHODE_%s_HT=%d" % (name.upper(), n)]) for n in hts]
    return _multi(name, units)


#: every library, by file name, in build order
LIBRARIES = {lib.name: lib for lib in (
    Library("libhode.so", PKG + "/csrc", "include/hode.h", units),  # the solvers, the LSTM, the readouts and the metrics
    _side("flow"),                            # the planar-flow posterior
    _side("mix"),                             # the two-model mixture CRPS
    _side("blend"),                           # the real-data two-model scoring kernels
    _side("datagen"),                         # the synthetic data generator (DataGeneratorRoche)
    _side("probe"),                           # test only: the shared device helpers on their own; nothing under hode/ loads it
    _multi("neural_odd", _neural_odd_units),  # the NeuralODE kernels at the odd latent sizes 5 .. 15, a unit per size
    _multi("roche_dims", _roche_dims_units),  # the hybrid Roche kernels at ROCHE_DIMS, a fixed-grid and a dopri5 unit per size
    _real_side("real_dims", REAL_DIMS_HTS),   # the real-data hybrid rhs at the latent sizes 5 .. 20, a unit per hidden-tile count
    _multi("lstm_seq", _lstm_seq_units),      # the LSTM kernels with the hidden state of every step: libhode.so's units again
    _real_side("real_step", REAL_STEP_HTS),   # the one-step-ahead solve of the real-data hybrid rhs, a unit per hidden-tile count
    _side("sylvester"),                       # the chain of Sylvester flows (flow.Sylvester, flow.sylvester_chain)
    _side("snf"),                             # the Sylvester-flow posterior with its Monte-Carlo KL (EncoderSylvesterLSTM)
    _multi("dopri5_pp", _dopri5_pp_units),    # dopri5 of the hybrid Roche rhs with per-patient step control, a unit per DP_DIMS
)}
#: libraries beside that table (its keys are pinned by tests/test_build_hip.py), built, linked and stamped with it
MORE_LIBRARIES = {lib.name: lib for lib in (
    _multi("dose", _dose_units),              # the fixed-grid adjoint of the hybrid Roche rhs with dose gradients, a unit per DP_DIMS
)}


#: libraries beside both (all_libraries() is pinned by tests/test_dose_host.py), built, linked and stamped with them
LATER_LIBRARIES = {lib.name: lib for lib in (
    _real_side("real_dose", REAL_DOSE_HTS),   # the adjoint of the real-data hybrid rhs with dose-table gradients, a unit per hidden-tile count
)}


#: libraries beside all three (every_library() is pinned by tests/test_real_dose_host.py), built, linked and stamped with them
PATIENT_LIBRARIES = {lib.name: lib for lib in (
    _real_side("real_pp", REAL_PP_HTS),       # dopri5 of the real-data hybrid rhs with per-patient step control, a unit per hidden-tile count
)}


def library(name):
    """The row of `name`, from LIBRARIES, MORE_LIBRARIES, LATER_LIBRARIES or PATIENT_LIBRARIES."""
    for table in (LIBRARIES, MORE_LIBRARIES, LATER_LIBRARIES):
        if name in table:
            return table[name]
    return PATIENT_LIBRARIES[name]


def all_libraries():
    """Every row of the first two tables, in build order."""
    return list(LIBRARIES.values()) + list(MORE_LIBRARIES.values())


def every_library():
    """Every row of the first three tables, in build order."""
    return all_libraries() + list(LATER_LIBRARIES.values())


def built_libraries():
    """Every row of all four tables, in build order: what build() compiles, links and stamps."""
    return every_library() + list(PATIENT_LIBRARIES.values())


OUT = LIBRARIES["libhode.so"].out
OBJ = LIBRARIES["libhode.so"].obj
_INCLUDE = re.compile(rb'^\s*#include\s+"([^"]+)"', re.M)


def _digest_sources(lib):
    """{name relative to the repository root: contents} of what `lib` is built from: the ABI header, every source of
    `src_dir`, the units' sources, and whatever these include in quotes, transitively, each name resolved against the
    including file.  An #include under #if counts (a superset is safe); one that leaves the tree or names no file does not."""
    lib = library(lib)
    todo = [lib.src_dir + "/" + f for f in os.listdir(os.path.join(ROOT, lib.src_dir)) if f.endswith((".hpp", ".hip", ".h"))]
    todo += [lib.header] + [os.path.relpath(s, ROOT).replace(os.sep, "/") for _, s, _ in lib.units()]
    files = {}
    while todo:
        f = todo.pop()
        if f in files:
            continue
        files[f] = open(os.path.join(ROOT, f), "rb").read()
        for inc in _INCLUDE.findall(files[f]):
            g = posixpath.normpath(posixpath.join(posixpath.dirname(f), inc.decode()))
            if not g.startswith("../") and os.path.isfile(os.path.join(ROOT, g)):
                todo.append(g)
    return files


def digest_files(lib):
    """What digest(lib) reads, relative to the repository root, sorted."""
    return sorted(_digest_sources(lib))


def digest(lib):
    """sha256 over everything the library is built from: the files of digest_files() under their relative names, the
    flags and the units.  Written next to the library after a build and compared by the tests and by the loader, so a
    library left over from other sources (e.g. after `git checkout`) is caught."""
    h = hashlib.sha256()
    for f, text in sorted(_digest_sources(lib).items()):
        h.update(f.encode())
        h.update(text)
    us = [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in library(lib).units()]
    h.update(repr((FLAGS, us)).encode())
    return h.hexdigest()


def source_digest():
    return digest("libhode.so")


def _deps_newest(obj, src):
    """Newest mtime among the files `obj` was compiled from (the -MD depfile hipcc left next to it), the ABI header and this
    script; None if there is no usable depfile (then the unit is rebuilt)."""
    dfile = obj[:-2] + ".d"
    try:
        txt = open(dfile).read()
    except OSError:
        return None
    deps = [x for x in txt.replace("\\\n", " ").split() if not x.endswith(":")]
    ts = [os.path.getmtime(__file__), os.path.getmtime(src)]
    for d in deps:
        if d.startswith("/opt/") or d.startswith("/usr/"):
            continue   # toolchain headers do not change inside a container
        try:
            ts.append(os.path.getmtime(d))
        except OSError:
            return None
    return max(ts)


def compile_one(name, src, extra, force, obj_dir=OBJ):
    obj = os.path.join(obj_dir, name + ".o")
    flags_txt = " ".join(FLAGS + extra)
    stamp = obj[:-2] + ".flags"
    if not force and os.path.exists(obj):
        newest = _deps_newest(obj, src)
        try:
            same_flags = open(stamp).read() == flags_txt
        except OSError:
            same_flags = False
        if newest is not None and same_flags and os.path.getmtime(obj) >= newest:
            return name, 0.0, ""
    t0 = time.time()
    cmd = [HIPCC] + FLAGS + extra + ["-MD", "-MF", obj[:-2] + ".d", "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (name, " ".join(cmd), r.stderr[-6000:]))
    with open(stamp, "w") as f:
        f.write(flags_txt)
    return name, time.time() - t0, r.stderr


def link(out, objs):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", "-o", out] + objs,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stderr[-4000:])


def build(jobs=7, force=False, verbose=True):
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        futs = []
        for lib in built_libraries():
            os.makedirs(lib.obj, exist_ok=True)
            futs += [ex.submit(compile_one, n, s, e, force, lib.obj) for n, s, e in lib.units()]
        for f in futs:
            name, dt, err = f.result()
            if verbose and dt:
                print("  hipcc %-14s %.1fs" % (name, dt), flush=True)
            if verbose and err.strip():
                print(err[-2000:], file=sys.stderr)
    for lib in built_libraries():
        objs = [os.path.join(lib.obj, n + ".o") for n, _, _ in lib.units()]
        if force or not os.path.exists(lib.out) or os.path.getmtime(lib.out) < max(os.path.getmtime(o) for o in objs):
            link(lib.out, objs)
            if verbose:
                print("  linked", os.path.relpath(lib.out, ROOT), flush=True)
        with open(lib.out + ".digest", "w") as f:
            f.write(digest(lib.name) + "\n")
    return OUT


def build_variant(tag, unit_flags, verbose=True):
    """Experiment builds (never loaded by the product): libhode_<tag>.so = the main build's objects with the units named in
    `unit_flags` ({unit: [extra flags]}) recompiled with those flags ON TOP of their product flags.  Select it at run time
    with HODE_LIBRARY=<path>.  The main library must be built first."""
    build(verbose=False)
    objs = []
    for name, src, extra in units():
        if name in unit_flags:
            obj = os.path.join(OBJ, "%s__%s.o" % (name, tag))
            cmd = [HIPCC] + FLAGS + extra + list(unit_flags[name]) + ["-c", src, "-o", obj]
            t0 = time.time()
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed for variant %s of %s:\n%s" % (tag, name, r.stderr[-6000:]))
            if verbose:
                print("  hipcc %s [%s] %.1fs" % (name, tag, time.time() - t0), flush=True)
            objs.append(obj)
        else:
            objs.append(os.path.join(OBJ, name + ".o"))
    out = os.path.join(os.path.dirname(OUT), "libhode_%s.so" % tag)
    link(out, objs)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=7)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--variant", help="tag of an experiment build (libhode_<tag>.so), with --unit-flags")
    ap.add_argument("--unit-flags", action="append", default=[], help='unit="extra flags" (repeatable), e.g. hode_rk_split="-DHODE_SPLIT_WPE_FWD=2"')
    a = ap.parse_args()
    if a.variant:
        uf = {}
        for item in a.unit_flags:
            k, v = item.split("=", 1)
            uf[k] = v.split()
        print(build_variant(a.variant, uf))
    else:
        build(a.j, a.force)
