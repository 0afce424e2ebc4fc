"""Guard (no GPU): every compiled instantiation of the solver / decoder kernel families is launched by some entry of
tests/kernel_variants.py's CASES -- the table tests/test_hip_kernel_variants.py runs against float64 -- or is listed as
UNREACHABLE with a reason; and the restated dispatch rules agree with the library's own tile-dependent workspace sizes.
A new tile class, method or flag that no test reaches fails here.

The Roche kernels branch at run time between inlined rhs bodies (kv.roche_body), which the symbols do not show: every
(instantiation, body) pair must be reached by a case too, and the branch itself is read out of the kernel source and
compared with kv.bodies(), so that a new body or a changed condition fails here as well."""
import ast
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest

import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc")
BUILD = os.path.join(CSRC, "build")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def compiled_kernel_names(obj_dir=BUILD):
    """Every kernel symbol (`.kd`) of the object files in `obj_dir` (libhode.so's by default), as kv.kernel_name spells it.
    tests/test_failure_cases.py reads both solver libraries with it."""
    objs = sorted(glob.glob(os.path.join(obj_dir, "*.o")))
    objs = [o for o in objs if "__" not in os.path.basename(o)]  # experiment builds (build_hip.build_variant)
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    from kernel_descriptor import kernel_descriptors
    return {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}


@pytest.fixture(scope="module")
def all_compiled():
    """Every kernel symbol (`.kd`) of the library's object files."""
    return compiled_kernel_names()


@pytest.fixture(scope="module")
def compiled(all_compiled):
    return {n for n in all_compiled if kv.family(n)}


def _covered():
    cov = {}
    for c in kv.CASES:
        for n in kv.kernels(c):
            cov.setdefault(n, []).append(c)
    return cov


def test_every_family_is_compiled(compiled):
    fams = {kv.family(n) for n in compiled}
    assert fams == set(kv.FAMILIES), sorted(set(kv.FAMILIES) - fams)


def test_every_compiled_instantiation_is_reached_by_a_case(compiled):
    missing = sorted(compiled - set(_covered()) - set(kv.UNREACHABLE))
    assert not missing, "%d compiled instantiations no CASES entry reaches:\n  %s" % (len(missing), "\n  ".join(missing))


def test_every_case_names_a_compiled_instantiation(compiled):
    """A restated rule that names a kernel the build does not contain is itself wrong."""
    unknown = sorted(set(_covered()) - compiled)
    assert not unknown, unknown
    assert not set(kv.UNREACHABLE) & set(_covered())
    assert set(kv.UNREACHABLE) <= compiled


def test_case_table_is_well_formed():
    ids = [kv.case_id(c) for c in kv.CASES]
    assert len(ids) == len(set(ids))
    for c in kv.CASES:
        assert kv.kernels(c)


def _pairs_covered():
    cov = {}
    for c in kv.CASES:
        b = kv.body(c)
        for n in kv.kernels(c):
            if b in kv.bodies(n):
                cov.setdefault((n, b), []).append(c)
    return cov


def test_every_roche_instantiation_body_pair_is_reached_by_a_case(compiled):
    pairs = {(n, b) for n in compiled - set(kv.UNREACHABLE) for b in kv.bodies(n)}
    assert len({n for n, _ in pairs}) >= 300  # every Roche family is in the build and counted
    missing = sorted(pairs - set(_pairs_covered()) - set(kv.UNREACHABLE_BODIES))
    assert not missing, "%d (instantiation, body) pairs no CASES entry reaches:\n  %s" % (
        len(missing), "\n  ".join("%s  %s" % p for p in missing))
    assert set(kv.UNREACHABLE_BODIES) <= pairs and not set(kv.UNREACHABLE_BODIES) & set(_pairs_covered())


def test_every_roche_case_names_its_body():
    for c in kv.CASES:
        ks = kv.kernels(c)
        if c["family"] in ("roche", "dopri5"):
            b = kv.body(c)
            assert c["theta"] in ("default", "general", "hill_ulp") and c["n_dose"] in (0, 1, 2, 3), c
            assert all(b in kv.bodies(n) for n in ks if kv.family(n) in kv.ROCHE_FAMILIES), c
            assert any(kv.family(n) in kv.ROCHE_FAMILIES for n in ks), c
        else:
            assert kv.body(c) is None and not any(kv.bodies(n) for n in ks)


def test_roche_body_rule():
    th = kv.theta_of
    assert kv.roche_body(False, 2.0, 2.0, 1) == "hill2_k1"
    for K in (0, 2, 3):
        assert kv.roche_body(False, 2.0, 2.0, K) == "hill2_kn"
        assert kv.roche_body(True, 2.5, 1.5, K) == "hill2_kn"  # ABLATE forces hill2
    assert kv.roche_body(True, 3.0, 1.0, 1) == "hill2_k1"
    assert kv.HILL_ULP == float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    assert kv.roche_body(False, *th(dict(theta="hill_ulp"))[:2], 1) == "general"
    for hill in kv.GENERAL_HILL + (kv.NEG_BASE_HILL,):
        t = th(dict(theta="general", hill=hill))
        assert len(t) == 13 and kv.roche_body(False, t[0], t[1], 1) == "general"
    assert any(2.0 not in th(dict(theta="general", hill=h))[:2] for h in kv.GENERAL_HILL)
    assert any(th(dict(theta="general", hill=h))[:2].count(2.0) == 1 for h in kv.GENERAL_HILL)
    assert kv.bodies("hode::split_bwd_kernel<12, 2, false, true, true>") == ("hill2_k1", "hill2_kn", "general")
    assert kv.bodies("hode::rk_fwd_kernel<8, 4, 2, true>") == ("hill2_k1", "hill2_kn")
    assert kv.bodies("hode::dp_initbwd_kernel<8, 4, true, false, 1>") == ("hill2_k1", "hill2_kn")
    assert kv.bodies("hode::dp_persist_kernel<8, false>") == ("hill2_k1", "hill2_kn", "general")
    assert kv.bodies("hode::split_fold_kernel") == ()


def test_general_hill_cases_cover_the_split_layout():
    for D in (8, 12):
        for method in kv.METHODS:
            assert any(c["family"] == "roche" and kv.body(c) == "general" and c["D"] == D and c["method"] == method
                       and kv.roche_layout(D, c["lanes"], kv.ROCHE_T) == "split" for c in kv.CASES), (D, method)


# ----------------------------------------------------------------------------- the runtime branch in the kernel source
ROCHE_SOURCES = ("hode_rk_kernels.hpp", "hode_rk_split.hip", "hode_rk_mf.hip", "hode_dopri5_kernels.hpp")
# the hill2 definitions kv.roche_body restates (whitespace normalised); dp_* attempt launches: decided by the host
HILL2_DEFS = ("ABLATE || (a.theta[0] == 2.0f && a.theta[1] == 2.0f)",
              "ABLATE || (a.hill2 >= 0 ? a.hill2 != 0 : (a.theta[0] == 2.0f && a.theta[1] == 2.0f))",
              "ABLATE || a.hill2 != 0")
# condition of the runtime if / else-if / else chain -> (HILL2, K1) of the call it guards
BRANCH_CONDS = {"hill2 && a.K == 1": (True, True), "hill2": (True, False), None: (False, False)}


def _norm(x):
    return " ".join(x.split())


def _strip_and_expand(src):
    """Comments removed, line continuations joined, and the function-like macros defined in the file expanded (e.g.
    HODE_DP_DISPATCH(BODY) in hode_dopri5_kernels.hpp)."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = src.replace("\\\n", " ")
    for name, arg, body in re.findall(r"^[ \t]*#define[ \t]+(\w+)\((\w+)\)([^\n]*)$", src, flags=re.M):
        src = re.sub(r"^[ \t]*#define[ \t]+%s\(.*$" % name, "", src, flags=re.M)
        src = re.sub(r"\b%s\((\w+)\)" % name, lambda m: re.sub(r"\b%s\b" % arg, m.group(1), body), src)
    return src


def _match(src, i, open_, close):
    """Index one past the bracket that closes src[i] (== open_)."""
    depth = 0
    for j in range(i, len(src)):
        if src[j] == open_:
            depth += 1
        elif src[j] == close:
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError("unbalanced %s" % open_)


def _constexpr_arms(body):
    """The arms of a top-level `if constexpr (...) {...} else if constexpr (...) {...} else {...}` chain, each with the
    text outside the chain appended; [body] when there is none."""
    m = re.search(r"\bif constexpr\s*\(", body)
    if not m:
        return [body]
    arms, i, start = [], m.start(), m.start()
    while True:
        j = _match(body, body.index("(", i), "(", ")")
        k = body.index("{", j)
        assert not body[j:k].strip(), body[i:k]
        e = _match(body, k, "{", "}")
        arms.append(body[k + 1:e - 1])
        rest = body[e:]
        m2 = re.match(r"\s*else\s+if constexpr\s*\(", rest)
        if m2:
            i = e + m2.end() - 1
            i = body.rindex("if", e, i)
            continue
        m3 = re.match(r"\s*else\s*\{", rest)
        if m3:
            k = e + m3.end() - 1
            e2 = _match(body, k, "{", "}")
            arms.append(body[k + 1:e2 - 1])
            e = e2
        outside = body[:start] + body[e:]
        return [a + outside for a in arms]


def roche_source_branches(csrc=CSRC):
    """{kernel: [set of (HILL2, K1) per if-constexpr arm]} for every __global__ Roche kernel in ROCHE_SOURCES, with every
    runtime branch's condition checked against BRANCH_CONDS and the hill2 definition against HILL2_DEFS."""
    out = {}
    for fn in ROCHE_SOURCES:
        src = _strip_and_expand(open(os.path.join(csrc, fn)).read())
        params = {}  # body function -> (index of HILL2, index of K1) in its template parameter list
        for tp, name in re.findall(r"template\s*<([^<>]*)>\s*HODE_DEV\s+void\s+(\w+)\s*\(", src):
            names = [p.split()[-1] for p in tp.split(",")]
            if "HILL2" in names and "K1" in names:
                params[name] = (names.index("HILL2"), names.index("K1"))
        for m in re.finditer(r"template\s*<[^<>]*>\s*__global__[^{;]*?\bvoid\s+(\w+)\s*\([^()]*\)\s*\{", src):
            kname, k = m.group(1), m.end() - 1
            body = src[k + 1:_match(src, k, "{", "}") - 1]
            calls = re.findall(r"\b(\w+)\s*<[^<>]*>\s*\(", body)
            if not any(c in params for c in calls):
                continue
            defs = re.findall(r"const bool hill2 = ([^;]*);", body)
            assert len(defs) == 1 and _norm(defs[0]) in HILL2_DEFS, (fn, kname, defs)
            arms = []
            for arm in _constexpr_arms(body):
                pairs = []
                for kw, cond, callee, targs in re.findall(
                        r"(else\s+if|if|else)\s*(?:\(([^()]*)\))?\s*(\w+)\s*<([^<>]*)>\s*\(", arm):
                    if callee not in params:
                        continue
                    args = [x.strip() for x in targs.split(",")]
                    ih, ik = params[callee]
                    assert args[ih] in ("true", "false") and args[ik] in ("true", "false"), (kname, callee, targs)
                    pair = (args[ih] == "true", args[ik] == "true")
                    key = _norm(cond) if kw.strip() != "else" else None
                    assert key in BRANCH_CONDS and BRANCH_CONDS[key] == pair, (fn, kname, kw, cond, callee, pair)
                    pairs.append(pair)
                assert pairs and len(pairs) == len(set(pairs)), (fn, kname, pairs)
                arms.append(set(pairs))
            assert kname not in out, kname
            out[kname] = arms
    return out


def test_roche_source_branches_match_the_body_rule(compiled):
    """Every (HILL2, K1) pair a Roche kernel's source dispatches, per if-constexpr arm, is a body kv.bodies() lists for its
    instantiations: all three for the full rhs; with ABLATE = true the hill2 definition (ABLATE || ...) leaves the
    HILL2 = true calls.  dp_bwd_kernel has six calls, three per arm."""
    src = roche_source_branches()
    assert set(src) == set(kv.ROCHE_FAMILIES), sorted(set(src) ^ set(kv.ROCHE_FAMILIES))
    assert len(src["dp_bwd_kernel"]) == 2 and len(src["dp_fwd_kernel"]) == 4
    seen = set()
    for n in compiled:
        fam = kv.family(n)
        if fam not in kv.ROCHE_FAMILIES:
            continue
        seen.add(fam)
        want = {kv.BODY_ARGS[b] for b in kv.bodies(n)}
        for arm in src[fam]:
            live = {p for p in arm if p[0] or not kv._ablate_arg(n)}
            assert live == want, (n, sorted(live), sorted(want))
    assert seen == set(kv.ROCHE_FAMILIES)


def test_host_hill2_read_back_is_the_same_comparison():
    """The dopri5 attempt launches take hill2 from the host (csrc/hode_dopri5.hip): the comparison kv.roche_body restates."""
    src = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_dopri5.hip")).read()))
    assert "a.hill2 = (hill[0] == 2.0f && hill[1] == 2.0f) ? 1 : 0;" in src
    assert "a.hill2 = -1;" in src


def test_kernel_name_normalisation():
    assert kv.kernel_name("void hode::(anonymous namespace)::neural_real_bwd_kernel<5, 4, 4, 3, 2>"
                          "(hode::(anonymous namespace)::NrArgs)") == "hode::neural_real_bwd_kernel<5, 4, 4, 3, 2>"
    assert kv.kernel_name("void hode::split_bwd_kernel<12, 2, false, false, true>(hode::SplitBwdArgs)") == \
        "hode::split_bwd_kernel<12, 2, false, false, true>"
    assert kv.kernel_name("hode::fold_partials_kernel(float const*, int)") == "hode::fold_partials_kernel"


# ------------------------------------------------------------------------------- restated rules against the library
def _classes(values, key):
    """Group consecutive values by `key`; returns [(key, [values])]."""
    out = []
    for v in values:
        k = key(v)
        if out and out[-1][0] == k:
            out[-1][1].append(v)
        else:
            out.append((k, [v]))
    return out


def _assert_size_follows_rule(values, key, size):
    """size(v) is constant inside every class of the rule and changes at every class boundary."""
    groups = _classes(values, key)
    sizes = []
    for k, vs in groups:
        s = {size(v) for v in vs}
        assert len(s) == 1 and 0 not in s, (k, vs, s)
        sizes.append(s.pop())
    for (k0, v0), (k1, v1), s0, s1 in zip(groups, groups[1:], sizes, sizes[1:]):
        assert s0 != s1, "rule predicts a new class between %s and %s, the library's size does not change" % (v0[-1], v1[0])
    return groups


def test_seqdec_tile_rule_matches_the_workspace_size():
    import hode
    from hode import _lib as L
    lib = hode.lib()
    for kind in ("tlstm", "gruode"):
        d = L.SeqdecDesc()
        d.struct_size = ctypes.sizeof(L.SeqdecDesc)
        d.kind, d.n_steps, d.n_action_times, d.batch, d.action_dim = kv.SEQDEC_KIND[kind], 4, 4, 37, 1

        def size(D):
            d.latent_dim = D
            return lib.hode_seqdec_workspace_bytes(d)
        groups = _assert_size_follows_rule(range(1, L.SEQDEC_MAX_LATENT + 1), kv.seqdec_tiles, size)
        assert [g[1][0] for g in groups] == [1, 14, 17]  # the boundaries 13|14 and 16|17


def _solve_desc(kind, D, H, B=37):
    from hode import _lib as L
    d = L.new_solve_desc()
    d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim, d.n_action_times = kind, L.METHODS["rk4"], B, D, 6, H, 5
    return d


def test_neural_real_tile_rule_matches_the_workspace_size():
    import hode
    from hode import _lib as L
    lib = hode.lib()
    for kind, Ds, starts in (("neural", range(1, 31), [1, 15, 17]), ("2nd", range(2, 61, 2), [2, 30, 34])):
        for H in (1, 16, 17, 43, 64):
            def size(D):
                return lib.hode_workspace_bytes(_solve_desc(kv.NR_KIND[kind], D, H), L.WS_RK_BWD)
            groups = _assert_size_follows_rule(Ds, lambda D: kv.neural_real_shape(kind, D, H)[:2], size)
            assert [g[1][0] for g in groups] == starts, (kind, H)
        for D in ((15, 16) if kind == "neural" else (30, 32)):
            def hsize(H):
                return lib.hode_workspace_bytes(_solve_desc(kv.NR_KIND[kind], D, H), L.WS_RK_BWD)
            groups = _assert_size_follows_rule(range(1, 65), lambda H: kv.neural_real_shape(kind, D, H)[2], hsize)
            assert [g[1][0] for g in groups] == [1, 17, 33, 49]


def test_real_mf_tile_rule_matches_the_workspace_size():
    """With grad_w1 set (the on-chip backward) the workspace holds RealGradAcc<HT> partials per wave: constant inside each
    hidden-tile class, different at 16|17, 32|33, 48|49; at H = 65 the library falls back to hode_real.hip's tape."""
    import hode
    from hode import _lib as L
    lib = hode.lib()
    buf = (ctypes.c_float * 4)()

    def size(H):
        d = _solve_desc(L.RHS_ROCHE_REAL, 20, H)
        d.grad_w1 = ctypes.addressof(buf)  # never dereferenced: only selects the on-chip layout
        return lib.hode_workspace_bytes(d, L.WS_RK_BWD)

    def key(H):
        return tuple(kv.real_kernels(20, H, kv.RK4))
    groups = _assert_size_follows_rule(range(1, 66), key, size)
    assert [g[1][0] for g in groups] == [1, 17, 33, 49, 65]
    assert key(65)[0].startswith("hode::real_kernel<20")
    # without grad_w1 the tape layout grows with every hidden unit (both the tape kernels and the tape-writing MFMA one)
    sizes = [lib.hode_workspace_bytes(_solve_desc(L.RHS_ROCHE_REAL, 20, H), L.WS_RK_BWD) for H in (16, 17, 64, 65)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4


# ------------------------------------------------------------------------------------------------ the whole library
def test_every_kernel_of_the_library_is_accounted_for(all_compiled):
    """Every kernel symbol of the build belongs to a covered family (FAMILIES) or is named in kv.OTHER_KERNELS with the
    test that checks it against a float64 reference: a new __global__ anywhere fails here until it is one or the other."""
    stray = sorted(n for n in all_compiled if not kv.family(n) and n not in kv.OTHER_KERNELS)
    assert not stray, "kernels outside FAMILIES and OTHER_KERNELS:\n  %s" % "\n  ".join(stray)
    assert set(kv.OTHER_KERNELS) <= all_compiled, sorted(set(kv.OTHER_KERNELS) - all_compiled)
    assert not any(kv.family(n) for n in kv.OTHER_KERNELS)
    covered = set(_covered())
    for name, test in kv.OTHER_KERNELS.items():
        assert name not in covered, name  # a case lists it: it belongs in FAMILIES
        path, func = test.split("::")
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {f.name for f in tree.body if isinstance(f, ast.FunctionDef)}, test


def test_new_families_are_covered_by_substantive_cases(compiled):
    """The NeuralODE, LSTM and readout instantiations in the build are exactly those the restated rules produce over their
    domains (kv.instantiations), and each is reached by a case where its arithmetic really runs (kv.substantive: T >= 3,
    B > 16 and ragged): a T = 1 or B = 1 entry alone does not count."""
    fams = {kv.family(n) for c in kv.CASES if c["family"] in kv.NEW_FAMILIES for n in kv.kernels(c)}
    have = {n for n in compiled if kv.family(n) in fams}
    want = kv.instantiations()
    assert have == want, (sorted(have - want), sorted(want - have))
    real = {n for c in kv.CASES if c["family"] in kv.NEW_FAMILIES and kv.substantive(c) for n in kv.kernels(c)}
    missing = sorted(want - real)
    assert not missing, "instantiations reached only by T = 1 / B <= 16 cases:\n  %s" % "\n  ".join(missing)
    for fam in kv.NEW_FAMILIES:  # and the degenerate calls are there on top
        cs = [c for c in kv.CASES if c["family"] == fam]
        assert any(c["B"] == 1 for c in cs) and any(c["T"] == 1 for c in cs), fam


def test_neural_rules():
    assert kv.neural_layout(6, 1) == "lane" and kv.neural_layout(12, 1) == "lane" and kv.neural_layout(6, 16) == "mf"
    assert kv.neural_layout(14) == "mf" and kv.neural_layout(4, 0) == "mf"
    with pytest.raises(AssertionError):
        kv.neural_layout(14, 1)
    assert kv.neural_grid(65, "mf") == 5 and kv.neural_grid(65, "lane") == 2 and kv.neural_grid(64, "lane") == 1
    assert kv.neural_fixed(8, kv.RK4, 0, False)[-1] == "hode::neural_mf_bwd_kernel<8, 2, false>"
    assert "hode::transpose_w2_kernel" in kv.neural_fixed(8, kv.RK4, 1, True)
    assert not any("initbwd" in n for n in kv.neural_dopri5_kernels(8, 0, False))
    assert not any("initbwd" in n for n in kv.neural_dopri5_kernels(8, 5, True))
    # the dose / tile edges the issue names appear somewhere in the table
    nc = [c for c in kv.CASES if c["family"] == "neural"]
    assert any(c["B"] % 16 and c["B"] % 64 for c in nc) and any(c["B"] == 65 and c["layout"] == "lane" for c in nc)
    assert any(c["B"] == 1 for c in nc) and any(c["T"] == 1 for c in nc)
    assert {c["perturb"] for c in nc} == {False, True} and {0, 1, 3} <= {c["n_dose"] for c in nc}
    assert {c["dose"] for c in nc} == {"grid", "dup", "third"}
    assert any(c["dose"] == "third" and c["method"] == "rk4" for c in nc)
    assert all(c["n_dose"] >= 2 for c in nc if c["dose"] != "grid")


def test_neural_source_pins_the_restated_rules():
    """The lines kv.neural_layout / neural_fixed / neural_dopri5_kernels restate, as they read in the source."""
    nh = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_neural.hip")).read()))
    assert "bool neural_lanes(const hode_solve_desc* d) { return d->lanes_per_patient == 1; }" in nh
    assert "if (!neural_lanes(d)) return launch_neural_mf(d, a, bwd, s);" in nh
    assert "bool neural_onchip(const hode_solve_desc* d) { return !neural_lanes(d) && d->grad_w1 != nullptr; }" in nh
    assert "if (D != 6 && D != 8 && D != 12)" in nh
    assert "const dim3 grid((d->batch + 63) / 64), block(64);" in nh
    # the launchers are next to the kernel templates they launch; the list of sizes serves both dispatch files
    mf = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_neural_mf_kernels.hpp")).read()))
    assert "const dim3 grid((d->batch + 15) / 16), block(64); const bool onchip = bwd && d->grad_w1 != nullptr;" in mf
    assert kv.NEURAL_DOPRI5_DIMS == kv.NEURAL_DIMS
    raw = open(os.path.join(CSRC, "hode_host.hpp")).read()
    assert "#define HODE_NEURAL_DIMS(X) " + " ".join("X(%d)" % D for D in kv.NEURAL_DOPRI5_DIMS) + "\n" in raw
    for unit in ("hode_neural_mf.hip", "hode_neural_dopri5.hip"):
        assert "HODE_NEURAL_DIMS(" in open(os.path.join(CSRC, unit)).read()
    nd = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_neural_dopri5_kernels.hpp")).read()))
    assert "if (a.n_acc > 0 && !(d->flags & HODE_FLAG_DETACH_FIRST_STEP)) {" in nd


def test_lstm_rules():
    """FLAT and VEC4 against an independent statement of them (the padded sizes; obs % 4), NT's bounds and its tie rule."""
    for H in range(1, 161):
        flat = kv.lstm_kernels(H, 20, 37, True)[3].endswith("true>")
        assert flat == (H in kv.LSTM_SIZES), H
        assert kv.lstm_kernels(H, 20, 37, True)[1].endswith("false>") == flat, H   # the forward's PAD: the padded sizes again
    for obs in range(1, 41):
        assert kv.lstm_kernels(16, obs, 37, True)[1].endswith("true, false>") == (obs % 4 == 0)   # VEC4; H = 16: no padded unit
        assert kv.lstm_kernels(16, obs, 37, True)[4].endswith("true>") == (obs % 4 == 0)
    assert [kv.choose_nt(B, True) for B in (1, 4096, 4097, 8193, 12289)] == [1, 1, 2, 3, 2]
    assert [kv.choose_nt(B, False) for B in (1, 4097, 8193, 12289)] == [1, 2, 3, 4]
    assert kv.lstm_geom(40, 100, 150, False, 4)[4] == 3  # the staging clamp after the override
    # the LDS bound is checked on the clamped tile: H = 129 .. 160 with obs = 100 at NT 4 -> 3 is supported
    assert kv.lstm_workspace_bytes(3, 12289, 101, 150, 100, False) > 0
    assert any(c["family"] == "lstm" and c["H"] > 128 and c["obs"] == 100 and c["nt"] == 4 for c in kv.CASES)
    assert kv.lstm_geom(40, 20, 150, True, 4)[4] == kv.choose_nt(150, True)  # override outside the bound: ignored
    seen = {}
    for c in kv.CASES:
        if c["family"] == "lstm" and c["nt"] is None:
            seen.setdefault(kv.lstm_geom(c["H"], c["obs"], c["B"], c["tape"])[4], []).append(c)
    assert sorted(seen) == [1, 2, 3, 4]  # each NT chosen from the batch size alone, not the override
    lc = [c for c in kv.CASES if c["family"] == "lstm"]
    for tpw in kv.LSTM_TPWS:
        hs = {c["H"] % 16 == 0 for c in lc if kv.lstm_geom(c["H"], c["obs"], c["B"], c["tape"])[1] == tpw}
        assert hs == {True, False}, tpw


def test_lstm_source_pins_the_restated_rules():
    src = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_lstm_tpw.hip")).read()))
    assert "constexpr int kFwdNW = kTPW <= 5 ? 4 : 8;" in src and "constexpr int kFwdTPW = kTPW <= 5 ? kTPW : kTPW / 2;" in src
    assert "return (a.OBS & 3) == 0 ? launch_fwd_pad<NT, true>(G, a, s) : launch_fwd_pad<NT, false>(G, a, s);" in src
    assert "return a.H == 16 * kTPW ? launch_fwd_vec<NT, VEC4, false>(G, a, s) : launch_fwd_vec<NT, VEC4, true>(G, a, s);" in src
    assert "return a.H == 16 * kTPW ? launch_bwd_flat<NT, true>(G, a, s) : launch_bwd_flat<NT, false>(G, a, s);" in src
    lh = _norm(_strip_and_expand(open(os.path.join(CSRC, "hode_lstm.hip")).read()))
    assert "static const int kSizes[] = {%s};" % ", ".join(str(v) for v in kv.LSTM_SIZES) in lh
    assert "const bool vec4 = (obs & 3) == 0 &&" in lh
    assert "if (d->patient_tiles >= 1 && d->patient_tiles <= (bwd_compatible ? 3 : 4)) G->NT = d->patient_tiles;" in lh
    import build_hip
    assert tuple(sorted(build_hip.LSTM_TPWS)) == tuple(sorted(kv.LSTM_TPWS))


def _lstm_desc(T, B, obs, H, tape, patient_tiles=0):
    from hode import _lib as L
    d = L.new_lstm_desc()
    d.seq_len, d.batch, d.input_dim, d.hidden_dim, d.obs_dim, d.save_tape = T, B, obs + 1, H, obs, int(tape)
    d.patient_tiles = patient_tiles
    return d


def test_lstm_geometry_matches_the_workspace_size():
    """hode_lstm_workspace_bytes against kv.lstm_workspace_bytes: the packed weights depend on Hp and KQ4, the tape on NT
    (nblk NT differs between tiles for ragged batches) -- with NT chosen by the batch size (both sides of every tie) and
    forced by the descriptor's patient_tiles, the staging clamp included."""
    import hode
    lib = hode.lib()
    Bs = (1, 17, 4095, 4096, 4097, 6145, 8192, 8193, 12288, 12289, 16385, 20481, 24577)
    n = 0
    for H in (1, 13, 16, 17, 47, 64, 65, 96, 97, 125, 128, 129, 160):
        for obs in (1, 20, 23, 80, 100):
            for B in Bs:
                for tape in (True, False):
                    got = lib.hode_lstm_workspace_bytes(_lstm_desc(3, B, obs, H, tape))
                    assert got == kv.lstm_workspace_bytes(3, B, obs + 1, H, obs, tape), (H, obs, B, tape)
                    n += 1
    assert n > 1000
    for nt in (1, 2, 3, 4):
        for B in (37, 101, 4097):
            for obs in (20, 100):
                got = lib.hode_lstm_workspace_bytes(_lstm_desc(2, B, obs, 40, True, nt))
                assert got == kv.lstm_workspace_bytes(2, B, obs + 1, 40, obs, True, nt), (nt, B, obs)


def test_readout_rules_match_the_workspace_size():
    """hode_readout_workspace_bytes = readout_waves * (1 + obs D + obs) floats: the waves depend on whether readout_mf was
    chosen (16 rows per wave-iteration against 64 / (obs / 4)) -- every obs at both latent dimensions with a window, with and
    without the descriptor's variant set to READOUT_VARIANT_VALU."""
    import hode
    from hode import _lib as L
    lib = hode.lib()
    assert kv.READOUT_VARIANT_VALU == L.READOUT_VARIANT_VALU
    for valu in (0, L.READOUT_VARIANT_VALU):
        for D in (4, 6, 8, 12):
            for obs in range(4, 129, 4):
                for rows in (1, 37, 1000, 40000):
                    d = L.ReadoutDesc()
                    d.struct_size = ctypes.sizeof(L.ReadoutDesc)
                    d.latent_dim, d.obs_dim, d.rows, d.variant = D, obs, rows, valu
                    want = kv.readout_waves(rows, obs, D, valu) * (1 + obs * D + obs) * 4
                    assert lib.hode_readout_workspace_bytes(d) == want, (valu, D, obs, rows)
    assert [o for o in range(4, 129, 4) if kv.readout_mf(12, o)] == [52, 56, 60, 64, 68, 72, 76, 80]
    assert [o for o in range(4, 129, 4) if kv.readout_mf(8, o)] == [36, 40, 44, 48]
    rc = [(c["D"], c["obs"]) for c in kv.CASES if c["family"] == "readout" and not c["valu"]]
    for edge in ((12, 48), (12, 52), (12, 80), (12, 84), (8, 32), (8, 36), (8, 48), (8, 52)):
        assert edge in rc, edge
    assert "if (d->latent_dim == 20) HODE_RM(20) else HODE_RM(4)" in open(os.path.join(CSRC, "hode_readout_mlp.hip")).read()


def test_neural_rule_matches_the_workspace_size():
    """hode_workspace_bytes(..., WS_RK_BWD) of the neural rhs: with grad_w1 (the on-chip backward) one block of
    2 HT 256 + 16 floats of partials per 16-patient wave (HT = ceil(10 D / 16)), independent of T and the method; without
    grad_w1, or with the lane layout, the four tapes (T - 1) stages (10 D + 10 D + D + 1 + D) B floats."""
    import hode
    from hode import _lib as L
    lib = hode.lib()
    buf = (ctypes.c_float * 4)()
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731

    def size(D, B, T, method, onchip, lanes):
        d = L.new_solve_desc()
        d.rhs_kind, d.method, d.batch, d.latent_dim, d.n_times, d.hidden_dim = L.RHS_NEURAL, L.METHODS[method], B, D, T, 10 * D
        d.lanes_per_patient = lanes
        if onchip:
            d.grad_w1 = ctypes.addressof(buf)  # never dereferenced: only selects the on-chip layout
        return lib.hode_workspace_bytes(d, L.WS_RK_BWD)

    for lanes in (0, 1):
        for D in (4, 6, 8, 10, 12, 14):
            HD, HT = 10 * D, (10 * D + 15) // 16
            for B in (1, 16, 17, 64, 65, 129):
                for T in (1, 2, 6):
                    for method, ns in (("euler", 1), ("midpoint", 2), ("rk4", 4)):
                        w2t = al(HD * D * 4)
                        inst = (T - 1) * ns
                        tapes = w2t + al(inst * HD * B * 4) * 2 + al(inst * (D + 1) * B * 4) + al(inst * D * B * 4)
                        onchip = w2t + al(kv.neural_grid(B, "mf") * (2 * HT * 256 + 16) * 4)
                        for oc in (True, False):
                            want = onchip if oc and not lanes else tapes
                            assert size(D, B, T, method, oc, lanes) == want, (lanes, D, B, T, method, oc)
