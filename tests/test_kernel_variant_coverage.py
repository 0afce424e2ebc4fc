"""Guard (no GPU): every compiled instantiation of the solver / decoder kernel families is launched by some entry of
tests/kernel_variants.py's CASES -- the table tests/test_hip_kernel_variants.py runs against float64 -- or is listed as
UNREACHABLE with a reason; and the restated dispatch rules agree with the library's own tile-dependent workspace sizes.
A new tile class, method or flag that no test reaches fails here."""
import ctypes
import glob
import os
import sys

import pytest

import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "build")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def compiled():
    objs = sorted(glob.glob(os.path.join(BUILD, "*.o")))
    objs = [o for o in objs if "__" not in os.path.basename(o)]  # experiment builds (build_hip.build_variant)
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    from kernel_descriptor import kernel_descriptors
    names = set()
    for o in objs:
        for dem, _ in kernel_descriptors(o):
            n = kv.kernel_name(dem)
            if kv.family(n):
                names.add(n)
    return names


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
