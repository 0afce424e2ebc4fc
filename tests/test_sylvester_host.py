"""CPU checks of the Sylvester flows (no GPU): the mirror modules (flow.Sylvester, flow.TriangularSylvester,
flow.sylvester_chain) against the reference's own numbers (G19, tests/golden/make_golden_sylvester.py), the float64
restatement (sylvester_eager) against G19, the two reproduced quirks, libhode_sylvester.so's C ABI and build-table row,
the compiled kernels against the GPU case table (tests/sylvester_cases.py), and the domain
refusals."""
import glob
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

import abi_checks
import build_hip
import flow
import kernel_variants as kv
import sylvester_cases as cases
import sylvester_eager as se

ROOT = build_hip.ROOT
LIB = "libhode_sylvester.so"
FUNCTIONS = {"hode_sylvester_" + n for n in ("version", "last_error_string", "workspace_bytes", "fwd", "bwd")}
E_NULL, E_SIZE, E_WORKSPACE = -1, -2, -3
SINGLE = ("syl_sum", "syl_terms", "tri_none", "tri_flip", "tri_perm", "tri_quirk")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_sylvester.npz"), allow_pickle=False)


def _rec(g, tag, name, dtype=None):
    pre = "%s_%s_" % (tag, name)
    out = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    assert out, pre
    return out


def _leaves(r, names):
    return [r["in_" + n].clone().requires_grad_(True) for n in names]


def _module_call(name, r):
    """The mirror's call for a G19 record -> (leaves, names, z, ldj)."""
    if name.startswith("syl"):
        names = ("zk", "r1", "r2", "q", "b")
        leaves = _leaves(r, names)
        mod = flow.Sylvester(r["in_r1"].shape[-1]).to(r["in_zk"].dtype)
        z, ldj = mod(*leaves, name == "syl_sum")
    else:
        names = ("zk", "r1", "r2", "b")
        leaves = _leaves(r, names)
        mod = flow.TriangularSylvester(r["in_zk"].shape[-1]).to(r["in_zk"].dtype)
        perm = r.get("perm")
        if name == "tri_quirk":
            z, ldj = mod(leaves[0], leaves[1], leaves[2], leaves[3], perm, True)   # bias fourth, permutation fifth
        else:
            z, ldj = mod._forward(*leaves, perm, name != "tri_flip")
    return leaves, names, z, ldj


# ------------------------------------------------------------------------------------------- 1. the mirror against G19
@pytest.mark.parametrize("name", SINGLE)
def test_modules_give_the_reference_float32_bits(g19, name):
    """Same operations in the same order as the reference on the same CPU: outputs and autograd gradients to the last bit."""
    r = _rec(g19, "f32", name)
    leaves, names, z, ldj = _module_call(name, r)
    assert z.dtype == torch.float32 and z.shape == r["z"].shape and ldj.shape == r["ldj"].shape
    assert torch.equal(z, r["z"]) and torch.equal(ldj, r["ldj"])
    grads = torch.autograd.grad((z * r["gz"]).sum() + (ldj * r["gl"]).sum(), leaves)
    for n, gr in zip(names, grads):
        assert torch.equal(gr, r["grad_" + n]), n


@pytest.mark.parametrize("name", SINGLE)
def test_modules_in_float64(g19, name):
    r = _rec(g19, "f64", name)
    leaves, names, z, ldj = _module_call(name, r)
    assert z.dtype == torch.float64
    torch.testing.assert_close(z, r["z"], rtol=0, atol=1e-12)
    torch.testing.assert_close(ldj, r["ldj"], rtol=0, atol=1e-12)


def _chain_args(r):
    return r["in_zk"].unsqueeze(0), r["in_r1"], r["in_r2"], r["in_b"], r["in_q"]


def test_chain_on_cpu_is_three_module_calls(g19):
    """sylvester_chain on CPU tensors: the K = 3 chain of G19, log_diag (S, B, K, M) and its sum."""
    r = _rec(g19, "f32", "chain3")
    z0, r1, r2, b, q = (t.clone().requires_grad_(True) for t in _chain_args(r))
    z, logdet, log_diag = flow.sylvester_chain(z0, r1, r2, b, q, want_log_diag=True)
    assert z.shape == (1,) + r["z"].shape and logdet.shape == (1, 5) and log_diag.shape == (1,) + r["ldj"].shape
    assert torch.equal(z[0], r["z"]) and torch.equal(log_diag[0], r["ldj"])
    torch.testing.assert_close(logdet[0], r["ldj"].sum(dim=(1, 2)), rtol=1e-6, atol=1e-6)
    assert len(flow.sylvester_chain(z0, r1, r2, b, q)) == 2
    grads = torch.autograd.grad((z[0] * r["gz"]).sum() + (log_diag[0] * r["gl"]).sum(), (z0, r1, r2, q, b))
    for n, gr in zip(("zk", "r1", "r2", "q", "b"), grads):
        torch.testing.assert_close(gr.reshape(r["grad_" + n].shape), r["grad_" + n], rtol=1e-5, atol=1e-6)


def test_module_surface_is_the_references():
    syl, tri = flow.Sylvester(4), flow.TriangularSylvester(5)
    assert syl.num_ortho_vecs == 4 and tri.z_size == 5
    assert list(syl.state_dict()) == ["triu_mask", "diag_idx"] and list(tri.state_dict()) == ["diag_idx"]
    assert torch.equal(syl.triu_mask, torch.triu(torch.ones(4, 4), diagonal=1).unsqueeze(0)) and not syl.triu_mask.requires_grad
    assert torch.equal(syl.diag_idx, torch.arange(4)) and syl.diag_idx.dtype == torch.int64
    x = torch.tensor([-0.5, 0.0, 2.0])
    for mod in (syl, tri):
        assert isinstance(mod.h, torch.nn.Tanh)
        assert torch.equal(mod.der_h(x), 1 - torch.tanh(x) ** 2) and torch.equal(mod.der_tanh(x), mod.der_h(x))
    import inspect
    assert list(inspect.signature(syl._forward).parameters) == ["zk", "r1", "r2", "q_ortho", "b", "sum_ldj"]
    assert list(inspect.signature(syl.forward).parameters) == ["zk", "r1", "r2", "q_ortho", "b", "sum_ldj"]
    assert list(inspect.signature(tri._forward).parameters) == ["zk", "r1", "r2", "b", "permute_z", "sum_ldj"]
    assert list(inspect.signature(tri.forward).parameters) == ["zk", "r1", "r2", "q_ortho", "b", "sum_ldj"]
    assert isinstance(flow.Planar(), torch.nn.Module)


# ------------------------------------------------------------------------------------ 2. the float64 restatement vs G19
def _eager_args(name, r):
    zk, r1, r2, b = r["in_zk"].unsqueeze(0), r["in_r1"].unsqueeze(1), r["in_r2"].unsqueeze(1), r["in_b"]
    q = r["in_q"].unsqueeze(1) if "in_q" in r else None
    perm = r["perm"].unsqueeze(0) if "perm" in r else None
    return zk, r1, r2, b.reshape(b.shape[0], 1, -1), q, perm


@pytest.mark.parametrize("name", SINGLE + ("chain3",))
def test_float64_restatement_against_reference(g19, name):
    r = _rec(g19, "f64", name)
    if name == "chain3":
        args, summed = _chain_args(r) + (None,), False
    else:
        args, summed = _eager_args(name, r), r["ldj"].dim() == 1
    gl = r["gl"].unsqueeze(0)
    z, logdet, log_diag, grads = se.forward_backward(*args, grad_z=r["gz"].unsqueeze(0), grad_logdet=gl if summed else None,
                                                     grad_log_diag=None if summed else gl.reshape(log_diag_shape(args)))
    torch.testing.assert_close(z[0], r["z"], rtol=0, atol=1e-12)
    got = logdet[0] if summed else log_diag[0].reshape(r["ldj"].shape)
    torch.testing.assert_close(got, r["ldj"], rtol=0, atol=1e-12)
    for n, gr in zip(("zk", "r1", "r2", "b", "q"), grads):
        if gr is not None:
            torch.testing.assert_close(gr.reshape(r["grad_" + n].shape), r["grad_" + n], rtol=0, atol=1e-12)


def log_diag_shape(args):
    z0, r1 = args[0], args[1]
    return (z0.shape[0], z0.shape[1], r1.shape[1], r1.shape[2])


# ------------------------------------------------------------------------------------------ 3. the reproduced quirks
def test_triangular_forward_takes_the_bias_fourth_and_the_permutation_fifth(g19):
    """TriangularSylvester.forward(zk, r1, r2, q_ortho, b, sum_ldj) hands `q_ortho` to _forward as the bias and `b` as the
    permutation index, as the reference's does."""
    r = _rec(g19, "f32", "tri_quirk")
    same = _rec(g19, "f32", "tri_perm")   # _forward(zk, r1, r2, bias, perm): the same call spelled properly
    assert torch.equal(r["z"], same["z"]) and torch.equal(r["ldj"], same["ldj"])
    tri = flow.TriangularSylvester(5)
    zk, r1, r2, bias, perm = r["in_zk"], r["in_r1"], r["in_r2"], r["in_b"], r["perm"]
    z, ldj = tri.forward(zk, r1, r2, bias, perm)
    assert torch.equal(z, r["z"]) and torch.equal(ldj, r["ldj"])
    z_none, _ = tri.forward(zk, r1, r2, bias, None)   # "b" = None: no permutation
    assert torch.equal(z_none, _rec(g19, "f32", "tri_none")["z"])
    with pytest.raises((IndexError, TypeError, RuntimeError)):
        tri.forward(zk, r1, r2, perm, bias)            # the order the argument names suggest does not work


def test_second_gather_is_forward_not_inverse(g19):
    """z'[i] = z[i] + w[p[i]] with the index of the input gather; for a 5-cycle that differs from the inverse scatter, for
    the flip (an involution) it does not."""
    for name, differs in (("tri_perm", True), ("tri_flip", False)):
        r = _rec(g19, "f64", name)
        zk, r1, r2, b, p = r["in_zk"], r["in_r1"], r["in_r2"], r["in_b"], r["perm"]
        w = torch.bmm(torch.tanh(torch.bmm(zk[:, None, p], r2.transpose(2, 1)) + b), r1.transpose(2, 1)).squeeze(1)
        forward_gather = zk + w[:, p]
        inverse = zk.clone()
        inverse[:, p] += w
        torch.testing.assert_close(r["z"], forward_gather, rtol=0, atol=1e-12)
        assert (not torch.allclose(forward_gather, inverse, atol=1e-6)) == differs
        z, _, _ = se.forward(zk.unsqueeze(0), r1.unsqueeze(1), r2.unsqueeze(1), b, None, p.unsqueeze(0))
        torch.testing.assert_close(z[0], forward_gather, rtol=0, atol=1e-12)
    for doc in (flow.sylvester_chain.__doc__, flow.TriangularSylvester.__doc__):   # and the docstrings say so
        assert "forward gather, not the inverse" in " ".join(doc.split())


# ------------------------------------------------------------------------------------------------------ 4. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _sylvester_lib as SL
    return abi_checks.built(SL.LIBRARY)


def test_header_functions_are_exported_and_bound(lib):
    from hode import _sylvester_lib as SL
    declared = abi_checks.declared_functions("hode_sylvester.h", "hode_sylvester_")
    assert declared == {name for name, _, _ in SL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_sylvester.h")
    assert "#define HODE_SYLVESTER_ABI_VERSION %d\n" % SL.HODE_SYLVESTER_ABI_VERSION in src
    assert lib.hode_sylvester_version() == SL.HODE_SYLVESTER_ABI_VERSION
    consts = {k: int(v) for k, v in re.findall(r"#define (HODE_SYLVESTER_[A-Z_]+) (-?\d+)", src)}
    assert (consts["HODE_SYLVESTER_MAX_LATENT"], consts["HODE_SYLVESTER_MAX_ORTHO"], consts["HODE_SYLVESTER_MAX_FLOWS"],
            consts["HODE_SYLVESTER_MAX_SAMPLES"]) == (SL.MAX_LATENT, SL.MAX_ORTHO, SL.MAX_FLOWS, SL.MAX_SAMPLES) == (32, 32, 16, 256)
    assert (consts["HODE_SYLVESTER_E_NULL"], consts["HODE_SYLVESTER_E_SIZE"], consts["HODE_SYLVESTER_E_WORKSPACE"]) == \
        (SL.E_NULL, SL.E_SIZE, SL.E_WORKSPACE) == (E_NULL, E_SIZE, E_WORKSPACE)


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _sylvester_lib as SL
    abi_checks.assert_c_layout("hode_sylvester.h", "hode_sylvester_desc", SL.SylvesterDesc, tmp_path)
    assert SL.new_desc().struct_size == __import__("ctypes").sizeof(SL.SylvesterDesc)


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_sylvester.h" and row.src_dir == build_hip.PKG + "/csrc/sylvester"
    assert [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()] == \
        [("hode_sylvester", row.src_dir + "/hode_sylvester.hip", [])]
    assert {build_hip.PKG + "/csrc/hode_common.hpp", build_hip.PKG + "/csrc/hode_side_error.hpp",
            "include/hode_sylvester.h"} <= set(build_hip.digest_files(LIB))
    from hode import _sylvester_lib as SL
    assert SL.LIBRARY.noun.startswith("the Sylvester flows")   # what the loader says has no CPU fallback


def test_new_device_helpers_stay_in_the_unit():
    """hode_common.hpp and hode_lanes.hpp are guarded by a helper-coverage test: this library adds nothing to them."""
    src = open(os.path.join(build_hip.CSRC, "sylvester", "hode_sylvester.hip")).read()
    assert "HODE_DEV" not in src and "hode_lanes.hpp" not in src
    assert sorted(f for f in os.listdir(os.path.join(build_hip.CSRC, "sylvester")) if f != "build") == ["hode_sylvester.hip"]


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    want = {"hode_sylvester::sylvester_%s_kernel<%d>" % (d, t) for d in ("fwd", "bwd") for t in cases.TILES}
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    covered = set().union(*(cases.kernels(c) for c in cases.CASES))
    assert covered == compiled, sorted(compiled ^ covered)
    for mode in ("dense", "tri"):   # every tile in both modes
        assert set().union(*(cases.kernels(c) for c in cases.CASES if c["mode"] == mode)) == compiled, mode
    assert not any(n.startswith("hode::") for n in compiled)   # none of them is a libhode.so family


def test_no_compiled_kernel_uses_scratch():
    row = build_hip.LIBRARIES[LIB]
    objs = sorted(glob.glob(os.path.join(row.obj, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    seen = set()
    for o in objs:
        for dem, kd in kernel_descriptors(o):
            assert struct.unpack_from("<I", kd, 4)[0] == 0, dem   # private_segment_fixed_size of the kernel descriptor
            seen.add(dem)
    assert len(seen) == 8


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    dense = [c for c in cs if c["mode"] == "dense"]
    tri = [c for c in cs if c["mode"] == "tri"]
    assert {(c["D"], c["M"]) for c in dense} >= set(cases.DENSE_DM) and len(cases.DENSE_DM) == 10
    assert {(c["D"], c["perm"]) for c in tri} >= {(D, p) for D in cases.TRI_D for p in cases.PERMS} and all(c["D"] == c["M"] for c in tri)
    for group in (dense, tri):
        assert {c["K"] for c in group} >= {1, 2, 16} and {c["S"] for c in group} >= {1, 3, 64, 65, 256}
        assert {c["B"] for c in group} >= {1, 2, 7, 65}
    assert sum(c["B"] == cases.BIG_B for c in cs) == 1 and cases.BIG_B == 4099 and len(cases.subset(cases.BIG_B)) == 192
    assert cases.subset(65) is None
    assert any(c["D"] == 32 and c["S"] > 64 and c["K"] == 16 for c in dense)   # the largest tile, several rounds, streamed flows
    assert any(c["S"] == 65 and c["B"] == 7 for c in cs)
    ins = cases.inputs(cases.CASES[4])
    for r in (ins["r1"], ins["r2"]):
        assert (torch.tril(r, diagonal=-1).abs().max() > 0) and (torch.tril(r, diagonal=-1).abs().max() < 0.2)   # dense, small
    dd = torch.diagonal(ins["r1"], dim1=-2, dim2=-1) * torch.diagonal(ins["r2"], dim1=-2, dim2=-1)
    assert dd.abs().max() <= 0.9
    qtq = ins["q"].transpose(-1, -2) @ ins["q"]
    assert (qtq - torch.eye(qtq.shape[-1])).abs().max() < 0.2


# ------------------------------------------------------------------------------------------------ 5. refusals, no GPU
def _desc(**over):
    from hode import _sylvester_lib as SL
    d = SL.new_desc()
    d.batch, d.latent_dim, d.n_ortho, d.n_flows, d.n_samples = 7, 6, 4, 3, 51
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_argument_errors_do_not_launch(lib):
    err = lib.hode_sylvester_last_error_string
    fwd, bwd, ws = lib.hode_sylvester_fwd, lib.hode_sylvester_bwd, lib.hode_sylvester_workspace_bytes
    ptrs = {k: 64 for k in ("z0", "r1", "r2", "b", "q")}
    for fn in (fwd, bwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        for field, bad in (("batch", 0), ("latent_dim", 0), ("latent_dim", 33), ("n_ortho", 0), ("n_ortho", 33), ("n_flows", 0),
                           ("n_flows", 17), ("n_samples", 0), ("n_samples", 257)):
            assert fn(_desc(**dict(ptrs, **{field: bad})), None) == E_SIZE and field.encode() in err(), field
        assert fn(_desc(**dict(ptrs, q=None)), None) == E_SIZE and b"triangular mode" in err()   # M 4 != D 6
        assert fn(_desc(perm=64, **ptrs), None) == E_SIZE and b"perm belongs to triangular mode" in err()
        assert fn(_desc(n_ortho=6), None) == E_NULL and b"z0 / r1 / r2 / b" in err()
    assert fwd(_desc(**ptrs), None) == E_NULL and b"z_out / logdet" in err()
    outs = dict(ptrs, z_out=64, logdet=64)
    need = ws(_desc())
    assert need == -(-2 * 51 * 7 * 6 * 4 // 256) * 256 and ws(_desc(n_flows=1)) == 0
    for bad in (_desc(batch=0), _desc(latent_dim=33), _desc(n_flows=17), _desc(n_samples=0), _desc(struct_size=8)):
        assert ws(bad) == 0
    assert fwd(_desc(workspace=64, workspace_bytes=need - 1, **outs), None) == E_WORKSPACE and b"workspace %d B < required %d B" % (need - 1, need) in err()
    assert fwd(_desc(workspace=68, workspace_bytes=need, **outs), None) == E_WORKSPACE and b"16-byte aligned" in err()
    assert bwd(_desc(**ptrs), None) == E_NULL and b"grad_z0 / grad_r1 / grad_r2 / grad_b" in err()
    grads = dict(ptrs, grad_z0=64, grad_r1=64, grad_r2=64, grad_b=64)
    assert bwd(_desc(**grads), None) == E_NULL                                                     # dense mode: grad_q
    grads["grad_q"] = 64
    assert bwd(_desc(**grads), None) == E_WORKSPACE and b"workspace is NULL" in err()            # K = 3 reads the tape
    assert bwd(_desc(workspace=64, workspace_bytes=need - 1, **grads), None) == E_WORKSPACE


def test_domain_refusals():
    from hode import HodeConfigError
    from hode.sylvester import check_domain
    check_domain(1, 1, 1, 1, 1)
    check_domain(100003, 32, 32, 16, 256)
    check_domain(7, 32, 1, 4, 50)
    check_domain(7, 6, 6, 4, 50, dense=False)
    for bad in ((0, 6, 4, 4, 50), (7, 0, 4, 4, 50), (7, 33, 4, 4, 50), (7, 6, 0, 4, 50), (7, 6, 33, 4, 50), (7, 6, 4, 0, 50),
                (7, 6, 4, 17, 50), (7, 6, 4, 4, 0), (7, 6, 4, 4, 257)):
        with pytest.raises(HodeConfigError):
            check_domain(*bad)
    with pytest.raises(HodeConfigError, match="triangular mode"):
        check_domain(7, 6, 4, 4, 50, dense=False)


def test_cpu_tensors_are_refused_by_the_launch_functions():
    from hode import HodeConfigError
    from hode.sylvester import sylvester_backward, sylvester_forward
    ins = cases.inputs(cases._case("dense", 6, 4, 2, 3, 5))
    args = [ins[k] for k in ("z0", "r1", "r2", "b", "q")]
    with pytest.raises(HodeConfigError, match="only on a HIP device"):
        sylvester_forward(*args)
    with pytest.raises(HodeConfigError, match="only on a HIP device"):
        sylvester_backward(*args, None, None, grad_z=ins["gz"])
    # the public call takes CPU tensors down the eager path instead
    z, logdet = flow.sylvester_chain(*args)
    rz, rl, _ = se.forward(*(t.double() for t in args))
    torch.testing.assert_close(z.double(), rz, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(logdet.double(), rl, rtol=1e-5, atol=1e-5)
    tri = cases.inputs(cases._case("tri", 5, 5, 3, 4, 2, "random"))
    z, logdet, log_diag = flow.sylvester_chain(tri["z0"], tri["r1"], tri["r2"], tri["b"], None, tri["perm"], want_log_diag=True)
    rz, rl, rd = se.forward(tri["z0"].double(), tri["r1"].double(), tri["r2"].double(), tri["b"].double(), None, tri["perm"])
    torch.testing.assert_close(z.double(), rz, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(log_diag.double(), rd, rtol=1e-5, atol=1e-5)


def test_no_cotangent_means_no_launch(monkeypatch):
    """With every cotangent absent the wrapper's backward returns without touching the library (or the saved tensors)."""
    import hode.sylvester as hs
    monkeypatch.setattr(hs, "sylvester_backward", lambda *a, **k: pytest.fail("launched"))
    assert flow._SylvesterChain.backward(object(), None, None, None) == (None,) * 7
    assert flow._SylvesterChain.backward(object(), None, None, torch.zeros(())) == (None,) * 7   # the placeholder output
