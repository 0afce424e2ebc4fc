"""CPU checks of the Sylvester-flow posterior (no GPU): the log-determinant against autograd's Jacobian, the structure of
r1, r2, Q and the flips, the eager path against the float64 restatement (snf_eager), model.EncoderSylvesterLSTM's surface,
VariationalInferenceFlow and evaluate_flow end to end with either encoder, the planar encoder unchanged through the new
dispatch, libhode_snf.so's C ABI and build-table row, the compiled kernels against the GPU case
table (tests/snf_cases.py), and the domain refusals."""
import glob
import inspect
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
import model
import snf_cases as cases
import snf_eager as se
import training_utils
from oracle.solvers import odeint as oracle_odeint

ROOT = build_hip.ROOT
LIB = "libhode_snf.so"
FUNCTIONS = {"hode_snf_" + n for n in ("version", "last_error_string", "workspace_bytes", "fwd", "bwd")}
E_NULL, E_SIZE, E_WORKSPACE = -1, -2, -3
CPU = torch.device("cpu")
OBS, ACT, HIDDEN = 20, 1, 40
TYPES = ("triangular", "householder")


def _heads64(c, seed=None):
    ins = cases.inputs(c, seed)
    return ins, [None if ins[k] is None else ins[k].double() for k in cases.HEADS]


# ------------------------------------------------------------------------------------------------- 1. the Jacobian
@pytest.mark.parametrize("D", [1, 2, 5, 6])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H", [0, 1, 2, 3])
def test_logdet_is_the_jacobians(D, K, H):
    """Independent of anyone's formulas: logdet - sum(z_K - 5) = log|det d z_K / d z_0| from autograd's Jacobian of the
    product's eager chain, in float64, per patient and draw."""
    c = cases._case("hh" if H else "tri", D, K, 2, 3, H)
    ins, (mu, lv, fd, d1, d2, b, v) = _heads64(c)
    r1, r2, q, perm = flow.sylvester_flow_parameters(fd, d1, d2, v)
    z0 = ins["noise"].double() * torch.exp(0.5 * lv) + mu
    zK, logdet = flow.sylvester_chain(z0, r1, r2, b, q, perm)
    for s in range(2):
        for i in range(3):
            def one(z):
                return flow.sylvester_chain(z.reshape(1, 1, D), r1[i:i + 1], r2[i:i + 1], b[i:i + 1],
                                            None if q is None else q[i:i + 1], perm)[0].reshape(D)
            jac = torch.autograd.functional.jacobian(one, z0[s, i])
            sign, logabs = torch.linalg.slogdet(jac)
            assert sign > 0   # |r1_mm r2_mm| < 1 keeps every flow orientation-preserving (and Q appears twice)
            assert abs(logabs.item() - logdet[s, i].item()) < 1e-10
    # and the posterior's logdet is the chain's plus the output layer's: the restatement states it separately
    _, _, full_logdet, _ = se.forward(mu, lv, fd, d1, d2, b, v, ins["noise"].double(), 0)
    torch.testing.assert_close(full_logdet - (zK - 5.0).sum(-1), logdet, rtol=0, atol=1e-10)


# ------------------------------------------------------------------------------------------------- 2. structure
def test_r1_r2_are_upper_triangular_with_diagonals_inside_the_unit_interval():
    ins = cases.inputs(cases._case("tri", 7, 3, 2, 4))
    fd = ins["full_d"]
    r1, r2, q, perm = flow.sylvester_flow_parameters(fd, 5.0 * ins["diag1"], 5.0 * ins["diag2"])
    assert q is None
    for r in (r1, r2):
        assert r.shape == fd.shape and bool((torch.tril(r, diagonal=-1) == 0).all())
        assert torch.diagonal(r, dim1=-2, dim2=-1).abs().max() < 1
    up = torch.triu(torch.ones(7, 7), diagonal=1).bool()
    assert torch.equal(r1[..., up], fd[..., up]) and torch.equal(r2[..., up], fd.transpose(-1, -2)[..., up])
    assert torch.equal(torch.diagonal(r1, dim1=-2, dim2=-1), torch.tanh(5.0 * ins["diag1"]))
    er1, er2, _ = se.parameters(fd, 5.0 * ins["diag1"], 5.0 * ins["diag2"])
    assert torch.equal(r1, er1) and torch.equal(r2, er2)


@pytest.mark.parametrize("H", [1, 2, 8])
def test_householder_q_is_orthogonal_in_float32(H):
    g = torch.Generator().manual_seed(H)
    v = torch.randn(3, 2, H, 32, generator=g)
    fd = torch.zeros(3, 2, 32, 32)
    _, _, q, perm = flow.sylvester_flow_parameters(fd, torch.zeros(3, 2, 32), torch.zeros(3, 2, 32), v)
    assert perm is None and q.dtype == torch.float32 and q.shape == (3, 2, 32, 32)
    assert (q.transpose(-1, -2) @ q - torch.eye(32)).abs().max() < 1e-6
    _, _, eq = se.parameters(fd.double(), torch.zeros(3, 2, 32).double(), torch.zeros(3, 2, 32).double(), v.double())
    assert (q.double() - eq).abs().max() < 1e-6
    if H == 1:   # one reflection: I - 2 v v^T / |v|^2
        w = v[:, :, 0] / v[:, :, 0].norm(dim=-1, keepdim=True)
        torch.testing.assert_close(q, torch.eye(32) - 2 * w.unsqueeze(-1) * w.unsqueeze(-2), rtol=0, atol=1e-6)


def test_odd_flows_flip():
    _, _, _, perm = flow.sylvester_flow_parameters(torch.zeros(2, 5, 4, 4), torch.zeros(2, 5, 4), torch.zeros(2, 5, 4))
    assert perm.shape == (5, 4) and perm.dtype == torch.int64
    for k in range(5):
        assert perm[k].tolist() == ([0, 1, 2, 3] if k % 2 == 0 else [3, 2, 1, 0])
        assert torch.equal(perm[k][perm[k]], torch.arange(4))   # an involution: the forward gather is the inverse


# ------------------------------------------------------------------------------------------- 3. eager consistency
@pytest.mark.parametrize("case", [cases._case("tri", 6, 4, 5, 3), cases._case("hh", 6, 4, 5, 3, 3), cases._case("hh", 5, 3, 4, 2, 8, 0),
                                  cases._case("tri", 1, 2, 3, 2)], ids=cases.case_id)
def test_cpu_eager_path_against_the_float64_restatement(case):
    ins, heads64 = _heads64(case)
    heads = [ins[k] for k in cases.HEADS]
    z, kl = flow.sylvester_posterior_sample(*heads, ins["noise"], ins["s_kl"])
    rz, rk, _, _ = se.forward(*heads64, ins["noise"].double(), ins["s_kl"])
    assert z.dtype == torch.float32 and z.shape == rz.shape and kl.shape == rk.shape
    assert (z.double() - rz).abs().max() <= 1e-5 * rz.abs().max()
    assert (kl.double() - rk).abs().max() <= 1e-5 * rk.abs().max()
    none, kl2 = flow.sylvester_posterior_sample(*heads, ins["noise"], ins["s_kl"], want_z=False)
    assert none is None and torch.equal(kl, kl2)
    # gradients in float64: the eager path differentiates to the restatement's numbers
    leaves = [None if h is None else h.clone().requires_grad_(True) for h in heads64]
    z64, kl64 = flow.sylvester_posterior_sample(*leaves, ins["noise"].double(), ins["s_kl"])
    grads = torch.autograd.grad((z64 * ins["gz"].double()).sum() + (kl64 * ins["gk"].double()).sum(), [t for t in leaves if t is not None])
    _, _, rgrads = se.forward_backward(*heads, ins["noise"], ins["s_kl"], grad_z=ins["gz"], grad_kl=ins["gk"])
    for n, got, ref in zip(cases.HEADS, grads, [g for g in rgrads if g is not None]):
        assert (got - ref).abs().max() <= 1e-9 * (1 + ref.abs().max()), n


@pytest.mark.parametrize("flow_type", TYPES)
def test_flow_draws_are_s_reparameterize_calls(flow_type):
    torch.manual_seed(0)
    enc = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 4, flow_type=flow_type, num_householder=3, normalize=False, device=CPU)
    g = torch.Generator().manual_seed(1)
    x, a, m = torch.randn(7, 3, OBS, generator=g), torch.zeros(7, 3, 1), torch.ones(7, 3, OBS)
    with torch.no_grad():
        eo = enc(x, a, m)
        eps = torch.randn(4, 3, 6, generator=g)
        z_out, ldj, z0 = enc.flow_draws(*eo, eps)
        assert z_out.shape == (4, 3, 6) and ldj.shape == (4, 3) and z0.shape == (4, 3, 6)
        for s in range(4):
            orig = torch.randn_like
            torch.randn_like = lambda *args, **kw: eps[s].clone()
            try:
                mu, lv, z_exp, ld, z0_s = enc.reparameterize(*eo)
            finally:
                torch.randn_like = orig
            assert z_exp.shape == (3, 6) and ld.shape == (3,) and z0_s.shape == (3, 6)
            torch.testing.assert_close(z_exp, z_out[s], rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(ld, ldj[s], rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(z0_s, z0[s], rtol=0, atol=0)
            assert enc.log_density(mu, lv, z_exp, ld, z0_s).shape == (3,)
        # posterior_sample is flow_draws + log_density against the Exponential(100) prior
        z2, kl = enc.posterior_sample(eo, eps, 1)
        log_q = enc.log_density(eo[0], eo[1], z_out, ldj, z0)
        torch.testing.assert_close(z2, z_out, rtol=1e-6, atol=1e-8)
        torch.testing.assert_close(kl, (log_q - model.ExponentialPrior.log_density(z_out))[1:].mean(0), rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------- 4. the encoder
@pytest.mark.parametrize("flow_type,H", [("triangular", None), ("householder", None), ("householder", 2)])
def test_encoder_surface(flow_type, H):
    D, K = 6, 4
    torch.manual_seed(0)
    enc = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, D, K, flow_type=flow_type, num_householder=H, device=CPU)
    n_h = 0 if flow_type == "triangular" else (D if H is None else H)
    assert enc.num_householder == n_h and enc.z_size == D and enc.num_flows == K and enc.q_z_nn_output_dim == HIDDEN
    assert enc.flow_type == flow_type and enc.normalize is True
    heads = ["lin", "log_var", "amor_d", "amor_diag1", "amor_diag2", "amor_b"] + (["amor_q"] if n_h else [])
    want = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"]
    want += [h + s for h in heads for s in (".weight", ".bias")]
    want += ["flow_%d.%s" % (k, b) for k in range(K) for b in (("diag_idx",) if n_h == 0 else ("triu_mask", "diag_idx"))]
    assert list(enc.state_dict().keys()) == want
    assert [n for n, _ in enc.named_children()] == ["lstm"] + heads + ["flow_%d" % k for k in range(K)]   # creation order
    assert all(isinstance(getattr(enc, "flow_%d" % k), flow.TriangularSylvester if n_h == 0 else flow.Sylvester) for k in range(K))
    assert enc.amor_d.out_features == K * D * D and enc.amor_diag1.out_features == enc.amor_b.out_features == K * D
    if n_h:
        assert enc.amor_q.out_features == K * n_h * D
    # the same seed gives the same lstm / lin / log_var as EncoderLSTM: the creation order starts alike
    torch.manual_seed(0)
    plain = model.EncoderLSTM(OBS + ACT, HIDDEN, D, device=CPU)
    assert all(torch.equal(plain.state_dict()[k], enc.state_dict()[k]) for k in plain.state_dict())
    x, a, m = torch.randn(7, 3, OBS), torch.zeros(7, 3, 1), torch.ones(7, 3, OBS)
    out = enc(x, a, m)
    assert len(out) == 7
    mu, lv, fd, d1, d2, b, v = out
    assert mu.shape == lv.shape == (3, D) and fd.shape == (3, K, D, D) and d1.shape == d2.shape == b.shape == (3, K, D)
    assert (v is None) if n_h == 0 else (v.shape == (3, K, n_h, D))
    h = enc.final_hidden(x, a, m)
    torch.testing.assert_close(mu, torch.exp(enc.lin(h)) / 10)          # the normalize rule of the other encoders
    torch.testing.assert_close(lv, enc.log_var(h) - 5.0)
    torch.testing.assert_close(fd, enc.amor_d(h).reshape(3, K, D, D))   # raw heads: no mask, no tanh
    torch.testing.assert_close(d1, enc.amor_diag1(h).reshape(3, K, D))
    assert list(inspect.signature(model.EncoderSylvesterLSTM.__init__).parameters) == \
        ["self", "input_dim", "hidden_dim", "output_dim", "num_flows", "flow_type", "num_householder", "normalize", "device"]


def test_model_names_and_refusals():
    tri = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 2, device=CPU)
    hh = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 2, flow_type="householder", device=CPU)
    planar = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 2, device=CPU)
    assert len({tri.model_name, hh.model_name, planar.model_name}) == 3
    assert "Triangular" in tri.model_name and "Householder" in hh.model_name
    with pytest.raises(ValueError, match="orthogonal"):
        model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 2, flow_type="orthogonal", device=CPU)
    with pytest.raises(ValueError, match="num_householder"):
        model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 2, flow_type="householder", num_householder=0, device=CPU)
    with pytest.raises(RuntimeError, match="batch size 1"):
        tri(torch.zeros(5, 1, OBS), torch.zeros(5, 1, 1), torch.ones(5, 1, OBS))


# ------------------------------------------------------------------------------------------------- 5. end to end
def _vi(flow_type, mc, planar=False, normalize=False):
    torch.manual_seed(3)
    if planar:
        enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=normalize, device=CPU)
    else:
        enc = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 4, flow_type=flow_type, num_householder=3, normalize=normalize, device=CPU)
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 8.0, 1.0, roche=True, method="rk4", device=CPU)
    dec._odeint = oracle_odeint
    return model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=mc)


def _data(B=3, T=9, seed=4):
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(T, B, 1)
    a[torch.randint(0, T - 1, (B,), generator=g), torch.arange(B), 0] = torch.rand(B, generator=g) * 5
    return {"measurements": 0.5 * torch.randn(T, B, OBS, generator=g), "actions": a,
            "masks": (torch.rand(T, B, OBS, generator=g) < 0.6).float()}


@pytest.mark.parametrize("flow_type", TYPES)
@pytest.mark.parametrize("mc", [1, 5])
def test_loss_and_backward_on_the_cpu(flow_type, mc):
    vi = _vi(flow_type, mc)
    assert vi.model_name == "VI_FLOW_%s_HybridDecoder.pkl" % vi.encoder.model_name
    data = _data()
    noise = 0.5 * torch.randn(1 if mc == 1 else 1 + mc, 3, 6, generator=torch.Generator().manual_seed(5))
    vi.noise = lambda n, like: noise[:n].clone()
    loss = vi.loss(data)
    loss.backward()
    assert loss.dim() == 0 and torch.isfinite(loss)
    for n, p in vi.encoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    # the loss is the likelihood of draw 0 plus the KL the encoder's posterior_sample states
    with torch.no_grad():
        eo = vi.encoder(data["measurements"], data["actions"], data["masks"])
        z_all, kl = vi.encoder.posterior_sample(eo, noise, 0 if mc == 1 else 1)
        x_hat, _ = vi.decoder(z_all[0], data["actions"])
        lik = torch.sum((data["measurements"] - x_hat) ** 2 * data["masks"]) / 3
        want = lik + torch.mean(-kl if mc == 1 else kl)
    torch.testing.assert_close(loss.detach(), want, rtol=1e-5, atol=1e-5)
    # the refusals of the planar posterior stay
    vi.prior_log_pdf = None
    with pytest.raises(TypeError):
        vi.loss(data)


@pytest.mark.parametrize("flow_type", TYPES + ("planar",))
def test_evaluate_flow_on_the_cpu(flow_type, monkeypatch, capsys):
    from test_evaluate import FakeGenerator, oracle_ensemble_crps
    vi = _vi(flow_type, 5, planar=flow_type == "planar", normalize=True)   # latents in the solver's range
    dg = FakeGenerator(6, 9, OBS, 6, seed=2, step=1.0)
    monkeypatch.setattr(training_utils, "_ensemble_crps", oracle_ensemble_crps)
    torch.manual_seed(7)
    out = training_utils.evaluate_flow(vi, dg, 3, 4, mc_itr=4)
    lines = capsys.readouterr().out.strip().split("\n")
    assert [line.split(",")[0] for line in lines] == ["rmse_z0", "rmse_x", "cprs_z0", "cprs_x"]
    assert len(out) == 6 and all(np.isfinite(v) for v in out)
    with pytest.raises(ValueError):
        training_utils.evaluate_flow(vi, dg, 3, 4, real=True)


def test_planar_encoder_is_unchanged_through_the_dispatch():
    """flow_kl and posterior_sample with EncoderPlanarLSTM: bit for bit what flow_draws + log_density gave before."""
    vi = _vi(None, 5, planar=True)
    data = _data()
    noise = torch.randn(6, 3, 6, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        eo = vi.encoder(data["measurements"], data["actions"], data["masks"])
        z_out, ldj, z0 = vi.encoder.flow_draws(*eo, noise)
        log_q = vi.encoder.log_density(eo[0], eo[1], z_out, ldj, z0)
        want_kl = torch.mean((log_q - model.ExponentialPrior.log_density(z_out))[1:], dim=0)
        for got_z, got_kl in (vi.flow_kl(eo, noise, 1), vi.encoder.posterior_sample(eo, noise, 1)):
            assert torch.equal(got_z, z_out) and torch.equal(got_kl, want_kl)
    # on the device the planar encoder's draws are hode.flow.planar_flow_sample's, called with the same arguments
    src = inspect.getsource(model.EncoderPlanarLSTM.posterior_sample)
    assert "planar_flow_sample(mu, log_var, u, w, b, eps, s_kl)" in src
    vi.prior_log_pdf = model.StandardNormalPrior.log_density
    assert vi.flow_kl(eo, noise, 1)[1].shape == (3,)   # any prior on the CPU


def test_a_non_exponential_prior_is_refused_on_the_device_path():
    from hode import HodeConfigError

    class _Cuda(torch.Tensor):
        is_cuda = True

    vi = _vi("triangular", 5)
    vi.prior_log_pdf = model.StandardNormalPrior.log_density
    mu = torch.zeros(3, 6).as_subclass(_Cuda)
    with pytest.raises(HodeConfigError, match=r"Exponential\(100\)"):
        vi.flow_kl((mu, mu), torch.zeros(2, 3, 6), 1)


# ------------------------------------------------------------------------------------------------------ 6. ABI, build
@pytest.fixture(scope="module")
def lib():
    from hode import _snf_lib as NL
    return abi_checks.built(NL.LIBRARY)


def test_header_functions_are_exported_and_bound(lib):
    from hode import _snf_lib as NL
    declared = abi_checks.declared_functions("hode_snf.h", "hode_snf_")
    assert declared == {name for name, _, _ in NL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    src = abi_checks.header_text("hode_snf.h")
    assert "#define HODE_SNF_ABI_VERSION %d\n" % NL.HODE_SNF_ABI_VERSION in src
    assert lib.hode_snf_version() == NL.HODE_SNF_ABI_VERSION
    consts = {k: int(v) for k, v in re.findall(r"#define (HODE_SNF_[A-Z_]+) (-?\d+)", src)}
    assert (consts["HODE_SNF_MAX_LATENT"], consts["HODE_SNF_MAX_FLOWS"], consts["HODE_SNF_MAX_SAMPLES"], consts["HODE_SNF_MAX_HOUSEHOLDER"]) == \
        (NL.MAX_LATENT, NL.MAX_FLOWS, NL.MAX_SAMPLES, NL.MAX_HOUSEHOLDER) == (32, 16, 256, 8)
    assert (consts["HODE_SNF_E_NULL"], consts["HODE_SNF_E_SIZE"], consts["HODE_SNF_E_WORKSPACE"]) == \
        (NL.E_NULL, NL.E_SIZE, NL.E_WORKSPACE) == (E_NULL, E_SIZE, E_WORKSPACE)


def test_struct_layout_matches_the_c_header(tmp_path):
    from hode import _snf_lib as NL
    abi_checks.assert_c_layout("hode_snf.h", "hode_snf_desc", NL.SnfDesc, tmp_path)
    assert NL.new_desc().struct_size == __import__("ctypes").sizeof(NL.SnfDesc)


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_snf.h" and row.src_dir == build_hip.PKG + "/csrc/snf"
    assert [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()] == \
        [("hode_snf", row.src_dir + "/hode_snf.hip", [])]
    assert set(build_hip.digest_files(LIB)) == {"include/hode_snf.h", build_hip.PKG + "/csrc/snf/hode_snf.hip",
                                                build_hip.PKG + "/csrc/hode_common.hpp", build_hip.PKG + "/csrc/hode_side_error.hpp"}
    from hode import _snf_lib as NL
    assert NL.LIBRARY.noun.startswith("the Sylvester-flow posterior")   # what the loader says has no CPU fallback


def test_new_device_helpers_stay_in_the_unit():
    """hode_common.hpp and hode_lanes.hpp are guarded by a helper-coverage test: this library adds nothing to them."""
    src = open(os.path.join(build_hip.CSRC, "snf", "hode_snf.hip")).read()
    assert "HODE_DEV" not in src and "hode_lanes.hpp" not in src
    assert "atomic" not in src.lower().replace("no float atomics", "")


def _objects():
    objs = sorted(glob.glob(os.path.join(build_hip.LIBRARIES[LIB].obj, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_descriptor import kernel_descriptors
    return [(dem, kd) for o in objs for dem, kd in kernel_descriptors(o)]


def test_every_compiled_kernel_is_reached_by_a_gpu_case():
    compiled = {kv.kernel_name(dem) for dem, _ in _objects()}
    want = {"hode_snf::snf_%s_kernel<%d>" % (d, t) for d in ("fwd", "bwd") for t in cases.TILES}
    assert compiled == want, (sorted(compiled - want), sorted(want - compiled))
    for mode in ("tri", "hh"):   # every tile in both types
        assert set().union(*(cases.kernels(c) for c in cases.CASES if c["mode"] == mode)) == compiled, mode


def test_no_compiled_kernel_uses_scratch():
    seen = set()
    for dem, kd in _objects():
        assert struct.unpack_from("<I", kd, 4)[0] == 0, dem   # private_segment_fixed_size of the kernel descriptor
        seen.add(dem)
    assert len(seen) == 8


def test_the_case_table_holds_what_the_issue_lists():
    cs = cases.CASES
    for mode in ("tri", "hh"):
        group = [c for c in cs if c["mode"] == mode]
        assert {c["D"] for c in group} >= {1, 3, 4, 5, 8, 9, 16, 17, 32}
        assert {c["K"] for c in group} >= {1, 2, 3, 16} and {c["S"] for c in group} >= {1, 3, 64, 65, 256}
        assert {c["B"] for c in group} >= {1, 2, 7, 65} and {c["s_kl"] for c in group} == {0, 1}
        assert any(c["D"] == 32 and c["S"] > 64 and c["K"] == 16 for c in group)
    assert {c["H"] for c in cs if c["mode"] == "hh"} >= {1, 2, 8} and all(c["H"] == 0 for c in cs if c["mode"] == "tri")
    assert all(0 <= c["s_kl"] < c["S"] for c in cs)
    assert sum(c["B"] == cases.BIG_B for c in cs) == 1 and cases.BIG_B == 4099 and len(cases.subset(cases.BIG_B)) == 192
    assert cases.subset(65) is None and len(cs) < 40   # a covering subset, not the product
    assert any(c["S"] == 65 and c["B"] == 7 for c in cs)
    assert set(cases.OWN_BOUNDS) <= {cases.case_id(c) for c in cs}
    ins = cases.inputs(cs[-2])
    assert torch.tril(ins["full_d"], diagonal=-1).abs().max() > 0   # dense raw head: the masks are the kernels' job
    assert (torch.tanh(ins["diag1"]) * torch.tanh(ins["diag2"])).abs().max() < 0.88


# ------------------------------------------------------------------------------------------------ 7. refusals, no GPU
def _desc(**over):
    from hode import _snf_lib as NL
    d = NL.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl, d.n_householder = 7, 6, 3, 51, 1, 2
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_argument_errors_do_not_launch(lib):
    err = lib.hode_snf_last_error_string
    fwd, bwd, ws = lib.hode_snf_fwd, lib.hode_snf_bwd, lib.hode_snf_workspace_bytes
    ptrs = {k: 64 for k in ("mu", "log_var", "full_d", "diag1", "diag2", "bias", "v", "noise")}
    for fn in (fwd, bwd):
        assert fn(None, None) == E_NULL and b"NULL" in err()
        assert fn(_desc(struct_size=8), None) == E_SIZE and b"struct_size 8" in err()
        for field, bad in (("batch", 0), ("latent_dim", 0), ("latent_dim", 33), ("n_flows", 0), ("n_flows", 17), ("n_samples", 0),
                           ("n_samples", 257), ("n_householder", -1), ("n_householder", 9), ("s_kl", -1), ("s_kl", 51)):
            assert fn(_desc(**dict(ptrs, **{field: bad})), None) == E_SIZE and field.encode() in err(), field
        assert fn(_desc(), None) == E_NULL and b"mu / log_var / full_d" in err()
        assert fn(_desc(**dict(ptrs, v=None)), None) == E_NULL and b"v must be non-NULL" in err()
    need = ws(_desc())
    assert need == -(-(3 + 2) * 51 * 7 * 6 * 4 // 256) * 256
    for bad in (_desc(batch=0), _desc(latent_dim=33), _desc(n_flows=17), _desc(n_samples=0), _desc(struct_size=8)):
        assert ws(bad) == 0
    assert fwd(_desc(**ptrs), None) == E_NULL and b"kl must be non-NULL" in err()
    outs = dict(ptrs, kl=64)
    assert fwd(_desc(**outs), None) == E_WORKSPACE and b"workspace is NULL" in err()
    assert fwd(_desc(workspace=64, workspace_bytes=need - 1, **outs), None) == E_WORKSPACE and b"workspace %d B < required %d B" % (need - 1, need) in err()
    assert fwd(_desc(workspace=68, workspace_bytes=need, **outs), None) == E_WORKSPACE and b"16-byte aligned" in err()
    assert bwd(_desc(**ptrs), None) == E_NULL and b"grad_mu / grad_log_var" in err()
    grads = dict(ptrs, **{"grad_" + k: 64 for k in ("mu", "log_var", "full_d", "diag1", "diag2", "bias")})
    assert bwd(_desc(**grads), None) == E_NULL                                             # Householder type: grad_v
    assert bwd(_desc(**dict(grads, n_householder=0)), None) == E_WORKSPACE and b"workspace is NULL" in err()
    grads["grad_v"] = 64
    assert bwd(_desc(workspace=64, workspace_bytes=need - 1, **grads), None) == E_WORKSPACE


def test_domain_refusals():
    from hode import HodeConfigError
    from hode.snf import check_domain
    check_domain(1, 1, 1, 1, 0, 0)
    check_domain(100003, 32, 16, 256, 8, 255)
    check_domain(10, 6, 4, 51, 0, 1)
    for bad in ((0, 6, 4, 50, 0, 1), (7, 0, 4, 50, 0, 1), (7, 33, 4, 50, 0, 1), (7, 6, 0, 50, 0, 1), (7, 6, 17, 50, 0, 1),
                (7, 6, 4, 0, 0, 0), (7, 6, 4, 257, 0, 1), (7, 6, 4, 50, -1, 1), (7, 6, 4, 50, 9, 1), (7, 6, 4, 50, 0, -1),
                (7, 6, 4, 50, 0, 50), (7, 6, 4, 50, 0, 0.5)):
        with pytest.raises(HodeConfigError):
            check_domain(*bad)


def test_cpu_tensors_are_refused_by_the_launch_functions(monkeypatch):
    from hode import HodeConfigError, _snf_lib as NL
    from hode.snf import snf_backward, snf_forward
    monkeypatch.setattr(NL, "lib", lambda: pytest.fail("the library was loaded"))
    ins = cases.inputs(cases._case("hh", 6, 2, 3, 5, 2))
    heads = [ins[k] for k in cases.HEADS]
    with pytest.raises(HodeConfigError, match="only on a HIP device"):
        snf_forward(*heads, ins["noise"])
    with pytest.raises(HodeConfigError, match="only on a HIP device"):
        snf_backward(*heads, ins["noise"], torch.zeros(8), grad_z=ins["gz"])
    z, kl = flow.sylvester_posterior_sample(*heads, ins["noise"])   # the public call takes CPU tensors down the eager path
    assert z.shape == (3, 5, 6) and kl.shape == (5,)


def test_no_cotangent_means_no_launch(monkeypatch):
    """With every cotangent absent the wrapper's backward returns without touching the library (or the saved tensors)."""
    import hode.snf as hs
    monkeypatch.setattr(hs, "snf_backward", lambda *a, **k: pytest.fail("launched"))
    assert flow._SylvesterPosterior.backward(object(), None, None) == (None,) * 10
    assert flow._SylvesterPosterior.backward(object(), torch.zeros(()), None) == (None,) * 10   # the placeholder output
