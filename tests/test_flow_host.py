"""CPU checks of the planar-flow posterior (no GPU): the host mirror (model.EncoderPlanarLSTM, VariationalInferenceFlow)
against the reference's own numbers (G11, tests/golden/make_golden_flow.py), the float64 restatement (flow_eager)
against G11, the domain refusals, libhode_flow.so's C ABI, and the guard that every compiled flow kernel is reached by a
case of the GPU test table."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_checks
import flow_eager as fe
import model
from oracle.solvers import odeint as oracle_odeint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW_BUILD = os.path.join(ROOT, "hybrid-ode-neurips-2021_amd", "csrc", "flow", "build")
CPU = torch.device("cpu")
OBS, ACT, HIDDEN = 20, 1, 40


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_flow.npz"))


def _sd(g, pre):
    return {k[len(pre):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def _cases(g):
    for ci in range(int(g["n_cases"])):
        pre = "c%d_" % ci
        D, K, B, normalize, _, _ = (int(v) for v in g[pre + "meta"])
        yield pre, D, K, B, bool(normalize)


class _Draws:
    """torch.randn_like replaced by the recorded draws, in order."""

    def __init__(self, draws):
        self.draws, self.orig = list(draws), torch.randn_like

    def __enter__(self):
        torch.randn_like = lambda *a, **k: self.draws.pop(0).clone()
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.orig


def test_encoder_mirror_against_reference(g11):
    for pre, D, K, B, normalize in _cases(g11):
        torch.manual_seed(0)
        enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, D, K, normalize=normalize, device=CPU)
        assert list(enc.state_dict().keys()) == [str(k) for k in g11[pre + "keys"]]
        assert enc.model_name == "PlanarLSTMEncoder" and enc.z_size == D and enc.num_flows == K
        assert enc.q_z_nn_output_dim == HIDDEN
        enc.load_state_dict(_sd(g11, pre + "enc_"))
        x, a, m = (torch.from_numpy(g11[pre + k]) for k in ("x", "a", "mask"))
        with torch.no_grad():
            eo = enc(x, a, m)
            for n, t in zip(("mu", "log_var", "u", "w", "b"), eo):
                assert t.shape == g11[pre + n].shape, n
                np.testing.assert_allclose(t.numpy(), g11[pre + n], rtol=1e-5, atol=1e-6, err_msg=n)
            with _Draws([torch.from_numpy(g11[pre + "rep_eps"])]):
                mu, lv, z, ldj, z0 = enc.reparameterize(*eo)
        np.testing.assert_allclose(z.numpy(), g11[pre + "rep_z"], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(ldj.numpy(), g11[pre + "rep_log_det_j"], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(z0.numpy(), g11[pre + "rep_z0"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(enc.log_density(mu, lv, z, ldj, z0).numpy(), g11[pre + "rep_log_density"],
                                   rtol=2e-5, atol=2e-5)


def _vi(g, lp, mc):
    enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=False, device=CPU)
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 8.0, 1.0, roche=True, method="rk4", device=CPU)
    dec._odeint = oracle_odeint
    enc.load_state_dict(_sd(g, lp + "enc_"))
    dec.load_state_dict(_sd(g, lp + "dec_"))
    vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=mc)
    data = {k2: torch.from_numpy(g[lp + k]) for k, k2 in (("x", "measurements"), ("a", "actions"), ("mask", "masks"))}
    return vi, data


@pytest.mark.parametrize("mc", [1, 50])
def test_loss_mirror_against_reference(g11, mc):
    lp = "c0_m%d_" % mc
    vi, data = _vi(g11, lp, mc)
    assert vi.model_name == str(g11[lp + "model_name"]) == "VI_FLOW_PlanarLSTMEncoder_HybridDecoder.pkl"
    noise = torch.from_numpy(g11[lp + "noise"])
    assert noise.shape[0] == (1 if mc == 1 else 1 + mc)
    vi.noise = lambda n, like: noise[:n].clone()
    loss = vi.loss(data)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g11[lp + "loss"]), rtol=1e-4)
    np.testing.assert_allclose(vi.z.detach().numpy(), g11[lp + "z"], rtol=1e-5, atol=1e-8)
    for prefix, mod in (("genc_", vi.encoder), ("gdec_", vi.decoder)):
        for n, p in mod.named_parameters():
            ref = g11[lp + prefix + n.replace(".", "__")]
            got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4 * (1 + np.abs(ref).max()), err_msg=prefix + n)


def test_flow_eager_against_reference(g11):
    for pre, D, K, B, normalize in _cases(g11):
        args = [torch.from_numpy(g11[pre + n]).double() for n in ("mu", "log_var", "u", "w", "b")]
        args[2], args[3], args[4] = args[2].reshape(B, K, D), args[3].reshape(B, K, D), args[4].reshape(B, K)
        noise = torch.from_numpy(g11[pre + "rep_eps"]).double().unsqueeze(0)
        z_out, kl, log_det, z0 = fe.forward(*args, noise, 0)
        np.testing.assert_allclose(z_out[0].numpy(), g11[pre + "rep_z"], rtol=3e-5, atol=1e-7)
        np.testing.assert_allclose(log_det[0].numpy(), g11[pre + "rep_log_det_j"], rtol=3e-5, atol=3e-5)
        np.testing.assert_allclose(z0[0].numpy(), g11[pre + "rep_z0"], rtol=1e-6, atol=1e-6)
        z_ref = torch.from_numpy(g11[pre + "rep_z"]).double()
        kl_ref = torch.from_numpy(g11[pre + "rep_log_density"]).double() - model.ExponentialPrior.log_density(z_ref)
        np.testing.assert_allclose(kl.numpy(), kl_ref.numpy(), rtol=3e-5, atol=3e-3)


def test_flow_eager_softplus_threshold_and_abs_log():
    x = torch.tensor([19.0, 20.0, 20.5, 40.0], dtype=torch.float64)
    assert torch.equal(fe.softplus_t20(x)[2:], x[2:])
    torch.testing.assert_close(fe.softplus_t20(x)[:2], torch.nn.functional.softplus(x)[:2])
    # log|g| for a negative g: derivative 1/g
    g = torch.tensor([-0.5], dtype=torch.float64, requires_grad=True)
    torch.log(torch.abs(g)).sum().backward()
    assert g.grad.item() == pytest.approx(-2.0)


def test_mirror_refusals():
    enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=False, device=CPU)
    with pytest.raises(RuntimeError, match="batch size 1"):
        enc(torch.zeros(5, 1, OBS), torch.zeros(5, 1, 1), torch.ones(5, 1, OBS))
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 8.0, 1.0, roche=True, method="rk4", device=CPU)
    dec._odeint = oracle_odeint
    data = {"measurements": torch.zeros(9, 3, OBS), "actions": torch.zeros(9, 3, 1), "masks": torch.ones(9, 3, OBS)}
    for mc in (1, 50):
        vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=None, mc_size=mc)
        with pytest.raises(TypeError):
            vi.loss(data)
    # the optimiser list of the reference's run_simulation_flow.py resolves
    vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=50)
    params = (list(vi.encoder.parameters()) + list(vi.decoder.output_function.parameters())
              + list(vi.decoder.ode.ml_net.parameters()))
    assert len(params) == 14 + 2 + 2


def test_evaluate_flow_real_raises():
    import training_utils

    class _G:
        test_size, expert_dim = 4, 4

        def get_split(self, fold, batch_size, chunk):
            return {"measurements": torch.zeros(9, 2, OBS), "actions": torch.zeros(9, 2, 1), "masks": torch.ones(9, 2, OBS),
                    "latents": torch.zeros(9, 2, 6)}

    with pytest.raises(ValueError):
        training_utils.evaluate_flow(None, _G(), 2, 5, real=True)


def test_domain_refusals():
    from hode import HodeConfigError
    from hode.flow import check_domain
    check_domain(1, 1, 1, 1, 0)
    check_domain(100003, 32, 16, 256, 1)
    for bad in ((0, 6, 4, 50, 1), (7, 0, 4, 50, 1), (7, 33, 4, 50, 1), (7, 6, 0, 50, 1), (7, 6, 17, 50, 1),
                (7, 6, 4, 0, 0), (7, 6, 4, 257, 1), (7, 6, 4, 50, 2), (7, 6, 4, 1, 1)):
        with pytest.raises(HodeConfigError):
            check_domain(*bad)


# ------------------------------------------------------------------------------------------------ libhode_flow.so ABI
@pytest.fixture(scope="module")
def flow_lib():
    from hode import _flow_lib as F
    return abi_checks.built(F.LIBRARY)


def test_header_functions_are_exported_and_bound(flow_lib):
    from hode import _flow_lib as F
    declared = abi_checks.declared_functions("hode_flow.h", "hode_flow_")
    assert declared == {name for name, _, _ in F.EXPORTS}
    for name in declared:
        assert getattr(flow_lib, name) is not None
    assert flow_lib.hode_flow_version() == F.HODE_FLOW_ABI_VERSION
    consts = dict(re.findall(r"#define (HODE_FLOW_MAX_[A-Z]+) (\d+)", abi_checks.header_text("hode_flow.h")))
    assert (int(consts["HODE_FLOW_MAX_LATENT"]), int(consts["HODE_FLOW_MAX_FLOWS"]), int(consts["HODE_FLOW_MAX_SAMPLES"])) == \
        (F.MAX_LATENT, F.MAX_FLOWS, F.MAX_SAMPLES)


def test_struct_size_matches_the_c_header(tmp_path):
    from hode import _flow_lib as F
    abi_checks.assert_c_layout("hode_flow.h", "hode_flow_desc", F.FlowDesc, tmp_path)


def test_argument_errors_do_not_launch(flow_lib):
    from hode import _flow_lib as F
    assert flow_lib.hode_flow_fwd(None, None) == -1 and b"NULL" in flow_lib.hode_flow_last_error_string()
    d = F.new_desc()
    d.struct_size = 8
    assert flow_lib.hode_flow_bwd(d, None) == -2 and b"struct_size" in flow_lib.hode_flow_last_error_string()
    d = F.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl = 7, 6, 4, 51, 1
    assert flow_lib.hode_flow_fwd(d, None) == -1  # pointers missing
    for field, bad in (("latent_dim", 33), ("n_flows", 17), ("n_samples", 257), ("batch", 0), ("s_kl", 2)):
        e = F.new_desc()
        e.batch, e.latent_dim, e.n_flows, e.n_samples, e.s_kl = 7, 6, 4, 51, 1
        setattr(e, field, bad)
        assert flow_lib.hode_flow_fwd(e, None) == -2, field


def test_every_flow_kernel_is_reached_by_a_gpu_case():
    objs = sorted(glob.glob(os.path.join(FLOW_BUILD, "*.o")))
    if not objs:
        pytest.skip("object files are not in the tree (library shipped pre-built)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_variants as kv
    from kernel_descriptor import kernel_descriptors
    compiled = {kv.kernel_name(dem) for o in objs for dem, _ in kernel_descriptors(o)}
    covered = set().union(*(fe.kernels(c) for c in fe.CASES))
    assert compiled, "no kernels found in %s" % FLOW_BUILD
    assert compiled <= covered, sorted(compiled - covered)
    assert covered <= compiled, sorted(covered - compiled)
    assert not any(n.startswith("hode::") for n in compiled)  # none of them is a libhode.so family
