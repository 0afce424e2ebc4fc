"""HIP real-data recurrent baselines (csrc/hode_seqdec.hip behind model.DecoderRealBenchmark) vs the eager restatement
(tests/seqdec_eager.py, pinned to the reference by G9 in tests/test_seqdec_host.py).  GPU only.
Tolerances as tests/test_hip_real.py: trajectory 2e-5 * (1 + max|h|), gradients rel-L2 1e-4."""
import copy
import os

import numpy as np
import pytest
import torch

import seqdec_eager

pytestmark = pytest.mark.gpu

OBS, ACT, STAT, HIDDEN = 24, 1, 11, 43


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _inputs(kind, D, B, Ta, t0, seed, dev):
    import model
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    dec = model.DecoderRealBenchmark(OBS, D, ACT, STAT, HIDDEN, Ta, 1, ode_type=kind, t0=t0, device=dev)
    init = (torch.randn(B, D, generator=gen) * 0.5).to(dev)
    a = ((torch.rand(Ta, B, ACT, generator=gen) < 0.3).float() * torch.rand(Ta, B, ACT, generator=gen) * 2).to(dev)
    s = torch.rand(Ta, B, STAT, generator=gen).to(dev)
    cot = torch.randn(Ta - t0, B, OBS, generator=gen).to(dev)
    return dec, init, a, s, cot


def _compare_with_eager(dec, init, a, s, cot):
    """GPU decoder forward + backward of sum(x_hat * cot) vs the eager restatement in fp64 on the same inputs."""
    ref = copy.deepcopy(dec).double()
    ref.t = dec.t  # the grid (and with it the fp32 time feature) is the decoder's own
    i64 = init.double().requires_grad_(True)
    xr, hr = seqdec_eager.decoder_forward(ref, i64, a.double())
    (xr * cot.double()).sum().backward()
    ig = init.clone().requires_grad_(True)
    x_hat, h = dec(ig, a, s)
    assert h.shape == hr.shape and x_hat.shape == xr.shape
    (x_hat * cot).sum().backward()
    torch.cuda.synchronize()
    tol = 2e-5 * (1 + hr.abs().max().item())
    assert (h.detach().double() - hr.detach()).abs().max().item() <= tol
    assert _rel(ig.grad, i64.grad) < 1e-4
    for (n, p), (_, q) in zip(dec.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) < 1e-4, n


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
@pytest.mark.parametrize("D", [4, 13, 20, 29])
@pytest.mark.parametrize("B", [1, 37, 100, 8191])
def test_decoder_vs_eager(kind, D, B):
    dev = _dev()
    _compare_with_eager(*_inputs(kind, D, B, 30, 8, 100 * D + B, dev))


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
@pytest.mark.parametrize("D", [4, 20])
def test_single_step(kind, D):
    """t0 = t_max - 1: T' = 1."""
    dev = _dev()
    dec, init, a, s, cot = _inputs(kind, D, 19, 30, 29, 7 + D, dev)
    assert dec.t.numel() == 1
    _compare_with_eager(dec, init, a, s, cot)


def test_golden_g9_on_the_gpu(golden_dir):
    import model
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g9_seqdec.npz"), allow_pickle=False)
    for ci in range(int(g["n_cases"])):
        pre = "c%d_" % ci
        D, t0, B, TA, obs, seed = (int(v) for v in g[pre + "meta"])
        dec = model.DecoderRealBenchmark(obs, D, ACT, STAT, HIDDEN, TA, 1, ode_type=str(g[pre + "kind"]), t0=t0, device=dev)
        dec.load_state_dict({k: torch.from_numpy(g[pre + "sd_" + k.replace(".", "__")]) for k in dec.state_dict()})
        init = torch.from_numpy(g[pre + "init"]).to(dev).requires_grad_(True)
        a = torch.from_numpy(g[pre + "a"]).to(dev)
        x_hat, h = dec(init, a, None)
        (x_hat * torch.from_numpy(g[pre + "cot"]).to(dev)).sum().backward()
        href = torch.from_numpy(g[pre + "h"])
        assert (h.detach().cpu() - href).abs().max().item() <= 2e-5 * (1 + href.abs().max().item())
        xref = torch.from_numpy(g[pre + "x_hat"])
        assert (x_hat.detach().cpu() - xref).abs().max().item() <= 2e-5 * (1 + xref.abs().max().item())
        assert _rel(init.grad, torch.from_numpy(g[pre + "g_init"])) < 1e-4
        for n, p in dec.named_parameters():
            assert _rel(p.grad, torch.from_numpy(g[pre + "g_" + n.replace(".", "__")])) < 1e-4, (ci, n)


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
def test_backward_is_bitwise_reproducible(kind):
    dev = _dev()
    dec, init, a, s, cot = _inputs(kind, 20, 1000, 30, 8, 3, dev)
    grads = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        ig = init.clone().requires_grad_(True)
        x_hat, _ = dec(ig, a, s)
        (x_hat * cot).sum().backward()
        grads.append([ig.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    for g0, g1 in zip(*grads):
        assert torch.equal(g0, g1)


def _vi(kind, dev, B=100, T=48, t0=24, seed=5):
    import model
    gen = torch.Generator().manual_seed(seed)
    input_dim = OBS + ACT + STAT + 1
    torch.manual_seed(seed)
    enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), 20, output_all=False, reverse=False, device=dev)
    dec = model.DecoderRealBenchmark(OBS, 20, ACT, STAT, HIDDEN, T, 1, ode_type=kind, t0=t0, device=dev)
    data = {"measurements": torch.randn(T, B, OBS, generator=gen).to(dev),
            "actions": ((torch.rand(T, B, ACT, generator=gen) < 0.15).float() * torch.rand(T, B, ACT, generator=gen)).to(dev),
            "masks": (torch.rand(T, B, OBS, generator=gen) < 0.5).float().to(dev),
            "statics": torch.rand(1, B, STAT, generator=gen).expand(T, B, STAT).contiguous().to(dev)}
    return enc, dec, data


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
@pytest.mark.parametrize("weight", [False, True])
def test_fused_and_unfused_vi_loss_agree(kind, weight):
    import model
    dev = _dev()
    enc, dec, data = _vi(kind, dev)
    vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=24, weight=weight)
    assert dec.fused_likelihood_ok(data["measurements"])
    out = []
    for fused in (True, False):
        vi.fuse_likelihood = fused
        for p in vi.parameters():
            p.grad = None
        loss = vi.loss(data)
        loss.backward()
        out.append((loss.detach(), [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in vi.parameters()]))
    assert abs(out[0][0].item() - out[1][0].item()) <= 1e-5 * abs(out[1][0].item())
    for g0, g1 in zip(out[0][1], out[1][1]):
        assert _rel(g0, g1) < 1e-4
    assert vi.x_hat.shape[0] == 48 - 24  # no row dropped for this decoder


def test_golden_vi_loss_on_the_gpu(golden_dir):
    import model
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g9_seqdec.npz"), allow_pickle=False)
    for vi_i in range(2):
        pre = "vi%d_" % vi_i
        D, t0, B, T, obs, seed = (int(v) for v in g[pre + "meta"])
        input_dim = obs + ACT + STAT + 1
        enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=dev)
        dec = model.DecoderRealBenchmark(obs, D, ACT, STAT, HIDDEN, T, 1, ode_type=str(g[pre + "kind"]), t0=t0, device=dev)
        for mod, tag in ((enc, "enc_"), (dec, "dec_")):
            mod.load_state_dict({k: torch.from_numpy(g[pre + tag + k.replace(".", "__")]) for k in mod.state_dict()})
        vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0, weight=False)
        data = {k: torch.from_numpy(g[pre + k]).to(dev) for k in ("measurements", "actions", "masks", "statics")}
        loss = vi.loss(data)
        loss.backward()
        ref = float(g[pre + "loss"])
        assert abs(loss.item() - ref) <= 1e-4 * (1 + abs(ref))
        for mod, tag in ((enc, "genc_"), (dec, "gdec_")):
            for n, p in mod.named_parameters():
                ref_g = torch.from_numpy(g[pre + tag + n.replace(".", "__")])
                got = torch.zeros_like(ref_g) if p.grad is None else p.grad.cpu()
                if ref_g.abs().max() == 0:  # elbo=False: the log-variance head takes no gradient
                    assert got.abs().max() == 0, (vi_i, n)
                else:
                    assert _rel(got, ref_g) < 1e-4, (vi_i, n)


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
def test_training_loop_and_evaluate_at_run_real_shapes(kind, tmp_path, golden_dir):
    """run_real.py's construction (obs 24, statics 11, D 20, batch 100, t0 24): two iterations of the mirrored training
    loop on DeviceFolds, a finite loss, a checkpoint with the reference's decoder keys; evaluate(real=True) runs."""
    import model
    import training_utils
    from hode.batches import DeviceFolds
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g9_seqdec.npz"), allow_pickle=False)
    obs_dim, action_dim, static_dim, t_max, step_size, t0, method = OBS, ACT, STAT, 48, 1, 24, kind
    encoder_output_dim = 20
    hidden_dim = int((obs_dim + action_dim + static_dim) * 1.2)
    input_dim = obs_dim + action_dim + static_dim + 1
    N = 400
    gen = torch.Generator().manual_seed(11)
    folds = DeviceFolds(torch.randn(t_max, N, obs_dim, generator=gen),
                        (torch.rand(t_max, N, 1, generator=gen) < 0.15).float() * torch.rand(t_max, N, 1, generator=gen),
                        torch.zeros(t_max, N, 4), (torch.rand(t_max, N, obs_dim, generator=gen) < 0.5).float(), 100, 100,
                        statics=torch.rand(1, N, static_dim, generator=gen).expand(t_max, N, static_dim), device=dev)
    torch.manual_seed(0)
    encoder = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), encoder_output_dim, output_all=False, reverse=False)
    decoder = model.DecoderRealBenchmark(
        obs_dim, encoder_output_dim, action_dim, static_dim, hidden_dim, t_max, step_size, ode_type=method, t0=t0
    )
    vi = model.VariationalInferenceReal(encoder, decoder, elbo=False, t0=t0)
    opt = torch.optim.Adam(vi.parameters(), lr=1e-3)
    vi, best, _ = training_utils.variational_training_loop(2, folds, vi, 100, opt, 1, path=str(tmp_path) + "/")
    assert np.isfinite(best) and best < 1e9
    ck = torch.load(str(tmp_path) + "/" + vi.model_name, map_location="cpu")
    pre = "c%d_" % [str(g["c%d_kind" % i]) for i in range(int(g["n_cases"]))].index(kind)
    assert list(ck["decoder_state_dict"].keys()) == [str(k) for k in g[pre + "sd_keys"]]
    eval_dec = model.DecoderRealBenchmark(obs_dim, encoder_output_dim, action_dim, static_dim, hidden_dim, t_max, step_size,
                                          ode_type=method, t0=0)
    eval_dec.load_state_dict(decoder.state_dict())
    out = training_utils.evaluate(model.VariationalInferenceReal(encoder, eval_dec, elbo=False, t0=t0), folds, 50, t0,
                                  mc_itr=3, real=True)
    assert len(out) == 6 and np.isfinite(out[3])


@pytest.mark.parametrize("kind", ["tlstm", "gruode"])
def test_full_size_vs_eager(kind):
    """8 192 patients, t_max 120, t0 24 (T' = 96), D 20."""
    dev = _dev()
    _compare_with_eager(*_inputs(kind, 20, 8192, 120, 24, 42, dev))
