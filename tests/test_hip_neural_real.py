"""HIP real-data neural ODE baselines (csrc/hode_neural_real_mf.hip behind model.NeuralODEReal / NeuralODEReal2nd) vs the
eager restatement (tests/neural_real_eager.py, pinned to the reference by G10 in tests/test_neural_real_host.py), G10
through DecoderReal, reproducibility, the loss paths and run_real's shapes.  GPU only.
Tolerances: trajectory 2e-5 * (1 + max|h|), gradients rel-L2 2e-4."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import neural_real_eager

pytestmark = pytest.mark.gpu

OBS, ACT, STAT, HIDDEN = 24, 1, 11, 43


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cases():
    """Every kind x D x method once; H, B, perturb and ode_step_div cycle so that each value meets each kind and method."""
    out = []
    Hs, Bs = (1, 17, 43, 64), (1, 37, 100)
    i = 0
    for kind, Ds in (("neural", (1, 4, 13, 20, 30)), ("2nd", (2, 6, 20, 40, 60))):
        for D in Ds:
            for method in ("euler", "midpoint", "rk4"):
                out.append((kind, D, method, Hs[i % 4], Bs[i % 3], bool(i % 2), 1 + (i // 2) % 2))
                i += 1
    return out


def _run(kind, D, method, H, B, perturb, div, dev, t0=3, t_end=9, Ta=7, seed=0):
    import hode
    import model
    gen = torch.Generator().manual_seed(seed)
    cls = model.NeuralODEReal if kind == "neural" else model.NeuralODEReal2nd
    torch.manual_seed(seed)
    ode = cls(D, ACT, STAT, H, t_end, 1, device=dev)
    y0 = (torch.randn(B, D, generator=gen) * 0.5)
    a = (torch.rand(Ta, B, 1, generator=gen) < 0.4).float() * torch.rand(Ta, B, 1, generator=gen) * 2
    t = torch.arange(t0 - 1, t_end, 1.0)
    cot = torch.randn(t.numel(), B, D, generator=gen)
    # kernels
    ode.set_action_static(a.to(dev), None)
    yg = y0.to(dev).requires_grad_(True)
    h = hode.odeint(ode, yg, t.to(dev), method=method, options={"step_size": 1.0 / div, "perturb": perturb})
    (h * cot.to(dev)).sum().backward()
    got = [yg.grad] + [p.grad for p in ode.ml_net.parameters()]
    # eager restatement on the CPU
    ps = [p.detach().cpu().clone().requires_grad_(True) for p in ode.ml_net.parameters()]
    yc = y0.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hc, _ = neural_real_eager.solve(kind, yc, *ps, a, t, method, step_size=1.0 / div, perturb=perturb)
    (hc * cot).sum().backward()
    want = [yc.grad] + [p.grad for p in ps]
    return h.detach().cpu(), hc.detach(), got, want


@pytest.mark.parametrize("kind,D,method,H,B,perturb,div", _cases())
def test_kernels_vs_eager(kind, D, method, H, B, perturb, div):
    h, hc, got, want = _run(kind, D, method, H, B, perturb, div, _dev())
    assert h.shape == hc.shape
    err = (h - hc).abs().max().item()
    assert err <= 2e-5 * (1 + hc.abs().max().item()), err
    for name, g, w in zip(("y0", "w1", "b1", "w2", "b2"), got, want):
        assert _rel(g, w) < 2e-4, (name, _rel(g, w))


def test_grid_from_minus_one_and_short_action():
    """t0 = 0 (grid starts at -1: stage rows by truncation) with an action shorter than the grid (zero-dose branch)."""
    dev = _dev()
    for kind, D in (("neural", 20), ("2nd", 40)):
        h, hc, got, want = _run(kind, D, "rk4", 43, 37, True, 1, dev, t0=0, t_end=12, Ta=5, seed=3)
        assert (h - hc).abs().max().item() <= 2e-5 * (1 + hc.abs().max().item())
        for g, w in zip(got, want):
            assert _rel(g, w) < 2e-4


def _g10_decoder(g, ci, dev):
    import model
    pre = "c%d_" % ci
    D, H, div, t0, TA, TMAX, B, obs, seed = (int(v) for v in g[pre + "meta"])
    dec = model.DecoderReal(obs, D, ACT, STAT, H, TMAX, 1, t0=t0, method=str(g[pre + "method"]), ode_step_size=1.0 / div,
                            ode_type=str(g[pre + "kind"]), device=dev)
    dec.load_state_dict({k: torch.from_numpy(g[pre + "sd_" + k.replace(".", "__")]) for k in dec.state_dict()})
    return dec, pre


def test_golden_g10_on_the_gpu(golden_dir):
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g10_neural_real.npz"), allow_pickle=False)
    for ci in range(int(g["n_cases"])):
        dec, pre = _g10_decoder(g, ci, dev)
        assert list(dec.state_dict()) == [str(k) for k in g[pre + "sd_keys"]]
        assert dec.model_name == str(g[pre + "model_name"])
        init = torch.from_numpy(g[pre + "init"]).to(dev).requires_grad_(True)
        x_hat, h = dec(init, torch.from_numpy(g[pre + "a"]).to(dev), torch.from_numpy(g[pre + "s"]).to(dev))
        (x_hat * torch.from_numpy(g[pre + "cot"]).to(dev)).sum().backward()
        ref_h = torch.from_numpy(g[pre + "h"])
        assert (h.detach().cpu() - ref_h).abs().max().item() <= 2e-5 * (1 + ref_h.abs().max().item()), ci
        ref_x = torch.from_numpy(g[pre + "x_hat"])
        assert (x_hat.detach().cpu() - ref_x).abs().max().item() <= 1e-4 * (1 + ref_x.abs().max().item()), ci
        assert _rel(init.grad, torch.from_numpy(g[pre + "g_init"])) < 2e-4, ci
        for n, p in dec.named_parameters():
            assert _rel(p.grad, torch.from_numpy(g[pre + "g_" + n.replace(".", "__")])) < 2e-4, (ci, n)


@pytest.mark.parametrize("kind,D,method", [("neural", 20, "midpoint"), ("2nd", 40, "rk4")])
def test_backward_is_bitwise_reproducible(kind, D, method):
    import model
    dev = _dev()
    gen = torch.Generator().manual_seed(4)
    torch.manual_seed(4)
    dec = model.DecoderReal(OBS, D, ACT, STAT, HIDDEN, 40, 1, t0=24, method=method, ode_step_size=1.0, ode_type=kind, device=dev)
    init = (torch.randn(1000, D, generator=gen) * 0.5).to(dev)
    a = ((torch.rand(40, 1000, 1, generator=gen) < 0.3).float() * torch.rand(40, 1000, 1, generator=gen)).to(dev)
    cot = torch.randn(16, 1000, OBS, generator=gen).to(dev)
    grads = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        ig = init.clone().requires_grad_(True)
        x_hat, _ = dec(ig, a, None)
        (x_hat * cot).sum().backward()
        grads.append([ig.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    for g0, g1 in zip(*grads):
        assert torch.equal(g0, g1)


def _vi(kind, D, method, dev, B=100, T=48, t0=24, seed=5):
    import model
    gen = torch.Generator().manual_seed(seed)
    input_dim = OBS + ACT + STAT + 1
    torch.manual_seed(seed)
    enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=dev)
    dec = model.DecoderReal(OBS, D, ACT, STAT, HIDDEN, T, 1, t0=t0, method=method, ode_step_size=1.0, ode_type=kind, device=dev)
    data = {"measurements": torch.randn(T, B, OBS, generator=gen).to(dev),
            "actions": ((torch.rand(T, B, ACT, generator=gen) < 0.15).float() * torch.rand(T, B, ACT, generator=gen)).to(dev),
            "masks": (torch.rand(T, B, OBS, generator=gen) < 0.5).float().to(dev),
            "statics": torch.rand(1, B, STAT, generator=gen).expand(T, B, STAT).contiguous().to(dev)}
    return enc, dec, data


@pytest.mark.parametrize("weight", [False, True])
def test_fused_and_unfused_vi_loss_agree(weight):
    import model
    dev = _dev()
    enc, dec, data = _vi("neural", 20, "midpoint", dev)
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
    _, dec40, data40 = _vi("2nd", 40, "rk4", dev)
    assert not dec40.fused_likelihood_ok(data40["measurements"])  # D = 40: the unfused loss


def test_golden_vi_loss_on_the_gpu(golden_dir):
    import model
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g10_neural_real.npz"), allow_pickle=False)
    for vi_i in range(2):
        pre = "vi%d_" % vi_i
        D, t0, B, T, obs, seed, hidden = (int(v) for v in g[pre + "meta"])
        input_dim = obs + ACT + STAT + 1
        enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=dev)
        dec = model.DecoderReal(obs, D, ACT, STAT, hidden, T, 1, t0=t0, method=str(g[pre + "method"]), ode_step_size=1.0,
                                ode_type=str(g[pre + "kind"]), device=dev)
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
                    assert _rel(got, ref_g) < 2e-4, (vi_i, n)


@pytest.mark.parametrize("kind,D,method", [("neural", 20, "midpoint"), ("2nd", 40, "rk4")])
def test_full_size_vi_loss_vs_cpu_pipeline(kind, D, method):
    """run_real's full size: 8 192 patients, t_max 120, t0 24.  The same VariationalInferenceReal on the CPU with the
    decoder's rhs stepped eagerly (the mirror's `forward` / `dose_at_time` through oracle.solvers.odeint)."""
    import model
    from oracle.solvers import odeint as oracle_odeint
    dev = _dev()
    enc, dec, data = _vi(kind, D, method, dev, B=8192, T=120, t0=24, seed=9)
    vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=24, weight=False)
    cenc, cdec = copy.deepcopy(enc).to("cpu"), copy.deepcopy(dec).to("cpu")
    cenc.device = cdec.device = cdec.ode.device = torch.device("cpu")
    cdec.t = dec.t.cpu()
    cdec.options = dict(dec.options, step_t=cdec.t)
    cdec._odeint = oracle_odeint
    cvi = model.VariationalInferenceReal(cenc, cdec, elbo=False, t0=24, weight=False)
    loss = vi.loss(data)
    loss.backward()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        closs = cvi.loss({k: v.cpu() for k, v in data.items()})
    closs.backward()
    assert abs(loss.item() - closs.item()) <= 1e-4 * abs(closs.item())
    # `neural`: every gradient at the kernels' tolerance.  `2nd`: y2 integrates y1 over 96 steps, the readout error and with
    # it every cotangent reach 1e6 .. 1e7 at this size, and the sums over 8 192 patients x 96 steps x 4 stages differ in
    # fp32 summation order between the two pipelines (CPU vs GPU, on both sides) by a few 1e-4: 1e-3 there.  The encoder
    # (hode_lstm kernels vs nn.LSTM on the CPU) sums the same large cotangents: 1e-3 for both kinds.
    dtol = 2e-4 if kind == "neural" else 1e-3
    for mods, cmods, tol in (((dec,), (cdec,), dtol), ((enc,), (cenc,), 1e-3)):
        for (n, p), (_, q) in zip(mods[0].named_parameters(), cmods[0].named_parameters()):
            if q.grad is None or q.grad.abs().max() == 0:
                assert p.grad is None or p.grad.abs().max() == 0, n
            else:
                assert _rel(p.grad, q.grad) < tol, (n, _rel(p.grad, q.grad))


@pytest.mark.parametrize("kind,D,method", [("neural", 20, "midpoint"), ("2nd", 40, "rk4")])
def test_training_loop_and_evaluate_at_run_real_shapes(kind, D, method, tmp_path, golden_dir):
    """run_real.py's construction (obs 24, statics 11, batch 100, t0 24, device from get_device()): two iterations of the
    mirrored training loop on DeviceFolds, a finite loss, a checkpoint with the reference's decoder keys; evaluate(real=True)
    runs."""
    import model
    import training_utils
    from hode.batches import DeviceFolds
    dev = _dev()
    g = np.load(os.path.join(golden_dir, "g10_neural_real.npz"), allow_pickle=False)
    obs_dim, action_dim, static_dim, t_max, step_size, t0 = OBS, ACT, STAT, 48, 1, 24
    hidden_dim = int((obs_dim + action_dim + static_dim) * 1.2)
    input_dim = obs_dim + action_dim + static_dim + 1
    N = 400
    gen = torch.Generator().manual_seed(11)
    folds = DeviceFolds(torch.randn(t_max, N, obs_dim, generator=gen),
                        (torch.rand(t_max, N, 1, generator=gen) < 0.15).float() * torch.rand(t_max, N, 1, generator=gen),
                        torch.zeros(t_max, N, 4), (torch.rand(t_max, N, obs_dim, generator=gen) < 0.5).float(), 100, 100,
                        statics=torch.rand(1, N, static_dim, generator=gen).expand(t_max, N, static_dim), device=dev)
    torch.manual_seed(0)
    encoder = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False)
    decoder = model.DecoderReal(obs_dim, D, action_dim, static_dim, hidden_dim, t_max, step_size, t0=t0, method=method,
                                ode_step_size=step_size / 1, ode_type=kind)
    vi = model.VariationalInferenceReal(encoder, decoder, elbo=False, t0=t0)
    opt = torch.optim.Adam(vi.parameters(), lr=1e-3)
    vi, best, _ = training_utils.variational_training_loop(2, folds, vi, 100, opt, 1, path=str(tmp_path) + "/")
    assert np.isfinite(best) and best < 1e9
    ck = torch.load(str(tmp_path) + "/" + vi.model_name, map_location="cpu")
    kinds = [str(g["c%d_kind" % i]) for i in range(int(g["n_cases"]))]
    pre = "c%d_" % kinds.index(kind)
    assert list(ck["decoder_state_dict"].keys()) == [str(k) for k in g[pre + "sd_keys"]]
    eval_dec = model.DecoderReal(obs_dim, D, action_dim, static_dim, hidden_dim, t_max, step_size, t0=0, method=method,
                                 ode_step_size=step_size / 1, ode_type=kind)
    eval_dec.load_state_dict(decoder.state_dict())
    out = training_utils.evaluate(model.VariationalInferenceReal(encoder, eval_dec, elbo=False, t0=t0), folds, 50, t0,
                                  mc_itr=3, real=True)
    assert len(out) == 6 and np.isfinite(out[3])
