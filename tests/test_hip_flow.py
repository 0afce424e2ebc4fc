"""The planar-flow posterior on the device (libhode_flow.so: hode_flow_fwd / hode_flow_bwd) against the float64
restatement (tests/flow_eager.py) over the D x K x S x B table, the gradient-input modes, the numerically special
branches, bit-identical repeats, the reference's numbers (G11), the fused loss against the CPU mirror, evaluate_flow
against an eager per-draw loop, and a short training run at the run_noise_level shape."""
import os

import numpy as np
import pytest
import torch

import flow_eager as fe
import model
from reference_checks import FLOW_GTOL as GTOL, FLOW_TOL as TOL, close as _close
from oracle.solvers import odeint as oracle_odeint

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OBS, ACT, HIDDEN = 20, 1, 40
STEP = 0.125  # the model-level comparisons integrate on a grid where rk4 stays finite


def _inputs(D, K, S, B, seed, scale_u=0.5):
    g = torch.Generator().manual_seed(seed)
    mu = 0.3 * torch.randn(B, D, generator=g)
    lv = -1.0 + 0.3 * torch.randn(B, D, generator=g)
    u = scale_u * torch.randn(B, K, D, generator=g)
    w = torch.randn(B, K, D, generator=g)
    w = w / w.norm(dim=-1, keepdim=True) * (0.5 + 0.5 * torch.rand(B, K, 1, generator=g))  # |w| in [0.5, 1]: bounded u_hat
    b = 0.3 * torch.randn(B, K, generator=g)
    noise = torch.randn(S, B, D, generator=g)
    gz = torch.randn(S, B, D, generator=g)
    gkl = torch.randn(B, generator=g)
    return mu, lv, u, w, b, noise, gz, gkl


def _device_run(mu, lv, u, w, b, noise, s_kl, gz=None, gkl=None):
    from hode.flow import planar_flow_sample
    ins = [t.to(DEV).requires_grad_(True) for t in (mu, lv, u, w, b)]
    z_out, kl = planar_flow_sample(*ins, noise.to(DEV), s_kl)
    obj = 0.0
    if gz is not None:
        obj = obj + (z_out * gz.to(DEV)).sum()
    if gkl is not None:
        obj = obj + (kl * gkl.to(DEV)).sum()
    grads = torch.autograd.grad(obj, ins, allow_unused=True) if torch.is_tensor(obj) else (None,) * 5
    grads = [torch.zeros_like(x) if gr is None else gr for gr, x in zip(grads, ins)]
    torch.cuda.synchronize()
    return z_out.detach().cpu(), kl.detach().cpu(), [gr.cpu() for gr in grads]


def _check(mu, lv, u, w, b, noise, s_kl, gz, gkl, tol=TOL, gtol=GTOL, idx=None):
    z, kl, grads = _device_run(mu, lv, u, w, b, noise, s_kl, gz, gkl)
    if idx is not None:  # large B: the fp64 yardstick on a subset of patients (each patient's sums are its own)
        mu, lv, u, w, b = (t[idx] for t in (mu, lv, u, w, b))
        noise, z = noise[:, idx], z[:, idx]
        gz = None if gz is None else gz[:, idx]
        gkl = None if gkl is None else gkl[idx]
        kl, grads = kl[idx], [gr[idx] for gr in grads]
    rz, rkl, rgrads = fe.forward_backward(mu, lv, u, w, b, noise.double(), s_kl, gz, gkl)
    _close(z, rz, tol, "z_out")
    _close(kl, rkl, tol, "kl")
    for n, gr, rg in zip(("mu", "log_var", "u", "w", "b"), grads, rgrads):
        _close(gr, rg, gtol, "grad_" + n)


def _subset(B):
    if B < 10000:
        return None
    g = torch.Generator().manual_seed(B)
    return torch.cat([torch.arange(64), torch.randint(0, B, (64,), generator=g), torch.arange(B - 64, B)])


@pytest.mark.parametrize("case", fe.CASES, ids=lambda c: "D%d_K%d_S%d_B%d_skl%d" % c)
def test_kernel_against_fp64(case):
    D, K, S, B, s_kl = case
    mu, lv, u, w, b, noise, gz, gkl = _inputs(D, K, S, B, seed=D * 1000 + K * 10 + S + B)
    _check(mu, lv, u, w, b, noise, s_kl, gz, gkl, idx=_subset(B))


@pytest.mark.parametrize("s_kl", [0, 1])
@pytest.mark.parametrize("mode", ["grad_z", "grad_kl", "both"])
def test_gradient_input_modes(s_kl, mode):
    mu, lv, u, w, b, noise, gz, gkl = _inputs(6, 4, 51, 10, seed=7)
    _check(mu, lv, u, w, b, noise, s_kl, gz if mode != "grad_kl" else None, gkl if mode != "grad_z" else None)


def test_softplus_threshold_branch():
    mu, lv, u, w, b, noise, gz, gkl = _inputs(6, 4, 50, 7, seed=11)
    w = w / w.norm(dim=-1, keepdim=True)
    u = 25.0 * w + 0.01 * u    # uw ~ 25 > 20: softplus(x) = x
    u[:, 1] = 19.0 * w[:, 1]    # and one flow just below the threshold
    _check(mu, lv, u, w, b, noise, 1, gz, gkl, tol=5e-4, gtol=5e-3)


def test_saturated_tanh():
    mu, lv, u, w, b, noise, gz, gkl = _inputs(6, 4, 50, 7, seed=12)
    b = b + 40.0 * torch.sign(b)   # |w . z + b| ~ 40: tanh = +-1, 1 - tanh^2 = 0
    _check(mu, lv, u, w, b, noise, 1, gz, gkl)


def test_near_zero_jacobian_term():
    D, K, S, B = 6, 1, 50, 7
    mu, lv, u, w, b, noise, gz, gkl = _inputs(D, K, S, B, seed=13)
    mu = torch.zeros(B, D)
    lv = torch.full((B, D), -12.0)    # z0 ~ 0 so that tanh(w . z + b) ~ 0
    b = torch.zeros(B, K)
    w = w / w.norm(dim=-1, keepdim=True)
    u = -5.0 * w                      # m(uw) = -1 + softplus(-5): 1 + psi . u_hat ~ 6.7e-3
    _check(mu, lv, u, w, b, noise, 1, gz, gkl, tol=1e-3, gtol=1e-2)


def test_bit_identical_repeats():
    for D, K, S, B in ((6, 4, 51, 10), (12, 4, 50, 10000)):
        args = _inputs(D, K, S, B, seed=21)
        r1 = _device_run(*args[:6], 1, args[6], args[7])
        r2 = _device_run(*args[:6], 1, args[6], args[7])
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
        for a, b in zip(r1[2], r2[2]):
            assert torch.equal(a, b)


def test_domain_refused_on_device():
    from hode import HodeConfigError
    from hode.flow import planar_flow_sample
    mu, lv, u, w, b, noise, _, _ = (t.to(DEV) for t in _inputs(6, 4, 51, 10, seed=1))
    with pytest.raises(HodeConfigError):
        planar_flow_sample(mu, lv, u, w, b, torch.randn(257, 10, 6, device=DEV))
    with pytest.raises(HodeConfigError):
        planar_flow_sample(torch.zeros(10, 33, device=DEV), torch.zeros(10, 33, device=DEV), torch.zeros(10, 4, 33, device=DEV),
                           torch.zeros(10, 4, 33, device=DEV), b, torch.randn(5, 10, 33, device=DEV))
    with pytest.raises(HodeConfigError):
        planar_flow_sample(mu, lv, u, w, b, noise[:1], s_kl=1)


# ---------------------------------------------------------------------------------------------------------- G11
@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_flow.npz"))


def _sd(g, pre):
    return {k[len(pre):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def test_g11_encoder_and_flow_on_device(g11):
    from hode.flow import planar_flow_sample
    for ci in range(int(g11["n_cases"])):
        pre = "c%d_" % ci
        D, K, B, normalize, _, _ = (int(v) for v in g11[pre + "meta"])
        enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, D, K, normalize=bool(normalize), device=DEV)
        enc.load_state_dict(_sd(g11, pre + "enc_"))
        x, a, m = (torch.from_numpy(g11[pre + k]).to(DEV) for k in ("x", "a", "mask"))
        with torch.no_grad():
            eo = enc(x, a, m)
            for n, t in zip(("mu", "log_var", "u", "w", "b"), eo):
                np.testing.assert_allclose(t.cpu().numpy(), g11[pre + n], rtol=1e-4, atol=1e-5, err_msg=n)
            eo_ref = [torch.from_numpy(g11[pre + n]).to(DEV) for n in ("mu", "log_var", "u", "w", "b")]
            z, kl = planar_flow_sample(*eo_ref, torch.from_numpy(g11[pre + "rep_eps"]).to(DEV).unsqueeze(0), s_kl=0)
        np.testing.assert_allclose(z[0].cpu().numpy(), g11[pre + "rep_z"], rtol=1e-4, atol=1e-7)
        z_ref = torch.from_numpy(g11[pre + "rep_z"]).double()
        kl_ref = torch.from_numpy(g11[pre + "rep_log_density"]).double() - model.ExponentialPrior.log_density(z_ref)
        np.testing.assert_allclose(kl.cpu().numpy(), kl_ref.numpy(), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("mc", [1, 50])
def test_g11_loss_on_device(g11, mc):
    lp = "c0_m%d_" % mc
    enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=False, device=DEV)
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 8.0, 1.0, roche=True, method="rk4", device=DEV)
    enc.load_state_dict(_sd(g11, lp + "enc_"))
    dec.load_state_dict(_sd(g11, lp + "dec_"))
    vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=mc)
    noise = torch.from_numpy(g11[lp + "noise"]).to(DEV)
    vi.noise = lambda n, like: noise[:n].clone()
    data = {k2: torch.from_numpy(g11[lp + k]).to(DEV) for k, k2 in (("x", "measurements"), ("a", "actions"), ("mask", "masks"))}
    loss = vi.loss(data)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g11[lp + "loss"]), rtol=1e-3)
    for prefix, mod in (("genc_", enc), ("gdec_", dec)):
        for n, p in mod.named_parameters():
            ref = g11[lp + prefix + n.replace(".", "__")]
            got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
            fin = np.isfinite(ref)  # the reference's own Hill-exponent gradients are NaN on this grid: not compared
            assert np.isfinite(got[fin]).all(), prefix + n
            if fin.any():
                assert np.abs(got[fin] - ref[fin]).max() <= 1e-2 * (np.abs(ref[fin]).max() + 1e-6), prefix + n


# ---------------------------------------------------------------------------------------- model-level paths
def _vi_pair(mc, seed=5):
    torch.manual_seed(seed)
    enc = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=False, device=DEV)
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 14 * STEP, STEP, roche=True, method="rk4", device=DEV)
    enc_c = model.EncoderPlanarLSTM(OBS + ACT, HIDDEN, 6, 4, normalize=False, device=torch.device("cpu"))
    dec_c = model.RocheExpertDecoder(OBS, 6, ACT, 14 * STEP, STEP, roche=True, method="rk4", device=torch.device("cpu"))
    dec_c._odeint = oracle_odeint
    enc_c.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    dec_c.load_state_dict({k: v.cpu() for k, v in dec.state_dict().items()})
    prior = model.ExponentialPrior.log_density
    return (model.VariationalInferenceFlow(enc, dec, prior_log_pdf=prior, mc_size=mc),
            model.VariationalInferenceFlow(enc_c, dec_c, prior_log_pdf=prior, mc_size=mc))


@pytest.mark.parametrize("mc", [1, 50])
def test_loss_and_backward_against_cpu_mirror(mc):
    vi, vi_c = _vi_pair(mc)
    B, T = 10, 15
    g = torch.Generator().manual_seed(3)
    x = 0.5 * torch.randn(T, B, OBS, generator=g)
    a = torch.zeros(T, B, 1)
    a[torch.randint(0, T - 1, (B,), generator=g), torch.arange(B), 0] = torch.rand(B, generator=g) * 10
    m = (torch.rand(T, B, OBS, generator=g) < 0.5).float()
    noise = 0.5 * torch.randn(1 if mc == 1 else 1 + mc, B, 6, generator=g)
    vi.noise = lambda n, like: noise[:n].to(DEV)
    vi_c.noise = lambda n, like: noise[:n].clone()
    loss = vi.loss({"measurements": x.to(DEV), "actions": a.to(DEV), "masks": m.to(DEV)})
    loss.backward()
    loss_c = vi_c.loss({"measurements": x, "actions": a, "masks": m})
    loss_c.backward()
    np.testing.assert_allclose(loss.item(), loss_c.item(), rtol=1e-3)
    for (n, p), (_, pc) in zip(list(vi.encoder.named_parameters()) + list(vi.decoder.named_parameters()),
                               list(vi_c.encoder.named_parameters()) + list(vi_c.decoder.named_parameters())):
        got = p.grad.cpu() if p.grad is not None else torch.zeros_like(pc)
        ref = pc.grad if pc.grad is not None else torch.zeros_like(pc)
        assert torch.isfinite(ref).all(), n
        assert (got - ref).abs().max().item() <= 1e-2 * (ref.abs().max().item() + 1e-6), n


def test_evaluate_flow_against_eager_per_draw_loop(capsys):
    import training_utils
    from hode.batches import DeviceFolds
    from oracle.evalmetrics import crps_ensemble
    vi, _ = _vi_pair(50, seed=9)
    folds = DeviceFolds.synthetic(60, 15, OBS, 6, 10, 20, DEV, seed=4, step=STEP)
    M, bs, t0 = 8, 10, 5
    n_chunks = folds.test_size // bs
    noises = [torch.randn(1 + M, bs, 6, device=DEV) for _ in range(n_chunks)]
    it = iter(noises)
    vi.noise = lambda n, like: next(it)
    got = training_utils.evaluate_flow(vi, folds, bs, t0, mc_itr=M)
    out = capsys.readouterr().out.splitlines()
    assert [line.split(",")[0] for line in out[-4:]] == ["rmse_z0", "rmse_x", "cprs_z0", "cprs_x"]

    # the reference's loop, one reparameterize call per draw (eps injected in the same order)
    se_z0, mse_x, c_z0, c_x = [], [], [], []
    E = folds.expert_dim
    with torch.no_grad():
        for chunk in range(n_chunks):
            data = folds.get_split("test", bs, chunk)
            eo = vi.encoder(data["measurements"][:t0], data["actions"][:t0], data["masks"][:t0])
            draws = list(noises[chunk])
            orig = torch.randn_like
            torch.randn_like = lambda *a, **k: draws.pop(0).clone()
            try:
                mu, lv, z0_hat, ldj, z0 = vi.encoder.reparameterize(*eo)
                x_hat, _ = vi.decoder(z0_hat, data["actions"])
                zs, xs = [], []
                for _ in range(M):
                    mu, lv, z_, ldj, z0_last = vi.encoder.reparameterize(*eo)
                    zs.append(z_)
                    xs.append(vi.decoder(z_, data["actions"])[0])
            finally:
                torch.randn_like = orig
            x_hat = x_hat[t0:]
            x_test, mask_test = data["measurements"][t0:], data["masks"][t0:]
            se_z0.append(torch.sum((z0[:, :E] - z0_hat[:, :E]) ** 2, dim=1).cpu())
            mse_x.append((torch.sum((x_test - x_hat) ** 2 * mask_test, dim=(0, 2)) / torch.sum(mask_test, dim=(0, 2))).cpu())
            z_mat = torch.stack(zs, -1).cpu().numpy()
            zt = z0_last.cpu().numpy()
            c_z0.append(np.mean([[crps_ensemble(zt[i, d], z_mat[i, d]) for d in range(E)] for i in range(bs)], axis=1))
            xm = torch.stack(xs, -1)[t0:].cpu().numpy()
            xt = x_test.cpu().numpy()
            cx = np.array([[[crps_ensemble(xt[t, i, o], xm[t, i, o]) for o in range(OBS)] for i in range(bs)]
                           for t in range(xt.shape[0])])
            c_x.append(cx.mean(axis=(0, 2)))
    mse = torch.cat(mse_x)
    ref = (torch.sqrt(torch.cat(se_z0).mean()).item(), np.mean(np.concatenate(c_z0)),
           torch.sqrt(mse[~torch.isnan(mse)].mean()).item(), np.mean(np.concatenate(c_x)))
    np.testing.assert_allclose([got[0], got[2], got[3], got[5]], ref, rtol=2e-3)


def test_training_at_run_noise_level_shape():
    """run_noise_level.sh's flow run: default DataConfig (obs 20, D 6, t_max 14, step 1), batch 10, dopri5, mc_size 50."""
    import sim_config
    from hode.batches import DeviceFolds
    dc = sim_config.DataConfig()
    T = int(dc.t_max / dc.step_size) + 1
    folds = DeviceFolds.synthetic(200, T, dc.obs_dim, dc.latent_dim, 20, 20, DEV, seed=2, step=float(dc.step_size))
    torch.manual_seed(0)
    enc = model.EncoderPlanarLSTM(dc.obs_dim + dc.action_dim, int(dc.obs_dim * 2.0), dc.latent_dim, 4, normalize=False,
                                  device=DEV)
    dec = model.RocheExpertDecoder(dc.obs_dim, dc.latent_dim, dc.action_dim, dc.t_max, dc.step_size, roche=True,
                                   method="dopri5", device=DEV)
    vi = model.VariationalInferenceFlow(enc, dec, prior_log_pdf=model.ExponentialPrior.log_density, mc_size=50)
    params = list(vi.encoder.parameters()) + list(vi.decoder.output_function.parameters()) + list(vi.decoder.ode.ml_net.parameters())
    opt = torch.optim.Adam(params, lr=0.01)
    losses = []
    for itr in range(40):
        data = folds.get_split("train", 10, itr % (folds.train_size // 10))
        opt.zero_grad()
        loss = vi.loss(data)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:5]), losses
