"""Every entry of tests/metric_cases.py through the C ABI (hode_ensemble_crps, hode_mc_kl_exponential) against float64.
GPU only.

CRPS: the fp64 sorted-form oracle (oracle.evalmetrics.crps_sorted) of the readout computed in fp64 from the exact fp32 h,
W and b.  Tolerance per element, no absolute floor: 2e-5 * (mean_m |x_m - y| + mean_m sum_d |W_od h_md| + |b_o|), the
readout terms dropped for the identity readout (so the offset case is held to its 1e-2 spread, not its 1e3 magnitude).

MC-KL: the literal fp64 autograd loop of tests/test_hip_mckl.py on the same noise.  Tolerance per element relative to
that element's own term magnitudes (mean_s of |log q_s| + |log p_s|, of |d/dmu| and of |d/dlog_var| per draw): 2e-5
(kl) or 1e-5 (gradients) plus S * 2^-24, the worst-case relative error of the kernel's S-term fp32 running sum.  The
bound, not a random-walk estimate, is the right one here: every clamped draw of an element adds the same constant, so
the rounding errors of its running sum share a sign and grow like S, not like sqrt(S)."""
import ctypes

import numpy as np
import pytest
import torch

import metric_cases as mc
from reference_checks import (CRPS_TOL, MCKL_GRAD_TOL, MCKL_KL_TOL, crps_oracle as _crps_oracle, mckl_scales as _mckl_scales,
                              mckl_sum_error, within as _within)
from test_hip_mckl import _reference  # the literal fp64 loop of the reference

pytestmark = pytest.mark.gpu



def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    import hode
    from hode import _lib as L
    return hode.lib(), L


# ------------------------------------------------------------------------------------------------------------- CRPS
def _crps_inputs(c, seed):
    """Logical fp32 tensors: h (Tn, M, B, Dv), truth (Tn, B, obs), w (obs, Dv) or None, b (obs,) or None."""
    g = torch.Generator().manual_seed(seed)
    Tn, B, M, Dv, obs = c["Tn"], c["B"], c["M"], c["Dv"], c["obs"]
    if c["values"] == "offset":
        h = 1000.0 + 0.01 * torch.randn(Tn, M, B, Dv, generator=g, dtype=torch.float64)
        truth = 1000.0 + 0.01 * torch.randn(Tn, B, obs, generator=g, dtype=torch.float64)
        h, truth = h.float(), truth.float()
    else:
        h = torch.randn(Tn, M, B, Dv, generator=g)
        truth = torch.randn(Tn, B, obs, generator=g) * 2.0
    w = b = None
    if c["readout"] != "identity":
        w = torch.randn(obs, Dv, generator=g) * 0.5
        if c["readout"] == "affine":
            b = torch.randn(obs, generator=g)
    if c["values"] in ("tied", "zero_spread"):
        h[:, 1:] = h[:, :1]
    if c["values"] == "truth_member":
        truth = h[:, c["M"] // 3, :, :obs].clone()
    if c["values"] == "zero_spread":
        truth = h[:, 0, :, :obs].clone()
    return h, truth, w, b


def _layout(c, h):
    """h laid out as the entry says: (flat fp32 storage, element offset of time 0, time / member / patient strides).
    Every element the kernel must not read is NaN."""
    Tn, M, B, Dv = h.shape
    t0 = 0
    if c["layout"] in ("member", "slice"):
        ms, ps = B * Dv, Dv
        ts = M * ms
        t0 = 2 if c["layout"] == "slice" else 0
    elif c["layout"] == "patient":
        ms, ps = Dv, M * Dv
        ts = B * ps
    else:  # padded: patient rows of Dv + 3, a 5-float gap between members and a 7-float gap between times
        ps = Dv + 3
        ms = B * ps + 5
        ts = M * ms + 7
    store = torch.full(((Tn + t0) * ts,), float("nan"))
    store.as_strided((Tn, M, B, Dv), (ts, ms, ps, 1), t0 * ts).copy_(h)
    return store, t0 * ts, (ts, ms, ps)


def _crps_call(lib, L, c, hdev, off, strides, truth_dev, w_dev, b_dev, out, batch=None, boff=0):
    """One hode_ensemble_crps call; out in ("crps", "sum", "both").  Returns (crps or None, crps_sum or None)."""
    B = c["B"] if batch is None else batch
    Tn, obs = c["Tn"], c["obs"]
    d = L.CrpsDesc()
    d.struct_size = ctypes.sizeof(L.CrpsDesc)
    d.n_times, d.batch, d.n_members, d.latent_dim, d.obs_dim = Tn, B, c["M"], c["Dv"], obs
    d.time_stride, d.member_stride, d.patient_stride = strides
    d.h = hdev.data_ptr() + 4 * (off + boff * strides[2])
    d.truth = truth_dev.data_ptr()
    d.w = 0 if w_dev is None else w_dev.data_ptr()
    d.b = 0 if b_dev is None else b_dev.data_ptr()
    full = torch.full((Tn, B, obs), float("nan"), device=hdev.device) if out in ("crps", "both") else None
    summed = torch.full((Tn, B), float("nan"), device=hdev.device) if out in ("sum", "both") else None
    d.crps = 0 if full is None else full.data_ptr()
    d.crps_sum = 0 if summed is None else summed.data_ptr()
    L.check(lib.hode_ensemble_crps(d, torch.cuda.current_stream().cuda_stream), "hode_ensemble_crps")
    torch.cuda.synchronize()
    return (None if full is None else full.cpu()), (None if summed is None else summed.cpu())


def _same_bits(a, b):
    assert a.shape == b.shape
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("c", mc.CRPS_CASES, ids=mc.crps_id)
def test_crps_case(c):
    dev = _dev()
    lib, L = _lib()
    h, truth, w, b = _crps_inputs(c, seed=mc.CRPS_CASES.index(c) + 1)
    ref, scale = _crps_oracle(h, truth, w, b)
    tol = CRPS_TOL * scale
    store, off, strides = _layout(c, h)
    hdev, tdev = store.to(dev), truth.to(dev)
    wdev = None if w is None else w.to(dev)
    bdev = None if b is None else b.to(dev)
    call = lambda out, **kw: _crps_call(lib, L, c, hdev, off, strides, tdev, wdev, bdev, out, **kw)
    full, summed = call(c["out"])

    if full is not None:
        err = (full.double() - ref).abs()
        worst = int(torch.argmax(err - tol))
        assert bool((err <= tol).all()), "worst element %d: got %r want %r tol %r" % (
            worst, float(full.flatten()[worst]), float(ref.flatten()[worst]), float(tol.flatten()[worst]))
        assert bool((full.double() >= -tol).all())
        if c["values"] == "zero_spread":
            assert bool((full == 0).all())
        if c["values"] == "tied":
            x = (h[:, 0, :, :c["obs"]].double() if w is None else
                 h[:, 0].double() @ w.double().t() + (0.0 if b is None else b.double()))
            assert bool(((full.double() - (x - truth.double()).abs()).abs() <= tol).all())
    if summed is not None:
        err = (summed.double() - ref.sum(-1)).abs()
        assert bool((err <= CRPS_TOL * scale.sum(-1)).all()), float((err / (scale.sum(-1))).max())
        if c["values"] == "zero_spread":
            assert bool((summed == 0).all())

    # deterministic: the same call again gives the same bits
    full2, summed2 = call(c["out"])
    for a, a2 in ((full, full2), (summed, summed2)):
        if a is not None:
            _same_bits(a, a2)
    # one call writing both outputs = the two single-output calls, bit for bit
    if c["out"] == "both":
        _same_bits(call("crps")[0], full)
        _same_bits(call("sum")[1], summed)
    # a sub-batch through `batch` and the h pointer (truth and outputs are dense, so a contiguous slice of it)
    if c["B"] >= 3:
        b0, nb = 1, c["B"] - 2
        tsub = truth[:, b0:b0 + nb].contiguous().to(dev)
        sf, ss = _crps_call(lib, L, c, hdev, off, strides, tsub, wdev, bdev, c["out"], batch=nb, boff=b0)
        if full is not None:
            _same_bits(sf, full[:, b0:b0 + nb])
        if summed is not None:
            _same_bits(ss, summed[:, b0:b0 + nb])


@pytest.mark.parametrize("M,Dv", mc.CRPS_REFUSED)
def test_crps_refuses_shapes_past_the_lds_bound(M, Dv):
    """(96, 128), (128, 96), (128, 128) with a readout need more than 160 KiB of LDS: refused before any launch.  The
    buffers are real and of the full size, so a wrong check could not touch foreign memory."""
    dev = _dev()
    import hode
    lib, L = _lib()
    assert not mc.crps_accepts(M, Dv, 8, "affine")
    Tn, B, obs = 2, 3, 8
    c = mc._crps(Tn, B, M, Dv, obs, "affine", "both", "member")
    h = torch.zeros(Tn, M, B, Dv)
    w, b = torch.zeros(obs, Dv, device=dev), torch.zeros(obs, device=dev)
    with pytest.raises(hode.HodeConfigError, match="LDS"):
        _crps_call(lib, L, c, h.reshape(-1).to(dev), 0, (M * B * Dv, B * Dv, Dv), torch.zeros(Tn, B, obs, device=dev),
                   w, b, "both")
    # the identity readout at the same (M, Dv) holds no readout in LDS and is accepted
    assert mc.crps_accepts(M, Dv, 8, "identity")


# ------------------------------------------------------------------------------------------------------------ MC-KL
def _mckl_inputs(c, seed):
    """mu, log_var (rows,), noise (S, rows) in fp32 for the entry's regime; no draw within 1e-5 (relative) of z = 0
    except the exact zeros of the 'zero' regime, so that fp32 and fp64 take the same branch."""
    g = torch.Generator().manual_seed(seed)
    rows, S = c["rows"], c["S"]
    lo, hi = c["lv"]
    lv = (lo + (hi - lo) * torch.rand(rows, generator=g, dtype=torch.float64)).float()
    sd = torch.exp(0.5 * lv.double())
    noise = torch.randn(S, rows, generator=g)
    if c["mu"] == "positive":
        mu = (10.0 * sd).float()
    elif c["mu"] == "clamped":
        mu = (-10.0 * sd).float()
    else:
        mu = (sd * 0.5 * torch.randn(rows, generator=g, dtype=torch.float64)).float()
    zero = torch.zeros(rows, dtype=torch.bool)
    if c["mu"] == "zero":
        zero[::7] = True
        mu[zero], lv[zero] = 0.0, 0.0
        nz = torch.zeros(S, int(zero.sum()))
        nz[:, 1::2] = -0.0
        noise[:, zero] = nz
    for _ in range(8):
        z = noise.double() * torch.exp(0.5 * lv.double()) + mu.double()
        near = (z.abs() <= 1e-5 * (mu.double().abs() + (z - mu.double()).abs())) & ~zero
        if not bool(near.any()):
            break
        noise[near] *= 1.1
    else:
        raise AssertionError("draws near z = 0 persist")
    if c["mu"] == "zero":
        assert bool((noise[:, zero] == 0).all()) and bool(torch.signbit(noise[:, zero][:, 1::2]).all())
    return mu, lv, noise, zero


def _mckl_call(lib, L, mu, lv, noise, rate, clamp, grads):
    dev = mu.device
    rows = mu.numel()
    kl = torch.full((rows,), float("nan"), device=dev)
    gmu = torch.full((rows,), float("nan"), device=dev)
    glv = torch.full((rows,), float("nan"), device=dev)
    d = L.McKlDesc()
    d.struct_size = ctypes.sizeof(L.McKlDesc)
    d.n_samples, d.rows, d.rate, d.clamp_value = noise.shape[0], rows, rate, clamp
    d.mu, d.log_var, d.noise, d.kl = mu.data_ptr(), lv.data_ptr(), noise.data_ptr(), kl.data_ptr()
    d.grad_mu = gmu.data_ptr() if grads in ("both", "mu") else 0
    d.grad_log_var = glv.data_ptr() if grads in ("both", "lv") else 0
    L.check(lib.hode_mc_kl_exponential(d, torch.cuda.current_stream().cuda_stream), "hode_mc_kl_exponential")
    torch.cuda.synchronize()
    return kl.cpu(), gmu.cpu(), glv.cpu()


@pytest.mark.parametrize("c", mc.MCKL_CASES, ids=mc.mckl_id)
def test_mckl_case(c):
    dev = _dev()
    lib, L = _lib()
    rate, clamp = float(c["rate"]), float(np.float32(mc.CLAMPS[c["clamp"]]))
    mu, lv, noise, zero = _mckl_inputs(c, seed=mc.MCKL_CASES.index(c) + 101)
    ref, mu_r, lv_r = _reference(mu, lv, noise, rate, clamp)
    ref.sum().backward()  # elements are independent: the per-element derivatives
    s_kl, s_gmu, s_glv, pos = _mckl_scales(mu, lv, noise, rate, clamp)
    frac = float(pos.double().mean())
    want = {"positive": frac == 1.0, "clamped": frac == 0.0, "mix": 0.0 < frac < 1.0 or c["rows"] * c["S"] < 4,
            "zero": 0.0 < frac < 1.0 and not bool(pos[:, zero].any())}[c["mu"]]
    assert want, (c["mu"], frac)
    md, lvd, nd = mu.to(dev), lv.to(dev), noise.to(dev)
    kl, gmu, glv = _mckl_call(lib, L, md, lvd, nd, rate, clamp, c["grads"])
    acc = mckl_sum_error(c["S"])
    _within(kl, ref.detach(), s_kl, MCKL_KL_TOL + acc, "kl")
    if c["grads"] in ("both", "mu"):
        _within(gmu, mu_r.grad, s_gmu, MCKL_GRAD_TOL + acc, "grad_mu")
    else:
        assert bool(torch.isnan(gmu).all())  # no buffer passed: nothing written
    if c["grads"] in ("both", "lv"):
        _within(glv, lv_r.grad, s_glv, MCKL_GRAD_TOL + acc, "grad_log_var")
    else:
        assert bool(torch.isnan(glv).all())
    if c["mu"] == "zero":  # z = 0 exactly clamps: d/dmu = (clamp - 0) / 1, not rate
        if c["grads"] in ("both", "mu"):
            assert bool((gmu[zero].double() == torch.tensor(clamp, dtype=torch.float64)).all())
    # every grad mode: kl bit-identical, each gradient bit-identical to the both-gradients call
    runs = {g: _mckl_call(lib, L, md, lvd, nd, rate, clamp, g) for g in ("both", "mu", "lv", "none")}
    for g, (k2, gm2, gl2) in runs.items():
        _same_bits(k2, kl)
        if g in ("both", "mu"):
            _same_bits(gm2, runs["both"][1])
        if g in ("both", "lv"):
            _same_bits(gl2, runs["both"][2])


def test_mckl_wrapper_passes_gradient_buffers_only_when_asked(monkeypatch):
    """hode.mckl.mc_kl_exponential under torch.no_grad passes NULL gradient pointers (the forward-only path of every
    validation pass); with only one of mu / log_var requiring a gradient it asks for both, and the gradient it returns
    matches the fp64 loop."""
    dev = _dev()
    from hode import _lib as L
    from hode.mckl import mc_kl_exponential
    real = L.lib()
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def hode_mc_kl_exponential(self, d, stream):
            seen.append((bool(d.grad_mu), bool(d.grad_log_var)))
            return real.hode_mc_kl_exponential(d, stream)

    monkeypatch.setattr(L, "lib", lambda: Spy())
    c = mc._mckl(33 * 8, 17, 100.0, "eps", (-9.0, -7.0), "mix", "both")
    mu, lv, noise, _ = _mckl_inputs(c, seed=7)
    clamp = float(np.float32(mc.CLAMPS["eps"]))
    ref, mu_r, lv_r = _reference(mu, lv, noise, 100.0, clamp)
    wts = torch.randn(mu.numel(), generator=torch.Generator().manual_seed(8)).double()
    (ref * wts).sum().backward()
    s_kl, s_gmu, s_glv, _ = _mckl_scales(mu, lv, noise, 100.0, clamp)

    with torch.no_grad():
        out = mc_kl_exponential(mu.to(dev).requires_grad_(True), lv.to(dev), noise.to(dev), 100.0, clamp)
    assert seen[-1] == (False, False) and not out.requires_grad
    _within(out.cpu(), ref.detach(), s_kl, MCKL_KL_TOL + mckl_sum_error(17), "kl (no_grad)")

    for which in ("mu", "lv"):
        md = mu.to(dev).requires_grad_(which == "mu")
        lvd = lv.to(dev).requires_grad_(which == "lv")
        out = mc_kl_exponential(md, lvd, noise.to(dev), 100.0, clamp)
        assert seen[-1] == (True, True)
        (out * wts.float().to(dev)).sum().backward()
        _within(out.detach().cpu(), ref.detach(), s_kl, MCKL_KL_TOL + mckl_sum_error(17), "kl")
        if which == "mu":
            assert lvd.grad is None
            _within(md.grad.cpu(), mu_r.grad, s_gmu * wts.abs(), MCKL_GRAD_TOL + mckl_sum_error(17), "grad_mu")
        else:
            assert md.grad is None
            _within(lvd.grad.cpu(), lv_r.grad, s_glv * wts.abs(), MCKL_GRAD_TOL + mckl_sum_error(17), "grad_log_var")
