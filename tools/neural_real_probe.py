"""Real-data neural ODE baselines (model.NeuralODEReal / NeuralODEReal2nd, csrc/hode_neural_real_mf.hip) at run_real's
full size: one JSON line per kind (``neural`` D 20 midpoint, ``2nd`` D 40 rk4) with the kernel forward / backward time,
the decoder forward + backward, the reference-style eager loop on the same GPU (the mirror's eager ``forward`` /
``dose_at_time`` -- one int(t) host sync and a full cumsum per rhs call -- through oracle.solvers.odeint, autograd
backward), the run_real-shaped training step, the MFMA / HBM bounds and the parity against the eager loop.

    python tools/neural_real_probe.py [--batch 8192] [--t-max 120] [--t0 24]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))

import torch  # noqa: E402

import model  # noqa: E402
from hode import _lib as L  # noqa: E402
from hode import neural_real  # noqa: E402
from hode.solver import _stream  # noqa: E402
from oracle.solvers import odeint as oracle_odeint  # noqa: E402

OBS, ACT, STAT = 24, 1, 11
PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def timed(fn, reps, warm_s=0.06):
    """ms per call from HIP events, after about `warm_s` of warm-up calls (as bench.py does)."""
    end = time.perf_counter() + warm_s
    fn()
    torch.cuda.synchronize()
    while time.perf_counter() < end:
        fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def mfma_count(kind, D, H, B, T, method):
    """MFMAs the kernels issue (16x16x4 f32), forward and backward, from the tile counts of hode_neural_real_mf.hip."""
    if kind == "2nd":
        qt = (D // 2 + 15) // 16
        ST, IT, OT = 2 * qt, (16 * qt + D // 2 + 2 + 15) // 16, qt
    else:
        ST, IT, OT = (D + 15) // 16, (D + 2 + 15) // 16, (D + 15) // 16
    HT = (H + 15) // 16
    S = STAGES[method]
    rhs = 4 * HT * IT + 4 * OT * HT
    vjp = 4 * HT * OT + 4 * ST * HT + 4 * HT * IT + 4 * OT * HT  # VJP + the weight-gradient outer products
    waves, steps = (B + 15) // 16, T - 1
    fwd = waves * steps * S * rhs
    bwd = waves * steps * (S * rhs + (S - 1) * 4 * HT * IT + S * vjp)  # recompute, hidden recompute, adjoint
    return fwd, bwd


def eager_decoder(dec):
    """The same decoder stepped like the reference: the mirror's eager rhs through the oracle's torchdiffeq loop."""
    dec._odeint = oracle_odeint
    return dec


def probe(kind, D, method, B, t_max, t0, dev):
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    hidden_dim = int((OBS + ACT + STAT) * 1.2)
    dec = model.DecoderReal(OBS, D, ACT, STAT, hidden_dim, t_max, 1, t0=t0, method=method, ode_step_size=1.0, ode_type=kind,
                            device=dev)
    init = (torch.randn(B, D, generator=gen) * 0.5).to(dev)
    a = ((torch.rand(t_max, B, 1, generator=gen) < 0.15).float() * torch.rand(t_max, B, 1, generator=gen)).to(dev)
    s = torch.rand(t_max, B, STAT, generator=gen).to(dev)
    T = dec.t.numel()
    cot = torch.randn(T - 1, B, OBS, generator=gen).to(dev)
    params = list(dec.parameters())

    # ---- kernels alone, through the C ABI
    l0, l2 = dec.ode.ml_net[0], dec.ode.ml_net[2]
    w = [x.detach().contiguous() for x in (l0.weight, l0.bias, l2.weight, l2.bias)]
    rows = neural_real.stage_rows(dec.t, method, True, t_max)
    dose = neural_real.dose_table(a, neural_real.table_index(rows, t_max).reshape(-1).to(dev)).contiguous()
    h = torch.empty(T, B, D, device=dev)
    d = neural_real._desc(neural_real.KINDS[kind], init, dec.t, dose, w[0], w[1], w[2], w[3], h, method)
    gh = torch.randn(T, B, D, device=dev)
    gy0 = torch.empty_like(init)
    gw = [torch.zeros_like(x) for x in w]
    d.grad_h, d.grad_y0 = gh.data_ptr(), gy0.data_ptr()
    d.grad_w1, d.grad_b1, d.grad_w2, d.grad_b2 = (x.data_ptr() for x in gw)
    lib = L.lib()
    nws = lib.hode_workspace_bytes(d, L.WS_RK_BWD)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nws
    L.check(lib.hode_rk_fwd(d, _stream()), "fwd")
    k_fwd = timed(lambda: L.check(lib.hode_rk_fwd(d, _stream()), "fwd"), 50)
    k_bwd = timed(lambda: L.check(lib.hode_rk_bwd(d, _stream()), "bwd"), 50)

    # ---- decoder forward + backward (dose table gather, kernels, readout MLP, autograd glue)
    def dec_step(dd):
        for p in params:
            p.grad = None
        ig = init.clone().requires_grad_(True)
        x_hat, hh = dd(ig, a, s)
        (x_hat * cot).sum().backward()
        return ig, hh
    t_dec = timed(lambda: dec_step(dec), 20)
    ik, hk = dec_step(dec)
    gk = [ik.grad.clone()] + [p.grad.clone() for p in params]

    # ---- the reference-style eager loop on the same GPU (same module, the rhs stepped eagerly)
    edec = eager_decoder(dec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t_eager = timed(lambda: dec_step(edec), 2, warm_s=0.0)
        ie, he = dec_step(edec)
    ge = [ie.grad] + [p.grad for p in params]
    dec._odeint = __import__("hode").odeint
    out = {"kind": kind, "latent": D, "hidden": hidden_dim, "method": method, "batch": B, "t_max": t_max, "t0": t0,
           "steps": T - 1, "kernel_fwd_ms": round(k_fwd, 4), "kernel_bwd_ms": round(k_bwd, 4),
           "decoder_fwd_bwd_ms": round(t_dec, 4), "eager_loop_fwd_bwd_ms": round(t_eager, 2),
           "speedup_vs_eager_loop": round(t_eager / t_dec, 1),
           "parity_max_abs_h": float((hk - he).detach().abs().max()),
           "parity_max_rel_l2_grad": max(float((x - y).norm() / y.norm()) for x, y in zip(gk, ge))}

    # ---- run_real-shaped training step (encoder, decoder, loss, Adam)
    input_dim = OBS + ACT + STAT + 1
    enc = model.EncoderLSTMReal(input_dim, int(input_dim * 1.2), D, output_all=False, reverse=False, device=dev)
    vi = model.VariationalInferenceReal(enc, dec, elbo=False, t0=t0)
    opt = torch.optim.Adam(vi.parameters(), lr=1e-3)
    data = {"measurements": torch.randn(t_max, B, OBS, generator=gen).to(dev), "actions": a,
            "masks": (torch.rand(t_max, B, OBS, generator=gen) < 0.5).float().to(dev), "statics": s}

    def train_step():
        opt.zero_grad()
        vi.loss(data).backward()
        opt.step()
    out["training_step_ms"] = round(timed(train_step, 10), 4)
    out["fused_loss"] = bool(dec.fused_likelihood_ok(data["measurements"]))

    # ---- bounds
    f_fwd, f_bwd = (2 * 16 * 16 * 4 * n for n in mfma_count(kind, D, hidden_dim, B, T, method))
    row = T * B * D * 4
    S = STAGES[method]
    b_fwd = row + (T - 1) * S * B * 4
    b_bwd = 2 * row + (T - 1) * S * B * 4 + B * D * 4
    for tag, f, b, ms in (("fwd", f_fwd, b_fwd, k_fwd), ("bwd", f_bwd, b_bwd, k_bwd)):
        mf, hb = f / PEAK_F32_MFMA * 1e3, b / PEAK_HBM * 1e3
        out["%s_mfma_floor_ms" % tag] = round(mf, 4)
        out["%s_hbm_floor_ms" % tag] = round(hb, 4)
        out["%s_bound" % tag] = "mfma" if mf >= hb else "hbm"
        out["%s_fraction_of_floor" % tag] = round(max(mf, hb) / ms, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--t-max", type=int, default=120)
    ap.add_argument("--t0", type=int, default=24)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind, D, method in (("neural", 20, "midpoint"), ("2nd", 40, "rk4")):
        print(json.dumps(probe(kind, D, method, args.batch, args.t_max, args.t0, dev)), flush=True)


if __name__ == "__main__":
    main()
