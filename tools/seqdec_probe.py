"""Real-data recurrent baselines (model.DecoderRealBenchmark, csrc/hode_seqdec.hip) at run_real's full size: one JSON line
per kind with the kernel forward / backward time, the decoder forward + backward, the reference-style eager step loop
(and for tlstm one nn.LSTM call over the sequence) on the same GPU, the run_real-shaped training step, the MFMA / HBM
bounds and the parity against the eager loop.

    python tools/seqdec_probe.py [--batch 8192] [--t-max 120] [--t0 24] [--latent 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd"))

import torch  # noqa: E402

import model  # noqa: E402
from hode import _lib as L  # noqa: E402
from hode import seqdec  # noqa: E402
from hode.solver import _stream  # noqa: E402

OBS, ACT, STAT = 24, 1, 11
PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


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


def eager_latent(dec, init, a):
    """The reference's decoder loop (model.py:942-962): one host sync per step, then the cell."""
    hidden, c = init[None], init[None]
    outs = []
    for tt in dec.t:
        t = int(tt.item())
        obs = a[t:t + 1]
        obs = torch.cat([obs, torch.ones_like(obs) * t / dec.t_max], dim=-1)
        out, (hidden, c) = dec.rnn(obs, (hidden, c))
        outs.append(out)
    return torch.cat(outs, dim=0)


def mfma_count(kind, D, B, T):
    HT, KT = (D + 15) // 16, (D + 3 + 15) // 16
    waves = (B + 15) // 16
    if kind == "tlstm":
        fwd = 4 * HT * KT * 4
        bwd = fwd + HT * 4 * HT * 4 + 4 * HT * KT * 4
    else:
        fwd = KT * KT * 4 + HT * KT * 4
        bwd = fwd + KT * HT * 4 + HT * KT * 4 + KT * KT * 4 + HT * KT * 4
    return waves * T * fwd, waves * T * bwd


def probe(kind, B, t_max, t0, D, dev):
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    hidden_dim = int((OBS + ACT + STAT) * 1.2)
    dec = model.DecoderRealBenchmark(OBS, D, ACT, STAT, hidden_dim, t_max, 1, ode_type=kind, t0=t0, device=dev)
    init = (torch.randn(B, D, generator=gen) * 0.5).to(dev)
    a = ((torch.rand(t_max, B, 1, generator=gen) < 0.15).float() * torch.rand(t_max, B, 1, generator=gen)).to(dev)
    s = torch.rand(t_max, B, STAT, generator=gen).to(dev)
    T = dec.t.numel()
    cot = torch.randn(T, B, OBS, generator=gen).to(dev)
    params = list(dec.parameters())

    # ---- kernels alone, through the C ABI
    idx, tau, _ = dec._step_tables(dev)
    r = dec.rnn
    w = (r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0) if kind == "tlstm" else (r.lin_hz.weight, r.lin_hn.weight, None, None)
    w = [None if x is None else x.detach().contiguous() for x in w]
    kd = L.SEQDEC_TLSTM if kind == "tlstm" else L.SEQDEC_GRUODE
    h = torch.empty(T, B, D, device=dev)
    c = torch.empty_like(h)
    d = seqdec._desc(kd, init, a, idx, tau, w[0], w[1], w[2], w[3], h)
    d.c = c.data_ptr() if kind == "tlstm" else 0
    gh = torch.randn(T, B, D, device=dev)
    grads = [torch.empty_like(init)] + [None if x is None else torch.empty_like(x) for x in w]
    d.grad_h, d.grad_init = gh.data_ptr(), grads[0].data_ptr()
    d.grad_w0, d.grad_w1 = grads[1].data_ptr(), grads[2].data_ptr()
    d.grad_b0 = 0 if grads[3] is None else grads[3].data_ptr()
    d.grad_b1 = 0 if grads[4] is None else grads[4].data_ptr()
    lib = L.lib()
    nws = lib.hode_seqdec_workspace_bytes(d)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nws
    L.check(lib.hode_seqdec_fwd(d, _stream()), "fwd")
    k_fwd = timed(lambda: L.check(lib.hode_seqdec_fwd(d, _stream()), "fwd"), 50)
    k_bwd = timed(lambda: L.check(lib.hode_seqdec_bwd(d, _stream()), "bwd"), 50)

    # ---- decoder forward + backward (kernels, readout MLP, autograd glue)
    def dec_step():
        for p in params:
            p.grad = None
        ig = init.clone().requires_grad_(True)
        x_hat, _ = dec(ig, a, s)
        (x_hat * cot).sum().backward()
    t_dec = timed(dec_step, 20)

    # ---- the reference-style eager loop on the same GPU
    def eager_step():
        for p in params:
            p.grad = None
        ig = init.clone().requires_grad_(True)
        x_hat = dec.output_function(eager_latent(dec, ig, a))
        (x_hat * cot).sum().backward()
    t_eager = timed(eager_step, 3)
    out = {"kind": kind, "batch": B, "t_max": t_max, "t0": t0, "latent": D, "steps": T,
           "kernel_fwd_ms": round(k_fwd, 4), "kernel_bwd_ms": round(k_bwd, 4),
           "decoder_fwd_bwd_ms": round(t_dec, 4), "eager_loop_fwd_bwd_ms": round(t_eager, 3),
           "speedup_vs_eager_loop": round(t_eager / t_dec, 1)}
    if kind == "tlstm":
        obs_all = torch.cat([a[idx.long()], tau.view(T, 1, 1).expand(T, B, 1)], dim=-1)

        def lstm_step():
            for p in params:
                p.grad = None
            ig = init.clone().requires_grad_(True)
            hh, _ = dec.rnn(obs_all, (ig[None], ig[None]))
            (dec.output_function(hh) * cot).sum().backward()
        t_lstm = timed(lstm_step, 10)
        out["nn_lstm_one_call_fwd_bwd_ms"] = round(t_lstm, 4)
        out["speedup_vs_nn_lstm"] = round(t_lstm / t_dec, 2)

    # ---- parity against the eager loop in this run
    for p in params:
        p.grad = None
    ig = init.clone().requires_grad_(True)
    x_hat, hk = dec(ig, a, s)
    (x_hat * cot).sum().backward()
    gk = [ig.grad.clone()] + [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    ie = init.clone().requires_grad_(True)
    he = eager_latent(dec, ie, a)
    (dec.output_function(he) * cot).sum().backward()
    ge = [ie.grad] + [p.grad for p in params]
    out["parity_max_abs_h"] = float((hk - he).detach().abs().max())
    out["parity_max_rel_l2_grad"] = max(float((x - y).norm() / y.norm()) for x, y in zip(gk, ge))

    # ---- run_real-shaped training step (encoder, decoder, fused loss, Adam)
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

    # ---- bounds
    f_fwd, f_bwd = (2 * 16 * 16 * 4 * n for n in mfma_count(kind, D, B, T))
    row = T * B * D * 4
    b_fwd = row * (2 if kind == "tlstm" else 1) + T * B * 4
    b_bwd = row * (3 if kind == "tlstm" else 1) + T * B * 4 + B * D * 4
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
    ap.add_argument("--latent", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind in ("tlstm", "gruode"):
        print(json.dumps(probe(kind, args.batch, args.t_max, args.t0, args.latent, dev)), flush=True)


if __name__ == "__main__":
    main()
