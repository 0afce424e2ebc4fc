"""Eager restatement of the real-data recurrent baseline decoders (``model.DecoderRealBenchmark``), written from the
reference's semantics (model.py:865-966): the CPU reference of tests/test_hip_seqdec.py.  tests/test_seqdec_host.py pins
it against the golden fixture G9 recorded from the reference itself.

    step k = 0 .. T'-1 reads the action row t_k = int(t[k]) and the time feature fp32(t_k) / t_max;
    tlstm : LSTM(2, D) with h0 = c0 = init, h[k] = hidden state after step k;
    gruode: h[k] = (1 - z[:D]) * (tanh(W_n (z * x_k)) - init), z = sigmoid(W_z x_k), x_k = [init, a[t_k], tau_k]
            (the reference's decoder hands the cell `init` as its state at every step)."""
import torch


def tables(t, t_max):
    rows = [int(v) for v in t.detach().cpu().tolist()]
    tau = torch.ones(len(rows), dtype=torch.float32, device=t.device) * torch.tensor(rows, dtype=torch.float32, device=t.device) / t_max
    return rows, tau


def tlstm(init, a, rows, tau, w_ih, w_hh, b_ih, b_hh):
    D = init.shape[1]
    h, c = init, init
    out = []
    for k, t in enumerate(rows):
        x = torch.cat([a[t], tau[k] * torch.ones_like(a[t])], dim=-1)
        gates = x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, g, o = (gates[:, q * D:(q + 1) * D] for q in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out, dim=0)


def gruode(init, a, rows, tau, w_z, w_n):
    D = init.shape[1]
    T, B = len(rows), init.shape[0]
    act = a[rows]                                               # (T', B, 1)
    x = torch.cat([init.expand(T, B, D), act, tau.view(T, 1, 1) * torch.ones_like(act)], dim=-1)
    z = torch.sigmoid(x @ w_z.t())
    n = torch.tanh((z * x) @ w_n.t())
    return (1 - z[..., :D]) * (n - init)


def decoder_latent(dec, init, a):
    """h of a ``model.DecoderRealBenchmark`` computed eagerly from its parameters."""
    rows, tau = tables(dec.t, dec.t_max)
    if dec.ode_type == "tlstm":
        r = dec.rnn
        return tlstm(init, a, rows, tau, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)
    return gruode(init, a, rows, tau, dec.rnn.lin_hz.weight, dec.rnn.lin_hn.weight)


def decoder_forward(dec, init, a):
    h = decoder_latent(dec, init, a)
    return dec.output_function(h), h
