"""Eager restatement of the real-data neural ODE baselines (``model.NeuralODEReal`` / ``NeuralODEReal2nd``), written from
the reference's semantics (model.py:660-862): the CPU reference of tests/test_hip_neural_real.py.
tests/test_neural_real_host.py pins it against the golden fixture G10 recorded from the reference itself.

    dose(t)  = cumsum(a, 0)[int(t)] per patient, int() truncating toward zero, zeros when int(t) >= Ta,
               negative rows indexed from the end;
    neural : dy/dt = m([y, dose(t)]),                 m = tanh(W2 tanh(W1 x + b1) + b2), W2: (D, H)
    2nd    : dy/dt = [m([y, dose(t)]), y[:, :D//2]],  W2: (D//2, H)
integrated by oracle.solvers.odeint with DecoderReal's options (perturb=True, step_size = 1 / ode_step_div)."""
import torch

from oracle.solvers import odeint


class Rhs(torch.nn.Module):
    def __init__(self, kind, w1, b1, w2, b2, a):
        super().__init__()
        self.kind, self.w1, self.b1, self.w2, self.b2, self.a = kind, w1, b1, w2, b2, a
        self.cs = torch.cumsum(a, dim=0)
        self.rows = []

    def dose(self, t):
        r = int(t)
        self.rows.append(r)
        if r >= self.a.shape[0]:
            return torch.zeros_like(self.a[0])
        return self.cs[r]

    def forward(self, t, y):
        x = torch.cat([y, self.dose(t)], dim=-1)
        m = torch.tanh(torch.tanh(x @ self.w1.t() + self.b1) @ self.w2.t() + self.b2)
        if self.kind == "2nd":
            return torch.cat([m, y[:, : y.shape[1] // 2]], dim=-1)
        return m


def solve(kind, y0, w1, b1, w2, b2, a, t, method, step_size=None, perturb=True):
    """h (len(t), B, D) and the action rows the rhs read, in call order."""
    f = Rhs(kind, w1, b1, w2, b2, a)
    opts = {"perturb": perturb}
    if step_size is not None:
        opts["step_size"] = step_size
    h = odeint(f, y0, t, method=method, options=opts)
    return h, f.rows


def decoder(kind, sd, init, a, t, method, step_size, prefix="ode.ml_net."):
    """x_hat, h of DecoderReal(ode_type=kind) with state_dict tensors ``sd`` (readout: Linear, ELU, Linear; row 0 dropped)."""
    h, rows = solve(kind, init, sd[prefix + "0.weight"], sd[prefix + "0.bias"], sd[prefix + "2.weight"], sd[prefix + "2.bias"],
                    a, t, method, step_size)
    z = torch.nn.functional.elu(h @ sd["output_function.0.weight"].t() + sd["output_function.0.bias"])
    x_hat = z @ sd["output_function.2.weight"].t() + sd["output_function.2.bias"]
    return x_hat[1:], h, rows
