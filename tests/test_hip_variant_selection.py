"""Kernel variants are selected through descriptor fields and keyword arguments, never through the process environment:
with every former tuning variable set (test_abi.STALE_ENV) each wrapper returns, bit for bit, what it returns in a clean
environment -- forward and backward, in one process.  The folds are fixed-order, so the kernels are run-to-run
reproducible and torch.equal is the bound.  GPU only."""
import pytest
import torch

from test_abi import STALE_ENV

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _backward(out, inputs, seed):
    """[out, grads of `inputs`] for the loss sum(out * cot) with a seeded cotangent."""
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    return [out.detach()] + [x.grad for x in inputs]


def _leaves(tensors, dev):
    return [x.detach().clone().to(dev).requires_grad_(True) for x in tensors]


def _neural(dev):
    """rk4, D = 14 (the lane layout has no such kernel), B = 17: one past a 16-patient wave."""
    from hode.neural import neural_solve
    D, B, T = 14, 17, 3
    gen = torch.Generator().manual_seed(14)
    prm = _leaves([torch.randn(10 * D, D + 1, generator=gen) * 0.3, torch.randn(10 * D, generator=gen) * 0.1,
                   torch.randn(D, 10 * D, generator=gen) * 0.1, torch.randn(D, generator=gen) * 0.1,
                   torch.randn(B, D, generator=gen)], dev)
    t = (torch.arange(T, dtype=torch.float32) * 0.375).to(dev)
    dosage = torch.rand(B, generator=gen).to(dev)
    times = torch.full((B, 1), 0.375).to(dev)  # on the grid: the impulse fires
    h = neural_solve(prm[4], *prm[:4], t, dosage, times, method="rk4")
    return _backward(h, prm, 1)


def _real(dev):
    """midpoint + perturb, D = 20, hidden 17 (two hidden tiles, the second ragged), B = 17."""
    from hode.real import real_solve
    D, H, B, T, Ta = 20, 17, 17, 3, 12
    gen = torch.Generator().manual_seed(20)
    prm = _leaves([torch.randn(B, D, generator=gen) * 0.3, torch.tensor([0.3, 0.2, 0.1]),
                   torch.randn(9 * H + 2 + 3 * (D - 4) ** 2, generator=gen) * 0.2], dev)
    t = torch.arange(7, 7 + T, dtype=torch.float32).to(dev)
    act = ((torch.rand(Ta, B, generator=gen) < 0.3).float() * torch.rand(Ta, B, generator=gen)).to(dev)
    h = real_solve(*prm, t, act, H, method="midpoint", perturb=True)
    return _backward(h, prm, 2)


def _roche(dev):
    """rk4, D = 12, B = 49: one past a 48-patient block of the split layout."""
    from hode import synth
    from hode.solver import pack_theta, roche_solve
    from oracle.rhs import RocheRHS, THETA_NAMES, dose_schedule
    D, B, T = 12, 49, 4
    inp = synth.solver_inputs(B, T, D, seed=12)
    torch.manual_seed(12)
    f = RocheRHS(D, synth.STEP)
    theta = pack_theta([getattr(f, n).detach().to(dev) for n in THETA_NAMES], dev)
    prm = _leaves([inp["z0"], f.ml_net[0].weight, f.ml_net[0].bias], dev)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    h = roche_solve(prm[0], theta, prm[1], prm[2], inp["t"].to(dev), dosage.to(dev), times.to(dev), method="rk4")
    return _backward(h, prm, 3)


def _lstm(dev):
    """H = 40 (padded to 48), obs = 20, B = 37: ragged against every patient tile."""
    from hode.lstm import lstm_encode
    H, obs, B, T = 40, 20, 37, 3
    gen = torch.Generator().manual_seed(40)
    torch.manual_seed(40)
    lstm = torch.nn.LSTM(obs + 1, H)
    prm = _leaves([lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0], dev)
    x = torch.randn(T, B, obs, generator=gen).to(dev)
    a = torch.rand(T, B, 1, generator=gen).to(dev)
    m = (torch.rand(T, B, obs, generator=gen) < 0.6).float().to(dev)
    return _backward(lstm_encode(x, a, m, *prm, reverse=True), prm, 4)


def _readout(dev):
    """D = 12, obs = 52: the first obs inside the matrix-core window; 32 rows."""
    from hode.readout import masked_sse_readout
    D, obs, T, B = 12, 52, 2, 16
    gen = torch.Generator().manual_seed(52)
    prm = _leaves([torch.randn(T, B, D, generator=gen), torch.randn(obs, D, generator=gen) * 0.3,
                   torch.randn(obs, generator=gen) * 0.1], dev)
    x = torch.randn(T, B, obs, generator=gen).to(dev)
    m = (torch.rand(T, B, obs, generator=gen) < 0.6).float().to(dev)
    lik = masked_sse_readout(prm[0], x, m, prm[1], prm[2])
    lik.backward()
    torch.cuda.synchronize()
    return [lik.detach()] + [p.grad for p in prm]


@pytest.mark.parametrize("call", [_neural, _real, _roche, _lstm, _readout], ids=lambda f: f.__name__.lstrip("_"))
def test_stale_tuning_variables_change_nothing(call, monkeypatch):
    dev = _dev()
    for name in STALE_ENV:
        monkeypatch.delenv(name, raising=False)
    clean = call(dev)
    for name, value in STALE_ENV.items():
        monkeypatch.setenv(name, value)
    stale = call(dev)
    assert len(clean) == len(stale) >= 4
    for i, (a, b) in enumerate(zip(clean, stale)):
        assert a is not None and torch.isfinite(a).all(), i
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
