"""``model.DecoderReal`` called with per-step initial states (a 3-D ``init``: the reference's one-step-ahead mode,
model.py:833-862) on CPU tensors with the oracle solver injected, against G18, the fixture recorded from the REFERENCE's class
(tests/golden/make_golden_real_step.py), under the bounds tests/test_lstm_baseline.py holds G17 to: outputs
2e-6 (1 + max|.|) absolute, gradients 2e-4 rel-L2.  Also the mode's structure (zero rows, the ``x_hat[0]`` cut, rows of
``init`` beyond t_max - 1 ignored) and every refusal, raised before a kernel library is loaded.  The GPU counterpart is
tests/test_hip_real_step.py."""
import os

import numpy as np
import pytest
import torch

import model
from oracle.solvers import odeint as oracle_odeint

TOL_OUT, TOL_G = 2e-6, 2e-4   # tests/test_lstm_baseline.py: TOL_OUT, TOL_G
METHODS = {0: "euler", 1: "midpoint", 2: "rk4"}
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_real_step.npz"), allow_pickle=False)


def load_decoder(g, k, device=CPU):
    """The decoder of case k with the fixture's weights (the reference's own state_dict keys), and its inputs."""
    T, B, obs, act, stat, hid = [int(v) for v in g["meta"]]
    D, t0, m, div = [int(v) for v in g["cases"][k]]
    dec = model.DecoderReal(obs, D, act, stat, hid, T, 1, t0=t0, method=METHODS[m], ode_step_size=1.0 / div, ode_type="hybrid", device=device)
    pre = "c%d_sd_" % k
    dec.load_state_dict({n[len(pre):].replace("__", "."): torch.from_numpy(g[n]) for n in g.files if n.startswith(pre)}, strict=True)
    dec._odeint = oracle_odeint
    inputs = {n: torch.from_numpy(g["c%d_%s" % (k, n)]) for n in ("init", "c1", "c2")}
    inputs["a"], inputs["s"] = torch.from_numpy(g["actions"]), torch.from_numpy(g["statics"])
    return dec, inputs


def close(got, want, tol=TOL_OUT):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= tol * (1 + np.abs(want).max()), err


def rel(got, want):
    got, want = got.detach().cpu().numpy().ravel(), np.asarray(want).ravel()
    return np.linalg.norm(got - want) / np.linalg.norm(want)


def check_case(g, k, dec, p, tol_out=TOL_OUT, tol_g=TOL_G):
    """Forward + backward of sum(x_hat c1) + sum(h c2) against the fixture; shared with the GPU file."""
    dev = p["init"].device
    init = p["init"].clone().requires_grad_(True)
    x_hat, h = dec(init, p["a"], p["s"])
    ((x_hat * p["c1"]).sum() + (h * p["c2"]).sum()).backward()
    close(x_hat, g["c%d_x_hat" % k], tol_out)
    close(h, g["c%d_h" % k], tol_out)
    T = h.shape[0]
    assert bool((h[0] == 0).all()) and bool((x_hat[0] == 0).all()) and x_hat.shape[0] == T - 1
    assert bool((init.grad[T - 1:] == 0).all()) and bool((init.grad[:T - 1] != 0).any(dim=(1, 2)).all())
    assert rel(init.grad, g["c%d_g_init" % k]) <= tol_g
    for n, q in dec.named_parameters():
        assert q.grad is not None and rel(q.grad, g["c%d_g_%s" % (k, n.replace(".", "__"))]) <= tol_g, n
    assert dev == init.grad.device


def test_the_fixture_holds_the_cases_the_issue_names(g18):
    rows = {tuple(int(v) for v in r) for r in g18["cases"]}
    assert rows == {(D, t0, m, div) for D in (7, 20) for t0 in (0, 1) for m, div in ((1, 1), (2, 2), (0, 1))}
    assert [int(v) for v in g18["meta"]] == [8, 5, 6, 1, 3, 5]
    assert all(float(np.abs(g18["c%d_h" % k]).max()) < 2 for k in range(len(rows)))


@pytest.mark.parametrize("k", range(12))
def test_decoder_reproduces_the_reference(g18, k):
    dec, p = load_decoder(g18, k)
    check_case(g18, k, dec, p)


def test_the_structure_of_the_mode(g18):
    """h[0] and x_hat[0] are zero; x_hat[0] sends nothing back, h[1] does; rows of init beyond t_max - 1 change nothing."""
    dec, p = load_decoder(g18, 0)
    T = p["init"].shape[0]
    init = p["init"].clone().requires_grad_(True)
    x_hat, h = dec(init, p["a"], p["s"])
    assert h.shape == (T, 5, 7) and x_hat.shape == (T - 1, 5, 6)
    gx, = torch.autograd.grad(x_hat.sum(), init, retain_graph=True)
    nonzero = [bool(r.any()) for r in gx]
    assert nonzero == [False] + [True] * (T - 2) + [False], nonzero   # the cut of x_hat[0]; the unused last row
    gh, = torch.autograd.grad(h[1].sum(), init)
    assert bool(gh[0].any()) and not bool(gh[1:].any())
    longer = torch.cat([p["init"], torch.full((3, 5, 7), float("nan"))])
    x2, h2 = dec(longer, p["a"], p["s"])
    assert torch.equal(x2, x_hat) and torch.equal(h2, h)
    assert torch.equal(dec.latent(p["init"], p["a"], p["s"]), h)
    # the 2-D mode is what it was
    x1, h1 = dec(p["init"][0], p["a"], p["s"])
    assert h1.shape == (dec.t.numel(), 5, 7) and x1.shape[0] == dec.t.numel() - 1 and bool((x1[0] != 0).any())


def _refusal_setup(monkeypatch, tmp_path):
    from hode import _real_dims_lib as RD, _real_step_lib as RS
    for lib in (RS.LIBRARY, RD.LIBRARY):
        monkeypatch.setattr(lib, "handle", None)
        monkeypatch.setattr(lib, "directory", str(tmp_path))   # nothing to load there
    return RS


def _solve(D=7, H=5, rows=3, t=None, **kw):
    from hode import real_step
    t = torch.arange(0.0, 4.0) if t is None else t
    return real_step.real_step_solve(torch.zeros(rows, 2, D), torch.zeros(3), torch.zeros(9 * max(H, 0) + 2 + 3 * (D - 4) ** 2), t,
                                     torch.zeros(4, 2), H, **kw)


def test_real_step_solve_refuses_before_any_launch(monkeypatch, tmp_path):
    """Every refusal of hode.real_step.real_step_solve: HodeConfigError that names what is served, on CPU tensors, with no
    kernel library loaded afterwards."""
    import hode
    RS = _refusal_setup(monkeypatch, tmp_path)
    served = "latent_dim 5 .. 20 with hidden_dim 1 .. 64"
    for kw, pat in ((dict(D=4), "latent_dim 4 with hidden_dim 5"), (dict(D=21), "latent_dim 21 with hidden_dim 5"),
                    (dict(H=0), "latent_dim 7 with hidden_dim 0"), (dict(H=65), "latent_dim 7 with hidden_dim 65")):
        with pytest.raises(hode.HodeConfigError, match=pat) as e:
            _solve(**kw)
        assert served in str(e.value) and "libhode_real_step.so" in str(e.value)
    with pytest.raises(hode.HodeConfigError, match="same number of solver steps in every interval") as e:
        _solve(t=torch.tensor([0.0, 1.0, 3.0, 4.0]), step_size=1.0)
    assert "1 .. 8 solver steps" in str(e.value)
    with pytest.raises(hode.HodeConfigError, match="no kernel for 9 solver steps per interval") as e:
        _solve(step_size=1.0 / 9)
    assert "1 .. 8 solver steps" in str(e.value)
    with pytest.raises(hode.HodeConfigError, match="needs 3 start states .one per interval.; init has 2 rows"):
        _solve(rows=2)
    with pytest.raises(hode.HodeConfigError, match="needs 1 start states"):
        _solve(t=torch.tensor([0.0]))
    with pytest.raises(hode.HodeConfigError, match="fixed-grid methods"):
        _solve(method="dopri5")
    with pytest.raises(hode.HodeConfigError, match="got 2-D"):
        from hode import real_step
        real_step.real_step_solve(torch.zeros(2, 7), torch.zeros(3), torch.zeros(74), torch.arange(0.0, 4.0), torch.zeros(4, 2), 5)
    # a served configuration goes on to the device check, still without loading anything
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        _solve(step_size=0.5)
    assert RS.LIBRARY.handle is None


def _decoder(ode_type="hybrid", t0=0, T=8, D=7, cls=None, device=CPU):
    cls = model.DecoderReal if cls is None else cls
    return cls(6, D, 1, 3, 5, T, 1, t0=t0, method="midpoint", ode_step_size=1.0, ode_type=ode_type, device=device)


def test_decoder_refusals(monkeypatch, tmp_path):
    """t0 >= 2 (fewer grid points than t_max), too few rows, and the kernel path's own refusals through the decoder."""
    import hode
    RS = _refusal_setup(monkeypatch, tmp_path)
    a, s = torch.zeros(8, 2, 1), torch.zeros(8, 2, 3)
    for odeint in (oracle_odeint, hode.odeint):
        dec = _decoder(t0=2)
        dec._odeint = odeint
        with pytest.raises(hode.HodeConfigError, match="at least t_max = 8 points, this decoder's has 7 .t0 = 2.*fewer than two time points"):
            dec(torch.zeros(8, 2, 7), a, s)
        dec = _decoder(t0=1)
        dec._odeint = odeint
        with pytest.raises(hode.HodeConfigError, match=r"t_max - 1 = 7, B, D.*got \(6, 2, 7\)"):
            dec(torch.zeros(6, 2, 7), a, s)
        with pytest.raises(hode.HodeConfigError, match=r"got \(1, 6, 2, 7\)"):
            dec.latent(torch.zeros(1, 6, 2, 7), a, s)
    for D in (4, 21):   # the kernel path: refused by real_step_solve; the oracle loop has no such limit
        dec = _decoder(D=D)
        with pytest.raises(hode.HodeConfigError, match="latent_dim %d with hidden_dim 5" % D):
            dec(torch.zeros(7, 2, D), a, s)
    dec = _decoder()
    dec.options["step_size"] = 0.1
    with pytest.raises(hode.HodeConfigError, match="no kernel for 10 solver steps"):
        dec(torch.zeros(7, 2, 7), a, s)
    dec = _decoder()
    with pytest.raises(hode.HodeConfigError, match="HIP device"):
        dec(torch.zeros(7, 2, 7), a, s)
    assert RS.LIBRARY.handle is None


def test_the_baselines_still_refuse_and_name_the_hybrid_decoder(monkeypatch):
    import hode
    a, s = torch.zeros(8, 2, 1), torch.zeros(8, 2, 3)
    for ode_type in ("tlstm", "gruode"):
        dec = _decoder(ode_type, cls=model.DecoderRealBenchmark)
        monkeypatch.setattr("hode.solver._require_gpu", lambda *x: None)
        with pytest.raises(hode.HodeConfigError, match="3-D init.*DecoderReal.ode_type='hybrid'. serves them"):
            dec.latent(torch.zeros(7, 2, 7), a, s)
    # neural / 2nd construct on a HIP device only: the branch is exercised on a hybrid decoder whose rhs is swapped
    for cls in (model.NeuralODEReal, model.NeuralODEReal2nd):
        dec = _decoder()
        dec.ode = cls(8, 1, 3, 5, 8, 1, CPU)
        dec.model_name = "DecoderReal_" + cls.kind
        for call in (dec.forward, dec.latent):
            with pytest.raises(hode.HodeConfigError, match="DecoderReal_%s.*3-D init.*served by the hybrid decoder" % cls.kind):
                call(torch.zeros(7, 2, 8), a, s)
