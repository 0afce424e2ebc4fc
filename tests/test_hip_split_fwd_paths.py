"""The split forward (hode_rk_split.hip, lanes_per_patient = 48) on the shapes where its prologue, ring parities, last-step
guards, spare lanes and dose paths can go wrong -- not the bench shape.  GPU only.

Tolerances are those of tests/test_hip_rk.py::_compare: h within 2e-5 * (1 + max|h|), gradients within 1e-4 (rel-L2) of the
CPU oracle.  The cases:
  * B in {1, 47, 48, 49, 97} (spare lanes of the expert wave; one workgroup, one plus a patient, two plus a patient) x
    T in {2, 3, 4, 5, 8} (prologue only, both ring parities, the guards of the last step), with D, the method, perturb and
    the doses per patient (0, 1, 2, 3: the `a.K == 0` path, the one-dose body, the table-walking body) rotating over them;
  * general Hill exponents (the non-HILL2 body) and the ablated rhs, with one dose and with two;
  * a dose exactly on a grid point, one ulp before and one ulp after it, with and without perturbed stage times;
  * the forward with and without the tape: byte-equal h, and the same h as the oracle's;
  * a NaN in one patient's y0: the status word reports it, every other patient keeps the bits of the clean run.
"""
import itertools

import pytest
import torch

from test_hip_rk import _case, _compare, _dev, _run_hip, _run_oracle

pytestmark = pytest.mark.gpu

METHODS = ("euler", "midpoint", "rk4")
HILL_THETA = (3.0, 1.5, 0.8, 1.3, 0.7, 0.9, 1.1, 0.6, 1.2, 0.5, 1.4, 0.75, 0.65)  # HillCure, HillPatho != 2
SHAPES = list(itertools.product((1, 47, 48, 49, 97), (2, 3, 4, 5, 8)))


def _rotation(i):
    """D, method, perturb and doses per patient of shape i: over twelve consecutive shapes every (D, method, perturb)
    occurs once, the dose count moves every third shape."""
    return (8, 12)[i % 2], METHODS[i % 3], bool((i // 2) % 2), (i // 3) % 4


def _cot(T, N, D, seed):
    return torch.randn(T, N, D, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=lambda i: "B%d-T%d-D%d-%s-p%d-K%d" % (SHAPES[i] + tuple(_rotation(i))))
def test_shapes_and_dose_counts(i):
    (N, T), (D, method, perturb, n_dose) = SHAPES[i], _rotation(i)
    dev = _dev()
    inp, f = _case(N, T, D, seed=300 + i, n_dose=n_dose)  # at most T - 1 doses fit the grid
    cot = _cot(T, N, D, 40 + i)
    _compare(_run_hip(inp, f, method, 48, dev, perturb=perturb, cot=cot), _run_oracle(inp, f, method, perturb=perturb, cot=cot))


@pytest.mark.parametrize("D", [8, 12])
@pytest.mark.parametrize("n_dose", [1, 2])
@pytest.mark.parametrize("kind", ["hill", "ablate"])
def test_general_hill_and_ablated_bodies(kind, n_dose, D):
    dev = _dev()
    N, T = 49, 5
    inp, f = _case(N, T, D, seed=330 + D + n_dose, n_dose=n_dose, ablate=kind == "ablate", theta=HILL_THETA if kind == "hill" else None)
    cot = _cot(T, N, D, 70)
    for method, perturb in (("rk4", False), ("midpoint", True), ("euler", False)):
        _compare(_run_hip(inp, f, method, 48, dev, perturb=perturb, cot=cot), _run_oracle(inp, f, method, perturb=perturb, cot=cot))


def _solve_with_times(inp, f, times, dosage, method, perturb, dev, cot):
    """The solve of `_run_hip` / `_run_oracle` with the dose times given, not derived from an action tensor."""
    from hode.solver import pack_theta, roche_solve
    from oracle.rhs import THETA_NAMES
    from oracle.solvers import odeint as oracle_odeint
    theta = pack_theta([getattr(f, n).detach().to(dev) for n in THETA_NAMES], dev)
    y0 = inp["z0"].to(dev).requires_grad_(True)
    w = f.ml_net[0].weight.detach().clone().to(dev).requires_grad_(True)
    b = f.ml_net[0].bias.detach().clone().to(dev).requires_grad_(True)
    h = roche_solve(y0, theta, w, b, inp["t"].to(dev), dosage.to(dev), times.to(dev), method=method, perturb=perturb, lanes_per_patient=48)
    (h * cot.to(dev)).sum().backward()
    hip = {"h": h.detach().cpu(), "gy0": y0.grad.cpu(), "gw": w.grad.cpu(), "gb": b.grad.cpu()}
    f.dosage, f.times = dosage, times
    f.zero_grad()
    y0c = inp["z0"].clone().requires_grad_(True)
    ho = oracle_odeint(f, y0c, inp["t"], method=method, options={"perturb": perturb} if perturb else None)
    (ho * cot).sum().backward()
    return hip, {"h": ho.detach(), "gy0": y0c.grad, "gw": f.ml_net[0].weight.grad, "gb": f.ml_net[0].bias.grad}


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("K", [1, 2])
def test_dose_on_a_grid_point_and_one_ulp_beside_it(K, perturb):
    """Patient 3j + 0 is dosed exactly at a grid point, 3j + 1 one ulp before it, 3j + 2 one ulp after it: whether stage 0 of
    that step and the last stage of the step before see the dose turns on one comparison per stage time."""
    dev = _dev()
    N, T, D = 49, 6, 12
    inp, f = _case(N, T, D, seed=350 + K)
    t = inp["t"]
    point = t[1 + torch.arange(N) % (T - 2)]
    side = torch.arange(N) % 3
    tau = torch.where(side == 1, torch.nextafter(point, point - 1), torch.where(side == 2, torch.nextafter(point, point + 1), point))
    times = tau[:, None] if K == 1 else torch.stack([t[0].expand(N), tau], dim=1)
    dosage = 1.0 + 5.0 * torch.rand(N, generator=torch.Generator().manual_seed(9))
    cot = _cot(T, N, D, 71)
    for method in METHODS:
        _compare(*_solve_with_times(inp, f, times.contiguous(), dosage, method, perturb, dev, cot))


def _plan(inp, f, method, perturb, tape, dev):
    from hode.plan import RocheRKPlan
    from hode.solver import pack_theta
    from oracle.rhs import THETA_NAMES, dose_schedule
    theta = pack_theta([getattr(f, n).detach().to(dev) for n in THETA_NAMES], dev)
    dosage, times = dose_schedule(inp["actions"], f.step_size)
    return RocheRKPlan(inp["z0"].to(dev), theta, f.ml_net[0].weight.detach().to(dev), f.ml_net[0].bias.detach().to(dev),
                       inp["t"].to(dev), dosage.to(dev), times.to(dev), method=method, perturb=perturb, lanes_per_patient=48, tape=tape)


@pytest.mark.parametrize("D", [8, 12])
@pytest.mark.parametrize("method", METHODS)
def test_h_does_not_depend_on_the_tape(D, method):
    """Two plans on the same inputs, one leaving the tape and one not: the forward's stores of h are the same bytes, and
    they are the oracle's trajectory."""
    dev = _dev()
    for N, T, n_dose, perturb in ((97, 8, 1, False), (49, 3, 2, True), (1, 2, 1, False)):
        inp, f = _case(N, T, D, seed=370 + D + N, n_dose=n_dose)
        hs = []
        for tape in (True, False):
            plan = _plan(inp, f, method, perturb, tape, dev)
            plan.h.fill_(-7.25)
            plan.forward()
            torch.cuda.synchronize()
            hs.append(plan.h.cpu())
        assert torch.equal(hs[0].view(torch.int32), hs[1].view(torch.int32))
        _compare({"h": hs[1]}, _run_oracle(inp, f, method, perturb=perturb), grads=False)


@pytest.mark.parametrize("D", [8, 12])
def test_more_workgroups_than_cus_take_the_four_wave_launch_with_the_same_bits(D):
    """With one dose per patient the launch carries a dose wave while every workgroup has a CU to itself, and leaves the
    doses with the learned waves past that (split_method).  Patients do not interact, so the first 96 patients of a batch of
    more workgroups than the device has CUs must come out with the bits they have in a batch of their own; a sample of the
    large batch is also held against the oracle."""
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N, T = 48 * (cus + 1) + 1, 4
    inp, f = _case(N, T, D, seed=380 + D)
    head = {"z0": inp["z0"][:96].clone(), "actions": inp["actions"][:, :96].clone(), "t": inp["t"]}
    for method, perturb in (("rk4", False), ("midpoint", True), ("euler", False)):
        big, small = _plan(inp, f, method, perturb, True, dev), _plan(head, f, method, perturb, True, dev)
        for plan in (big, small):
            plan.h.fill_(-7.25)
            plan.forward()
        torch.cuda.synchronize()
        assert torch.equal(big.h[:, :96].contiguous().view(torch.int32), small.h.view(torch.int32))
        pick = torch.arange(0, N, 97)
        part = {"z0": inp["z0"][pick].clone(), "actions": inp["actions"][:, pick].clone(), "t": inp["t"]}
        _compare({"h": big.h[:, pick.to(dev)].cpu()}, _run_oracle(part, f, method, perturb=perturb), grads=False)


@pytest.mark.parametrize("tape", [False, True])
@pytest.mark.parametrize("D,N,row", [(12, 97, 48), (8, 49, 47), (12, 47, 0)])
def test_status_reports_a_nan_patient_and_the_others_are_unchanged(D, N, row, tape):
    dev = _dev()
    from hode import _lib as L
    from hode.solver import pack_theta
    from oracle.rhs import THETA_NAMES, dose_schedule
    T = 5
    inp, f = _case(N, T, D, seed=390 + D)
    theta = pack_theta([getattr(f, n).detach().to(dev) for n in THETA_NAMES], dev).contiguous()
    dosage, times = dose_schedule(inp["actions"], f.step_size)
    keep = [theta, inp["t"].to(dev), dosage.to(dev).float().contiguous(), times.to(dev).float().contiguous(),
            f.ml_net[0].weight.detach().to(dev).contiguous(), f.ml_net[0].bias.detach().to(dev).contiguous()]
    lib = L.lib()

    def forward(y0):
        h = torch.full((T, N, D), -7.25, device=dev)
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        d = L.new_solve_desc()
        d.rhs_kind, d.method, d.perturb, d.batch, d.latent_dim, d.n_times, d.n_dose = L.RHS_ROCHE, L.METHODS["rk4"], 0, N, D, T, 1
        d.lanes_per_patient = 48
        d.theta, d.t, d.dosage, d.dose_times, d.w1, d.b1 = (x.data_ptr() for x in keep)
        d.y0, d.h, d.status = y0.data_ptr(), h.data_ptr(), status.data_ptr()
        d.flags = L.FLAG_TAPE if tape else 0
        n = lib.hode_workspace_bytes(d, L.WS_RK_FWD)
        ws = torch.empty(max(n, 4), device=dev, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        L.check(lib.hode_rk_fwd(d, torch.cuda.current_stream().cuda_stream), "hode_rk_fwd")
        torch.cuda.synchronize()
        return int(status), h

    y0 = inp["z0"].to(dev).contiguous()
    word, clean = forward(y0)
    assert word == 0 and bool(torch.isfinite(clean).all())
    bad = y0.clone()
    bad[row, 1] = float("nan")   # an expert component: it reaches the learned block of the same patient through the ring
    word, h = forward(bad)
    assert word == L.STATUS_NONFINITE
    others = [p for p in range(N) if p != row]
    assert torch.equal(h[:, others].view(torch.int32), clean[:, others].view(torch.int32))
    assert not bool(torch.isfinite(h[-1, row]).all())
