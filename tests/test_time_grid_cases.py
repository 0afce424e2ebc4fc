"""Guard (no GPU) of tests/time_grids.py, the table tests/test_hip_time_grids.py runs against float64: it makes those GPU
tests meaningful and keeps a precision artefact from being mistaken for a kernel bug.

1. the grids' invariants (exact nodes, distinct neighbouring steps);
2. branch agreement: every (step, stage) time as the kernels form it in fp32 and as the oracle forms it in fp64 falls on the
   same side of every dose time of the case (and reads the same action row in the real-data families);
3. discrimination: the fp64 reference on the same nodes with the step sizes rotated by one position, and on the uniform
   grid of the same span, is at least 100 tolerances away from the true one, so a kernel that used a neighbour's dt fails;
4. fp32 headroom: the fp32 CPU oracle of every fixed-grid case is within half of each tolerance from fp64;
5. coverage: through the dispatch rules of tests/kernel_variants.py the table reaches every kernel family that takes a grid,
   and both ring depths of the split backward; the families of the three ragged-size side libraries (real_dims, real_step,
   neural_odd, neural_odd_dopri5) reach every kernel of libhode_real_dims.so, libhode_real_step.so and libhode_neural_odd.so;
6. the one-step-ahead sub-step grids: sub2 / sub3 give 2 / 3 solver steps per interval with a clipped last one, and a
   reference stepped along a wrong row of the (N, S + 1) table is >= 100 tolerances away."""
import numpy as np
import pytest
import torch

import kernel_variants as kv
import time_grids as tg
from reference_checks import GRAD_TOL, NEURAL_REAL_GRAD_TOL, TRAJ_TOL


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _traj(a, b):
    """Trajectory distance in units of test_hip_kernel_variants._traj_ok's bound."""
    return float((a.double() - b.double()).abs().max()) / (TRAJ_TOL * (1 + float(b.abs().max())))


# ----------------------------------------------------------------------------------------------------------- 1. grids
def test_ragged_steps_rule():
    s = tg.RAGGED_STEPS
    assert all(1 <= x <= 24 for x in s)
    for a, b in zip(s, s[1:]):
        assert max(a, b) >= 4 * min(a, b), (a, b)
    for i in range(len(s) - 3):
        assert len(set(s[i:i + 4])) == 4, s[i:i + 4]
    assert s[:9] == (8, 1, 24, 4, 16, 2, 12, 3, 20)


@pytest.mark.parametrize("name", ["ragged", "offset+", "offset-"])
def test_ragged_grids_are_exact_and_share_a_prefix(name):
    full = tg.grid64(name, tg.MAX_T)
    assert full[0] == tg.GRID_START[name]
    for T in range(1, tg.MAX_T + 1):
        t = tg.grid64(name, T)
        assert np.array_equal(t, full[:T])
        assert np.array_equal(t * 64, np.round(t * 64)) and np.all(np.diff(t) > 0)
        t32 = tg.grid(name, T).numpy()
        assert t32.dtype == np.float32 and np.array_equal(t32.astype(np.float64), t)
        dt32 = np.diff(t32)
        assert np.array_equal(dt32.astype(np.float64), np.diff(t)) and np.array_equal((dt32 / 2).astype(np.float64), np.diff(t) / 2)
    if name == "offset-":
        assert full[0] < 0 < full[-1]


def test_clustered_grid():
    t = tg.grid64("clustered", tg.DOPRI5_T)
    assert np.array_equal(t * 256, np.round(t * 256)) and np.all(np.diff(t) > 0)
    assert np.array_equal(tg.grid("clustered", tg.DOPRI5_T).numpy().astype(np.float64), t)
    d = np.diff(t) * 256
    run = best = 0
    for x in d:
        run = run + 1 if x == 1 else 0
        best = max(best, run)
    assert best + 1 >= 5 and d.max() >= 256  # a run of >= 5 nodes 1/256 apart, a gap >= 1.0


def test_case_table_is_well_formed():
    ids = [tg.case_id(c) for c in tg.CASES]
    assert len(ids) == len(set(ids)) and len(ids) <= 340
    for c in tg.CASES:
        assert tg.kernels(c)
        assert c["grid"] != "clustered" or c["family"] in ("dopri5", "neural_dopri5", "neural_odd_dopri5")
    # the side libraries' families come after the 240 cases of libhode.so's kernels, whose ids stay what they were
    import hashlib
    old = ids[:len(tg.OLD_CASES)]
    assert len(old) == 240 and tg.CASES[:240] == tg.OLD_CASES and 80 <= len(tg.SIDE_CASES) <= 100
    assert hashlib.sha256("\n".join(old).encode()).hexdigest() == "1e8b5bd52e89ca5499fbff82abf9b47c40ae0306b6ee0267daeeed0bbf2876df"
    assert {c["family"] for c in tg.SIDE_CASES} == {"real_dims", "real_step", "neural_odd", "neural_odd_dopri5"}


# ------------------------------------------------------------------------------------------------ 2. branch agreement
def _fixed(family):
    return tg.family(family)


@pytest.mark.parametrize("family", ["roche", "neural", "neural_odd"])
def test_fp32_and_fp64_stage_times_fall_on_the_same_side_of_every_dose_time(family):
    n = 0
    for c in _fixed(family):
        t = tg.grid64(c["grid"], c["T"])
        s32 = tg.stage_times32(t, c["method"], c["perturb"]).astype(np.float64).reshape(-1, 1)
        s64 = tg.stage_times64(t, c["method"], c["perturb"]).reshape(-1, 1)
        p = tg.roche_inputs(c) if family == "roche" else tg.neural_inputs(c)
        tau = np.unique(p["times"].numpy().astype(np.float64)).reshape(1, -1)
        assert np.array_equal(s32 >= tau, s64 >= tau), tg.case_id(c)
        assert np.array_equal(s32 == tau, s64 == tau), tg.case_id(c)
        n += s32.size * tau.size
        if family != "roche" and not c["perturb"]:
            assert (s32 == tau).any()  # the impulse fires somewhere
    assert n > 1000


def test_dose_placement():
    """On nodes (t[0] and the last-but-one included), before t[0] on the offset grids, inside a step for Roche; K = 1 and 3."""
    for fam in ("roche", "neural", "neural_odd"):
        cs = _fixed(fam)
        assert {c["n_dose"] for c in cs} == {1, 3}
        for c in cs:
            t = tg.grid64(c["grid"], c["T"])
            tau = (tg.roche_inputs(c) if fam == "roche" else tg.neural_inputs(c))["times"].numpy().astype(np.float64)
            assert tau.shape[1] == c["n_dose"]
            assert (tau == t[0]).any() and (tau == t[-2]).any()
            assert (tau < t[0]).any() == c["grid"].startswith("offset")
            inside = ~np.isin(tau, t) & (tau > t[0])
            assert inside.any() == (fam == "roche")
            if fam == "roche":
                assert np.isin(tau[inside], t[:-1] + np.diff(t) / 4).all()


def test_real_stage_times_read_the_same_action_row_in_fp32_and_fp64():
    """Roche real: floor(t) (csrc/hode_real_args.hpp real_dose); the oracle's `t >= k` for k = 1 .. Ta is the same row."""
    seen = set()
    for c in tg.family("real"):
        t = tg.grid64(c["grid"], c["T"])
        r32 = np.floor(tg.stage_times32(t, c["method"], c["perturb"]).astype(np.float64))
        r64 = np.floor(tg.stage_times64(t, c["method"], c["perturb"]))
        assert np.array_equal(r32, r64), tg.case_id(c)
        assert len(np.unique(r64)) >= 2  # stages on both sides of an integer
        frac = t - np.floor(t)
        assert (frac != 0).sum() >= len(t) - 2
        seen.update((c["grid"], int(r) > tg.REAL_TA[c["grid"]]) for r in np.unique(r64))
    assert ("offset+", True) in seen  # floor(t) past the last action row: the min(Ta, .) clamp


def _rows_of(t, method, perturb):
    """floor of every (step, stage) time of a grid as the kernels form it in fp32 and as the oracle forms it in fp64."""
    r32 = np.floor(tg.stage_times32(t, method, perturb).astype(np.float64))
    r64 = np.floor(tg.stage_times64(t, method, perturb))
    return r32, r64


def test_real_dims_stage_times_read_the_same_action_row_in_fp32_and_fp64():
    """libhode_real_dims.so: the same rule as the real family's.  Over the table: a step whose stages read two different
    rows (midpoint and rk4 each, so a stage that took its neighbour's row shows), a row past the last action row (the
    min(Ta, .) clamp binds), a negative stage time (n < 1 without "no dose yet")."""
    two_rows, past, negative = set(), False, False
    for c in tg.family("real_dims"):
        t = tg.grid64(c["grid"], c["T"])
        r32, r64 = _rows_of(t, c["method"], c["perturb"])
        assert np.array_equal(r32, r64), tg.case_id(c)
        assert len(np.unique(r64)) >= 2
        assert ((t - np.floor(t)) != 0).sum() >= len(t) - 2
        if (r64.min(axis=1) != r64.max(axis=1)).any():
            two_rows.add(c["method"])
        past |= bool((r64 > tg.REAL_TA[c["grid"]]).any())
        negative |= bool((tg.stage_times32(t, c["method"], c["perturb"]) < 0).any())
    assert two_rows == {"midpoint", "rk4"} and past and negative


def test_real_step_stage_times_read_the_same_action_row_in_fp32_and_fp64():
    """libhode_real_step.so: per interval, from the rows of hode.real_step.interval_grids -- the numbers the kernels walk --
    against the grid the fp64 oracle builds from step_size for that interval.  Over the table: the conditions of the
    real_dims test."""
    from oracle.solvers import _fixed_grid
    two_rows, past, negative = set(), False, False
    for c in tg.family("real_step"):
        p = tg.real_step_inputs(c)
        rows = tg.real_step_rows(c)
        assert rows.dtype == torch.float32 and rows.shape == (c["N"], c["S"] + 1)
        t64 = p["t"].double()
        for i in range(c["N"]):
            g64 = _fixed_grid(t64[i:i + 2], p["step_size"]).numpy()
            assert np.array_equal(rows[i].numpy().astype(np.float64), g64), (tg.case_id(c), i)
            r32 = np.floor(tg.stage_times32(rows[i].numpy(), c["method"], c["perturb"]).astype(np.float64))
            r64 = np.floor(tg.stage_times64(g64, c["method"], c["perturb"]))
            assert np.array_equal(r32, r64), (tg.case_id(c), i)
            if (r64.min(axis=1) != r64.max(axis=1)).any():
                two_rows.add(c["method"])
            past |= bool((r64 > p["Ta"]).any())
            negative |= bool((tg.stage_times32(rows[i].numpy(), c["method"], c["perturb"]) < 0).any())
        a = p["a"][:, 0, 0]
        assert float(a[0]) > 0 and float(a[-1]) > 0 and p["a"].shape[0] == p["Ta"]
    assert two_rows == {"midpoint", "rk4"} and past and negative
    # per grid, over its starts: doses lie before the window and inside it (dose k acts from t = k on), a stage reads past Ta
    for g in tg.SUB_STEPS:
        before = inside = beyond = 0
        for c in tg.family("real_step"):
            if c["grid"] != g:
                continue
            t, Ta = tg.step_grid64(g, c["start"], c["N"]), tg.STEP_TA[(g, c["start"])]
            k = np.arange(1, Ta + 1)
            before += int((k <= t[0]).any())
            inside += int(((k > t[0]) & (k < t[-1])).any())
            rows = tg.real_step_rows(c).numpy()
            beyond += int(any((np.floor(tg.stage_times32(r, c["method"], c["perturb"])) > Ta).any() for r in rows))
        assert before >= 1 and inside >= 1 and beyond >= 1, (g, before, inside, beyond)


def test_sub_step_grids_clip_the_last_sub_step_and_are_exact_in_fp32():
    """sub2 / sub3 with step_size 0.5 / 0.25: exactly 2 / 3 solver steps in every interval from all three starts, every value
    exact in fp32, the last sub-step clipped to a different length per interval, row i ends exactly on t[i + 1].  The ragged
    grid with step_size 0.125 mixes 1 and 2 steps and is refused."""
    import hode
    from hode.real_step import interval_grids
    want_last = {"sub2": (0.25, 0.5, 0.125, 0.375, 0.0625, 0.5, 0.1875), "sub3": (0.0625, 0.25, 0.125, 0.1875, 0.25, 0.03125, 0.234375)}
    for name, S in (("sub2", 2), ("sub3", 3)):
        step = tg.SUB_STEP_SIZE[name]
        for start in tg.STEP_STARTS:
            t64 = tg.step_grid64(name, start, 7)
            t32 = torch.tensor(t64, dtype=torch.float32)
            assert np.array_equal(t32.numpy().astype(np.float64), t64)
            rows = interval_grids(t32, step)
            assert rows.shape == (7, S + 1) and rows.dtype == torch.float32
            r = rows.numpy().astype(np.float64)
            assert np.array_equal(r[:, 0], t64[:-1]) and np.array_equal(r[:, -1], t64[1:])
            assert np.array_equal(r[:, :-1], t64[:-1, None] + step * np.arange(S)[None, :])  # exact: multiples of 1/64
            assert np.array_equal(r * 64, np.round(r * 64))
            d = np.diff(r, axis=1)
            assert np.all(d[:, :-1] == step) and tuple(d[:, -1]) == want_last[name]
            assert np.array_equal(np.diff(rows.numpy(), axis=1).astype(np.float64), d)  # dt as the kernels form it
            assert len(set(d[:, -1])) >= 5 and (d[:, -1] < step).sum() >= 5
    for start in tg.STEP_STARTS:
        with pytest.raises(hode.HodeConfigError, match="1 and 2"):
            interval_grids(torch.tensor(tg.step_grid64("ragged", start, 7), dtype=torch.float32), 0.125)
        assert interval_grids(torch.tensor(tg.step_grid64("ragged", start, 7), dtype=torch.float32)).shape == (7, 2)


def test_neural_real_stage_rows_match_the_fp64_eager_rows():
    """hode.neural_real.stage_rows (trunc of the fp32 stage times, on the host) against the rows the fp64 eager rhs reads."""
    from hode import neural_real
    neg = past = 0
    for c in tg.family("neural_real"):
        Ta = tg.REAL_TA[c["grid"]]
        rows = neural_real.stage_rows(tg.grid(c["grid"], c["T"]), c["method"], c["perturb"], Ta)
        t = tg.grid64(c["grid"], c["T"])
        r64 = np.trunc(tg.stage_times64(t, c["method"], c["perturb"])).astype(np.int64)
        assert np.array_equal(rows.numpy(), r64), tg.case_id(c)
        assert np.array_equal(np.trunc(tg.stage_times32(t, c["method"], c["perturb"]).astype(np.float64)), r64)
        _, eager_rows = tg.neural_real_solve_cpu(c)
        assert eager_rows == r64.reshape(-1).tolist(), tg.case_id(c)
        neg += int((r64 < 0).any())
        past += int((r64 >= Ta).any())
        if c["grid"] == "offset-":
            assert (r64 < 0).any() and len(np.unique(neural_real.table_index(rows, Ta).numpy())) >= 2
    assert neg >= 3 and past >= 3


# ------------------------------------------------------------------------------------------------- 3. discrimination
def _first(family, method, **kw):
    for c in tg.family(family):
        if c["method"] == method and all(c[k] == v for k, v in kw.items()):
            return c
    raise LookupError((family, method, kw))


def _solver(family, c):
    if family == "roche":
        p = tg.roche_inputs(c)
        return lambda t=None: tg.roche_solve_cpu(p, c["method"], c["perturb"], c["ablate"], t=t)
    if family == "neural":
        p = tg.neural_inputs(c)
        return lambda t=None: tg.neural_solve_cpu(p, c["method"], c["perturb"], t=t)
    if family == "neural_odd":
        p = tg.neural_inputs(c)
        return lambda t=None: tg.neural_solve_cpu(p, c["method"], c["perturb"], t=t)
    if family in ("real", "real_dims"):
        p, _ = tg.real_problem(c)
        return lambda t=None: tg.real_solve_cpu(c, p, t=t)
    if family == "real_step":
        p = tg.real_step_inputs(c)
        return lambda t=None: tg.real_step_solve_cpu(c, p, t=t)
    return lambda t=None: tg.neural_real_solve_cpu(c, t=t)[0]


def _grid64(c):
    return tg.step_grid64(c["grid"], c["start"], c["N"]) if c["family"] == "real_step" else tg.grid64(c["grid"], c["T"])


@pytest.mark.parametrize("method", list(kv.METHODS))
@pytest.mark.parametrize("family", tg.FIXED_FAMILIES)
def test_inputs_tell_a_neighbours_step_size_from_the_right_one(family, method, record_property):
    """real_step: the interval lengths are rotated (and made uniform) while the start states stay in place; its gradient is
    the one with respect to the start states."""
    kw = dict(roche=dict(ablate=False, grid="ragged", T=8), neural=dict(grid="ragged", T=8), real=dict(grid="ragged"),
              neural_real=dict(grid="ragged"), real_dims=dict(grid="ragged"), real_step=dict(N=7),
              neural_odd=dict(grid="ragged", T=8))[family]
    c = _first(family, method, **kw)
    solve = _solver(family, c)
    ref = solve()
    t = _grid64(c)
    gtol = NEURAL_REAL_GRAD_TOL if family == "neural_real" else GRAD_TOL
    gkey = "ginit" if family == "real_step" else "gy0"
    for what, wrong_t in (("rotated", tg.rotated(t)), ("uniform", tg.uniform_like(t))):
        assert wrong_t[0] == t[0] and abs(wrong_t[-1] - t[-1]) < 1e-12 and not np.array_equal(wrong_t, t)
        wrong = solve(wrong_t)
        dh, dg = _traj(wrong["h"], ref["h"]), _rel(wrong[gkey], ref[gkey]) / gtol
        record_property("%s_h_in_tolerances" % what, dh)
        record_property("%s_gy0_in_tolerances" % what, dg)
        assert dh >= 100 and dg >= 100, (what, dh, dg)


@pytest.mark.parametrize("method", list(kv.METHODS))
@pytest.mark.parametrize("grid", ["sub2", "sub3"])
def test_real_step_inputs_tell_a_wrong_table_row_from_the_right_one(grid, method, record_property):
    """Per-interval rows and the clipped last sub-step: the fp64 reference stepped along the table rows as they stand is the
    reference itself, bit for bit; with the last two entries of every row swapped (the clipped sub-step taken for a full
    one), with every interval on its neighbour's row shape (rotated lengths) and on the uniform grid it is >= 100 tolerances
    away in h and grad_init."""
    c = _first("real_step", method, grid=grid, N=7)
    p = tg.real_step_inputs(c)
    ref = tg.real_step_ref(c)
    rows = tg.real_step_rows(c).double()
    same = tg.real_step_solve_cpu(c, p, rows=rows)
    for k in ref:
        assert torch.equal(same[k], ref[k]), k
    swapped = rows.clone()
    swapped[:, -2], swapped[:, -1] = rows[:, -1], rows[:, -2]
    t = _grid64(c)
    wrongs = {"swapped": tg.real_step_solve_cpu(c, p, rows=swapped), "rotated": tg.real_step_solve_cpu(c, p, t=tg.rotated(t)),
              "uniform": tg.real_step_solve_cpu(c, p, t=tg.uniform_like(t))}
    for what, wrong in wrongs.items():
        dh, dg = _traj(wrong["h"], ref["h"]), _rel(wrong["ginit"], ref["ginit"]) / GRAD_TOL
        record_property("%s_h_in_tolerances" % what, dh)
        record_property("%s_ginit_in_tolerances" % what, dg)
        assert dh >= 100 and dg >= 100, (what, dh, dg)


# ---------------------------------------------------------------------------------------------------- 4. fp32 headroom
def _theta_ratio(g, r):
    g, r = g.double().flatten(), r.double().flatten()
    bound = 1e-4 * r.abs() + 1e-6 * r.norm()
    return float(((g - r).abs() / bound).max())


HEADROOM = 0.5


@pytest.mark.parametrize("family", tg.FIXED_FAMILIES)
def test_fp32_oracle_is_within_half_of_every_tolerance(family, record_property):
    """The fp32 CPU oracle against the fp64 one on every distinct fixed-grid problem of the table, in units of the GPU
    test's bounds (the uniform-grid table of tests/kernel_variants.py sits at 0.08).  Worst ratios measured: roche 0.153,
    neural 0.005, real 0.005, neural_real 0.006; the side libraries' families: real_dims 0.011, real_step 0.011 (one fp64
    and one fp32 oracle solve per interval), neural_odd 0.006."""
    worst, seen = 0.0, set()
    for c in tg.family(family):
        if family == "roche":
            key = (c["D"], c["ablate"], c["n_dose"], c["grid"], c["T"], c["method"], c["perturb"])
            if key in seen:
                continue
            p, ref = tg.roche_inputs(c), tg.roche_ref(c)
            f32 = tg.roche_solve_cpu(p, c["method"], c["perturb"], c["ablate"], dtype=torch.float32)
        elif family in ("neural", "neural_odd"):
            key = (c["D"], c["B"], c["T"], c["n_dose"], c["grid"], c["method"], c["perturb"])
            if key in seen:
                continue
            p = tg.neural_inputs(c)
            ref = tg.neural_solve_cpu(p, c["method"], c["perturb"])
            f32 = tg.neural_solve_cpu(p, c["method"], c["perturb"], dtype=torch.float32)
        elif family == "real_step":
            key = tg.case_id(c)
            p, ref = tg.real_step_inputs(c), tg.real_step_ref(c)
            f32 = tg.real_step_solve_cpu(c, p, dtype=torch.float32)
        elif family in ("real", "real_dims"):
            key = (c["D"], c["H"], c.get("B"), c["method"], c["perturb"], c["grid"])
            if key in seen:
                continue
            p, ref = tg.real_problem(c)
            f32 = tg.real_solve_cpu(c, p, dtype=torch.float32)
            again = tg.real_solve_cpu(c, p)  # the flat inputs rebuild the problem's own oracle
            assert torch.equal(again["h"], ref["h"]) and torch.equal(again["gw"], ref["gw"])
        else:
            key = tg.case_id(c)
            ref, f32 = tg.neural_real_solve_cpu(c)[0], tg.neural_real_solve_cpu(c, dtype=torch.float32)[0]
        seen.add(key)
        gtol = NEURAL_REAL_GRAD_TOL if family == "neural_real" else GRAD_TOL
        ratios = {"h": _traj(f32["h"], ref["h"])}
        for k in ref:
            if k == "h":
                continue
            assert torch.isfinite(ref[k]).all(), (tg.case_id(c), k)
            if float(ref[k].abs().max()) > 0:
                ratios[k] = _rel(f32[k], ref[k]) / gtol
        if family == "roche":
            ratios["gth_comp"] = _theta_ratio(f32["gth"], ref["gth"])
        bad = {k: v for k, v in ratios.items() if not v <= HEADROOM}
        assert not bad, (tg.case_id(c), bad)
        worst = max(worst, max(ratios.values()))
    record_property("worst_fp32_ratio", worst)
    print("fp32 headroom %s: worst ratio %.4f over %d problems" % (family, worst, len(seen)))


# --------------------------------------------------------------------------------------------------------- 5. coverage
def test_table_reaches_every_kernel_family_that_takes_a_grid():
    want = set(kv.FAMILIES) - set(tg.NO_GRID_FAMILIES)
    got = {kv.family(n) for c in tg.CASES for n in tg.kernels(c)}
    assert want <= got, sorted(want - got)
    assert set(tg.NO_GRID_FAMILIES) <= set(kv.FAMILIES)
    for fam in ("rk_fwd_kernel", "split_bwd_kernel", "mf_bwd_kernel", "neural_mf_bwd_kernel", "neural_bwd_kernel", "real_kernel",
                "real_mf_kernel", "neural_real_bwd_kernel", "dp_fwd_kernel", "dp_initbwd_kernel", "ndp_fwd_kernel",
                "ndp_initbwd_kernel"):
        assert fam in want, fam


def test_table_reaches_both_ring_depths_of_the_split_backward():
    """split_bwd_kernel<D, METHOD, ABLATE, NEED_TH, TAPE>: CW = TAPE selects the extra (c-) wave and with it the ring depth
    3 instead of 2 (csrc/hode_rk_split.hip); the tape pointer selects TAPE, and euler has none (kv.roche_fixed)."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hybrid-ode-neurips-2021_amd", "csrc",
                            "hode_rk_split.hip")).read()
    assert "constexpr bool CW = TAPE;" in src and "static constexpr int RD = CW ? 3 : 2;" in src
    seen = {}
    for c in tg.family("roche"):
        for n in tg.kernels(c):
            if kv.family(n) == "split_bwd_kernel":
                args = [x.strip() for x in n[n.index("<") + 1:n.rindex(">")].split(",")]
                seen.setdefault((int(args[1]), args[4]), set()).add(c["T"])
    for m in (kv.MIDPOINT, kv.RK4):
        for tape in ("true", "false"):
            assert seen.get((m, tape), set()) >= set(tg.SPLIT_TS), (m, tape, seen.get((m, tape)))
    assert seen[(kv.EULER, "false")] >= set(tg.SPLIT_TS) and (kv.EULER, "true") not in seen


def test_roche_table_covers_the_layouts_and_flags_the_grid_code_depends_on():
    cs = tg.family("roche")
    for lanes, dims, layout in tg.ROCHE_LAYOUTS:
        for method in kv.METHODS:
            mine = [c for c in cs if c["lanes"] == lanes and c["method"] == method]
            assert all(kv.roche_layout(c["D"], lanes, c["T"]) == layout and c["D"] in dims for c in mine)
            rag = [c for c in mine if c["grid"] == "ragged"]
            assert {c["T"] % 2 for c in rag} == {0, 1} and {c["perturb"] for c in rag} == {False, True}
            assert {"offset+", "offset-"} <= {c["grid"] for c in mine}
    for key in ("tape", "need_theta", "ablate"):
        assert {c[key] for c in cs} == {False, True}
    for method in kv.METHODS:
        for tape in (False, True):
            ts = {c["T"] for c in cs if c["lanes"] in (0, 48) and c["method"] == method and c["tape"] == tape
                  and c["grid"] == "ragged"}
            assert ts >= set(tg.SPLIT_TS), (method, tape, ts)


def test_other_tables_cover_what_the_issue_names():
    nc = tg.family("neural")
    for layout, onchip in (("mf", True), ("mf", False), ("lane", False)):
        for method in kv.METHODS:
            mine = [c for c in nc if c["layout"] == layout and c["onchip"] == onchip and c["method"] == method]
            assert {c["perturb"] for c in mine} == {False, True} and {c["grid"] for c in mine} == {"ragged", "offset-"}
    assert {c["T"] for c in nc} == {2, 5, 8}
    dc = tg.family("dopri5")
    assert {(c["D"], c["lanes"]) for c in dc} == {(c["D"], c["lanes"]) for c in kv.CASES if c["family"] == "dopri5"}
    for fam in ("dopri5", "neural_dopri5"):
        assert {(c["grid"], c["detach"]) for c in tg.family(fam)} == {(g, d) for g in ("clustered", "offset+") for d in (False, True)}
    assert {(c["method"], c["grid"]) for c in tg.family("real")} == {(m, g) for m in kv.METHODS for g in ("ragged", "offset+")}
    assert {(c["kind"], c["method"], c["grid"]) for c in tg.family("neural_real")} == {
        (k, m, g) for k in ("neural", "2nd") for m in kv.METHODS for g in ("ragged", "offset-")}
    names = {n.split("<")[0] for c in tg.family("real") for n in tg.kernels(c)}
    assert names == {"hode::real_kernel", "hode::real_mf_kernel", "hode::real_grad_fold_kernel"}
    assert any(n.endswith("true, false>") for c in tg.family("real") for n in tg.kernels(c))  # the tape-writing backward


def test_side_tables_reach_every_kernel_of_their_libraries():
    """libhode_real_dims.so, libhode_real_step.so and libhode_neural_odd.so, folds and the dose prelude included, by the
    libraries' own lists of kernel symbols (tests/*_cases.py expected_kernels, which their host tests hold to the objects)."""
    import neural_odd_cases
    import real_dims_cases
    import real_step_cases

    def reached(*families):
        return {n for f in families for c in tg.family(f) for n in tg.kernels(c)}

    assert reached("real_dims") == real_dims_cases.expected_kernels()
    assert reached("real_step") == real_step_cases.expected_kernels()
    assert reached("neural_odd", "neural_odd_dopri5") == neural_odd_cases.expected_kernels()
    assert tg.NEURAL_ODD_DIMS == neural_odd_cases.DIMS
    # the fixed-grid and the dopri5 table each reach their own kernels without the other's help, the shared fold aside
    fixed, dp = reached("neural_odd"), reached("neural_odd_dopri5")
    assert {n for n in neural_odd_cases.expected_kernels() if "neural_mf_" in n} <= fixed
    assert {n for n in neural_odd_cases.expected_kernels() if "ndp_" in n} <= dp


def test_side_tables_cover_what_the_issue_names():
    import real_dims_cases
    import real_step_cases
    rd = tg.family("real_dims")
    pairs = {(ht, m) for ht in real_dims_cases.HTS for m in kv.METHODS}
    for g in ("ragged", "offset+"):
        assert {(real_dims_cases.ht(c["H"]), c["method"]) for c in rd if c["grid"] == g} == pairs
    assert any(c["grid"] == "offset-" for c in rd) and {c["T"] for c in rd} == {tg.REAL_T}
    assert {c["D"] for c in rd} == {5, 7, 8, 9, 19} <= set(real_dims_cases.DIMS) and {c["B"] for c in rd} == {1, 17, 37}
    assert {c["H"] for c in rd} == {1, 16, 17, 43, 64}
    for m in kv.METHODS:
        assert {c["perturb"] for c in rd if c["method"] == m} == {False, True}, m
    rs = tg.family("real_step")
    assert {(real_step_cases.ht(c["H"]), c["method"]) for c in rs} == pairs
    assert {c["S"] for c in rs} == {1, 2, 3} and {c["N"] for c in rs} == {2, 7} and {c["B"] for c in rs} == {1, 17, 37}
    assert {c["D"] for c in rs} == {5, 8, 19, 20}
    assert {c["C"] for c in rs} >= {0, 1, 2, 3} and {c["C"] - c["N"] for c in rs} >= {0, 2}  # ..., N and N + 2
    assert {(c["grid"], c["start"]) for c in rs} == {(g, s) for g in tg.SUB_STEPS for s in tg.STEP_STARTS} == set(tg.STEP_TA)
    assert all(c["S"] == tg.SUB_STEPS[c["grid"]] <= real_step_cases.MAX_SUBSTEPS for c in rs)
    for m in kv.METHODS:
        assert {c["perturb"] for c in rs if c["method"] == m} == {False, True}, m
    chained = [c for c in rs if c["grid"] == "ragged"][:3]  # the cases held bit for bit to the chained kernels
    assert sorted(c["D"] <= 19 for c in chained) == [False, True, True] and {c["start"] for c in chained} == set(tg.STEP_STARTS)
    no = tg.family("neural_odd")
    for D in tg.NEURAL_ODD_DIMS:
        for m in kv.METHODS:
            assert {c["grid"] for c in no if c["D"] == D and c["method"] == m} == {"ragged", "offset-"}
    assert {c["T"] for c in no} == {2, 5, 8} and {c["B"] for c in no} == {17, 37, 65} and {c["n_dose"] for c in no} == {1, 3}
    for m in kv.METHODS:
        assert {c["perturb"] for c in no if c["method"] == m} == {False, True}, m
    nd = tg.family("neural_odd_dopri5")
    assert {(c["D"], c["detach"]) for c in nd} == {(D, d) for D in tg.NEURAL_ODD_DIMS for d in (False, True)}
    assert {(c["grid"], c["detach"]) for c in nd} == {(g, d) for g in ("clustered", "offset+") for d in (False, True)}
    assert {c["T"] for c in nd} == {tg.DOPRI5_T}


# -------------------------------------------------------------------------------- dopri5: the clustered grid's purpose
def test_clustered_grid_puts_several_outputs_in_one_accepted_step():
    """The free-running fp32 oracle on the clustered grid: an accepted step covers >= 3 output times and >= 2 cover none
    (the GPU test asserts the same from the kernel's own tape)."""
    from oracle.solvers import odeint as oracle_odeint
    from test_hip_kernel_variants import _roche_setup
    t = tg.grid("clustered", tg.DOPRI5_T)
    inp, f = _roche_setup(8, False, kv.DOPRI5_N, tg.DOPRI5_T, seed=48, t=t)
    f.set_action(inp["actions"])
    st = {}
    with torch.no_grad():
        oracle_odeint(f, inp["z0"], t, method="dopri5", rtol=1e-7, atol=1e-8, stats=st)
    counts = tg.outputs_per_step(st["tape"], t.double().numpy())
    assert max(counts) >= 3 and sum(1 for n in counts if n == 0) >= 2, counts
