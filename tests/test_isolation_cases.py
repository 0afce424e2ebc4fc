"""Guard (no GPU) of tests/isolation_cases.py, the table tests/test_hip_isolation.py runs: every compiled forward, backward
and fold of the real-data and recurrent families -- in libhode.so, libhode_real_dims.so, libhode_real_step.so and
libhode_lstm_seq.so -- is named by a case of the main table; and the expected answer of every poisoned run is pinned to the
family's float64 reference, not to the kernels: the reference turns exactly the poisoned patient non-finite (main table) or
saturates back to finite values (SATURATING), every other patient keeps the bits of the clean run, and a poisoned cotangent
reaches what isolation_cases.cot_reaches says.  A condition, checked here; it is not a tolerance."""
import pytest
import torch

import build_hip
import isolation_cases as ic
import kernel_variants as kv
from test_kernel_variant_coverage import compiled_kernel_names


@pytest.mark.parametrize("lib", sorted(ic.FAMILIES))
def test_every_compiled_kernel_of_the_families_is_named_by_a_case(lib):
    """Every `.kd` symbol of the listed families is launched by a case of the main table (the readouts: of READOUT_CASES):
    a new instantiation that no case names fails here."""
    compiled = {n for n in compiled_kernel_names(build_hip.LIBRARIES[lib].obj) if ic.base(n) in ic.FAMILIES[lib]}
    named = {k for c in ic.CASES + ic.READOUT_CASES if ic.library(c) == lib for k in ic.kernels(c)}
    assert {ic.base(n) for n in compiled} == set(ic.FAMILIES[lib])
    assert named <= compiled, sorted(named - compiled)
    missing = sorted(compiled - named)
    assert not missing, "%d compiled kernels no isolation case names:\n  %s" % (len(missing), "\n  ".join(missing))


def test_the_table_is_well_formed():
    every = ic.CASES + ic.SATURATING + ic.READOUT_CASES
    ids = [ic.case_id(c) for c in every]
    assert len(ids) == len(set(ids))
    groups = {}
    for c in every:
        assert 0 <= c["row"] < c["B"] and c["value"] in ic.VALUE_NAMES and 0 <= c["n"] < c["T"], c
        key, idx = ic.forward_target(c)
        assert ic.setup(c)[key][idx].numel() == 1 and key not in ("idx", "tau", "t", "w", "theta", "wflat"), c   # data, never a table or a weight
        groups.setdefault((c["family"].replace("_mlp", ""), c.get("kind"), c.get("lib")), []).append(c)   # both readouts: one group
    for key, cs in groups.items():   # every axis value reaches every family, the shape edges and the sharp cases included
        assert {c["value"] for c in cs} == set(ic.VALUE_NAMES), key
        if key[0] == "lstm":
            assert all(c["B"] % (16 * c["nt"]) == 2 for c in cs), key   # the last workgroup of every patient tile is ragged
            assert {c["T"] for c in cs} == {1, 2, 6} and {c["reverse"] for c in cs} == {0, 1}, key
            assert {c["what"] for c in cs} == set(ic.LSTM_WHATS) and {c["B"] - c["row"] for c in cs} >= {1, 2}, key
            assert any(c.get("sharp") and c["row"] == c["B"] - 2 and c["col"] == 0 and c["what"] == "x1" for c in cs), key
        else:
            assert {c["B"] for c in cs} == {5, 50}, key
            assert {c["T"] for c in cs} == ({2, 3, 6} if key[0] == "real_step" else {1, 2, 6}), key
            assert {c["row"] for c in cs if c["B"] == 50} == {0, 15, 16, 47, 48, 49}, key
            assert any(c.get("sharp") and (c["row"], c["col"]) == (48, 0) for c in cs), key
            assert any(c.get("sharp") and c["row"] == 49 for c in cs), key
        if key[0] not in ("readout", "readout_mlp"):
            assert {c["n"] for c in cs if c["T"] == 6} == {0, 3, 5}, key
    for c in ic.CASES + ic.SATURATING:
        if c["family"] == "seqdec" and c["what"] == "a":   # a row that idx really reads
            assert ic.forward_target(c)[1][0] in ic.setup(c)["idx"].tolist()
    assert {c["what"] for c in ic.READOUT_CASES} == set(ic.READOUT_WHATS)
    # position invariance: every family, both LSTM libraries at every patient tile
    fams = {(c["family"], c.get("kind"), c.get("lib")) for c in ic.POSITION_CASES}
    assert fams == {k for k in groups if k[0] != "readout"}
    assert {(c["lib"], c["nt"]) for c in ic.POSITION_CASES if c["family"] == "lstm"} == {(l, n) for l in ("final", "seq") for n in (1, 2, 3, 4)}
    assert all(c["B"] == 50 and c["T"] == 6 for c in ic.POSITION_CASES)


def test_saturating_is_not_empty_and_holds_padded_hidden_sizes():
    lstm = [c for c in ic.SATURATING if c["family"] == "lstm"]
    assert lstm and {c["lib"] for c in lstm} == {"final", "seq"}
    assert {c["H"] for c in lstm} >= {44, 75} and all(c["H"] not in kv.LSTM_SIZES for c in lstm)
    assert all(c["value"] in ("+inf", "-inf") and c["what"] in ("x1", "a") for c in lstm)
    assert {16 * ((c["H"] + 15) // 16) for c in lstm} == set(kv.LSTM_SIZES)   # padded units at every compiled size


def _others(c):
    keep = torch.ones(c["B"], dtype=torch.bool)
    keep[c["row"]] = False
    return keep.nonzero().flatten()


def _n_bad(xs):
    return sum(int((~torch.isfinite(x)).sum()) for x in xs)


@pytest.mark.parametrize("c", ic.CASES + ic.SATURATING, ids=ic.case_id)
def test_float64_reference_on_the_poisoned_inputs(c):
    """Forward: the clean run is finite; poisoned, every other patient has the bits of the clean run at every output, and the
    poisoned patient is non-finite (main table: in its last output row -- for the one-step-ahead solve the row of the
    poisoned interval, for an action the row of the step that reads it) or finite everywhere (SATURATING).  Adjoint: a
    poisoned cotangent leaves every other patient's gradient bits, and reaches what ic.cot_reaches says."""
    p = ic.setup(c)
    has_cot = c["family"] != "lstm" or c["tape"]
    clean = ic.reference(c, p, p["cot"] if has_cot else None)
    bad = ic.reference(c, ic.poisoned(c))
    others = _others(c)
    for k in ("h", "c"):
        if k in clean:
            ax = ic.out_axis(c, k)
            assert bool(torch.isfinite(clean[k]).all())
            assert torch.equal(bad[k].index_select(ax, others), clean[k].index_select(ax, others)), k
    rows = ic.bad_rows(c, bad)
    if c in ic.SATURATING:
        assert not any(bool(v.any()) for v in rows.values()), rows
    else:
        h_rows = rows["h"]
        if h_rows.dim() == 0:
            assert bool(h_rows)
        elif c["family"] == "real_step":
            want = torch.zeros(c["T"], dtype=torch.bool)
            want[c["interval"] + 1] = True
            assert torch.equal(h_rows, want)
        elif c["family"] == "seqdec" and c["kind"] == "gruode" and c["what"] == "a":
            assert bool(h_rows[c["k"]]) and int(h_rows.sum()) == 1   # no recurrence: the row of the step that reads the action
        else:
            last = (0 if c["reverse"] else c["T"] - 1) if c["family"] == "lstm" else c["T"] - 1
            assert bool(h_rows[last])
    if not has_cot:
        return
    got = ic.reference(c, p, ic.poisoned_cot(c))
    reaches = ic.cot_reaches(c)
    assert _n_bad(clean["summed"]) == 0
    if clean["pp"] is not None:
        ax = ic.out_axis(c, "grad_y0")
        assert torch.equal(got["pp"].index_select(ax, others), clean["pp"].index_select(ax, others))
        mine = got["pp"].select(ax, c["row"])
        assert bool(torch.isfinite(mine).all()) == (reaches == "nothing")
    if reaches == "steps":
        assert _n_bad(got["summed"]) > 0   # the poisoned patient's term is summed, not dropped
    else:
        assert all(torch.equal(a, b) for a, b in zip(got["summed"], clean["summed"]))


@pytest.mark.parametrize("c", ic.READOUT_CASES, ids=ic.case_id)
def test_float64_readout_on_the_poisoned_inputs(c):
    """The loss and the parameter gradients are sums over every (time, patient) row: non-finite; grad_h keeps its bits in
    every other row and is non-finite in the poisoned one -- behind mask 0 as well: (x - x_hat)^2 * mask is a product."""
    p = ic.setup(c)
    clean, bad = ic.readout_reference(c, p), ic.readout_reference(c, ic.poisoned(c))
    assert bool(torch.isfinite(clean["lik"])) and _n_bad([clean["grad_h"]] + clean["summed"]) == 0
    assert not bool(torch.isfinite(bad["lik"])) and all(_n_bad([g]) > 0 for g in bad["summed"])
    keep = torch.ones(c["T"], c["B"], dtype=torch.bool)
    keep[c["n"], c["row"]] = False
    assert torch.equal(bad["grad_h"][keep], clean["grad_h"][keep])
    assert not bool(torch.isfinite(bad["grad_h"][c["n"], c["row"]]).all())
