"""The Sylvester flows on the device (libhode_sylvester.so: hode_sylvester_fwd / hode_sylvester_bwd through hode.sylvester and
flow.sylvester_chain) against the float64 restatement (tests/sylvester_eager.py): the case table of
tests/sylvester_cases.py forward and every gradient, the cotangent modes, the numerically special branches, bit-identical
repeats, sentinels around every buffer the library writes, refused descriptors, the presentations and cotangents autograd
hands the binding (tests/binding_cases.py's views; the wrapper lives in flow.py, outside that file's OPS table), and the
reference's numbers (G19) through the modules."""
import os

import numpy as np
import pytest
import torch

import binding_cases as bc
import flow
import sylvester_cases as cases
import sylvester_eager as se
from reference_checks import FLOW_GTOL as GTOL, FLOW_TOL as TOL, close as _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRADS = ("z0", "r1", "r2", "b", "q")
SMALL = cases._case("dense", 6, 6, 4, 51, 10)
SMALL_TRI = cases._case("tri", 5, 5, 3, 51, 10, "random")


def _args(ins, dev=DEV):
    return [None if ins[k] is None else ins[k].to(dev) for k in ("z0", "r1", "r2", "b", "q", "perm")]


def _objective(outs, ins, use, dev=DEV):
    obj = 0.0
    for out, key in zip(outs, ("gz", "gl", "gd")):
        if key in use:
            obj = obj + (out * ins[key].to(dev)).sum()
    return obj


def _device_run(ins, use=("gz", "gl", "gd")):
    """z_K, logdet, log_diag and the gradients of sum(outputs x cotangents in `use`), on the CPU."""
    args = _args(ins)
    leaves = [a.requires_grad_(True) for a in args[:5] if a is not None]
    outs = flow.sylvester_chain(*args, want_log_diag=True)
    obj = _objective(outs, ins, use)
    grads = torch.autograd.grad(obj, leaves, allow_unused=True) if torch.is_tensor(obj) else (None,) * len(leaves)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in outs], [g.cpu() for g in grads] + ([None] if ins["q"] is None else [])


def _reference(ins, use, idx=None):
    pick = lambda t, dim: t if (t is None or idx is None) else t.index_select(dim, idx)   # noqa: E731
    return se.forward_backward(pick(ins["z0"], 1), pick(ins["r1"], 0), pick(ins["r2"], 0), pick(ins["b"], 0), pick(ins["q"], 0),
                               ins["perm"], grad_z=pick(ins["gz"], 1) if "gz" in use else None,
                               grad_logdet=pick(ins["gl"], 1) if "gl" in use else None,
                               grad_log_diag=pick(ins["gd"], 1) if "gd" in use else None)


def _check(ins, use=("gz", "gl", "gd"), tol=TOL, gtol=GTOL, idx=None):
    outs, grads = _device_run(ins, use)
    rz, rl, rd, rgrads = _reference(ins, use, idx)
    if idx is not None:   # large B: the fp64 yardstick on a subset of patients (each patient's sums are its own)
        outs = [o.index_select(1, idx) for o in outs]
        grads = [None if g is None else g.index_select(1 if n == "z0" else 0, idx) for n, g in zip(GRADS, grads)]
    for n, got, ref in zip(("z_K", "logdet", "log_diag"), outs, (rz, rl, rd)):
        assert got.shape == ref.shape and got.dtype == torch.float32, n
        _close(got, ref, tol, n)
    for n, got, ref in zip(GRADS, grads, rgrads):
        assert (got is None) == (ref is None), n
        if got is not None:
            assert got.shape == ref.shape, n
            _close(got, ref, gtol, "grad_" + n)
    return outs, grads


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_kernel_against_fp64(case):
    _check(cases.inputs(case), idx=cases.subset(case["B"]))


@pytest.mark.parametrize("case", [SMALL, SMALL_TRI], ids=cases.case_id)
@pytest.mark.parametrize("use", [("gz",), ("gl",), ("gd",), ("gz", "gl", "gd")], ids=["z", "logdet", "log_diag", "all"])
def test_cotangent_modes(case, use):
    _check(cases.inputs(case), use=use)


def test_no_cotangent_launches_no_backward(monkeypatch):
    import hode.sylvester as hs
    ins = cases.inputs(SMALL)
    args = _args(ins)
    leaves = [a.requires_grad_(True) for a in args[:5]]
    outs = flow.sylvester_chain(*args, want_log_diag=True)
    other = torch.ones(3, device=DEV, requires_grad=True)
    monkeypatch.setattr(hs, "sylvester_backward", lambda *a, **k: pytest.fail("the backward was launched"))
    grads = torch.autograd.grad((other * 2).sum() + 0 * len(outs), leaves + [other], allow_unused=True)
    assert all(g is None for g in grads[:5]) and torch.equal(grads[5].cpu(), torch.full((3,), 2.0))
    # and a forward that needs no gradient asks for no tape
    with torch.no_grad():
        z, logdet = flow.sylvester_chain(*_args(ins))
    torch.cuda.synchronize()
    assert torch.equal(z.cpu(), outs[0].detach().cpu()) and torch.equal(logdet.cpu(), outs[1].detach().cpu())


# ------------------------------------------------------------------------------------------------ special branches
def test_saturated_tanh():
    for case in (SMALL, SMALL_TRI):
        ins = cases.inputs(case, seed=12)
        ins["b"] = ins["b"] + 40.0 * torch.sign(ins["b"])   # |a| ~ 40: tanh = +-1, 1 - tanh^2 = 0
        _check(ins)


def test_jacobian_term_near_zero_and_negative():
    """1 + (1 - h^2) r1_mm r2_mm down to 7e-3 and below zero: the sign under |.| and the 1 / g of its derivative.  The
    looser bounds are test_hip_flow.test_near_zero_jacobian_term's, for the same reason: g itself is a difference of
    two numbers near 1, so its float32 rounding (6e-8) is relative 1e-5 of g and of everything divided by it."""
    ins = cases.inputs(cases._case("dense", 6, 6, 1, 50, 7), seed=13)
    ins["z0"] = 1e-3 * ins["z0"]
    ins["b"] = torch.zeros_like(ins["b"])           # a ~ 0: h ~ 0, 1 - h^2 ~ 1
    eye = torch.eye(6, dtype=torch.bool)
    target = torch.tensor([-0.993, -1.5, -0.95, -3.0, -1.02, 0.5])   # g ~ 0.007, -0.5, 0.05, -2, -0.02, 1.5
    ins["r1"] = torch.where(eye, torch.ones(()), ins["r1"])
    ins["r2"] = torch.where(eye, torch.diag_embed(target.expand(7, 1, 6)), ins["r2"])
    outs, _ = _check(ins, tol=1e-3, gtol=1e-2)
    ref = se.forward(*(None if t is None else t.double() for t in (ins["z0"], ins["r1"], ins["r2"], ins["b"], ins["q"])))[2]
    assert torch.isfinite(outs[2]).all() and (ref[..., 0] < -4).all() and (ref[..., 3] > 0.6).all()


def test_one_ortho_vector():
    for D in (3, 32):
        _check(cases.inputs(cases._case("dense", D, 1, 2, 5, 3)))


def test_identity_row_inside_perm():
    ins = cases.inputs(cases._case("tri", 5, 5, 3, 7, 4, "random"), seed=5)
    ins["perm"][1] = torch.arange(5)
    assert not torch.equal(ins["perm"][0], torch.arange(5))
    _check(ins)


def test_non_involutive_perm_is_a_forward_gather():
    """The device follows the reference's second gather: with a 5-cycle the inverse scatter gives another z."""
    ins = cases.inputs(cases._case("tri", 5, 5, 1, 3, 2, "random"), seed=6)
    p = torch.tensor([[2, 0, 3, 4, 1]])
    ins["perm"] = p
    outs, _ = _check(ins)
    z0, r1, r2, b = (ins[k].double() for k in ("z0", "r1", "r2", "b"))
    w = torch.einsum("sbm,bjm->sbj", torch.tanh(torch.einsum("sbj,bmj->sbm", z0[..., p[0]], r2[:, 0]) + b[:, 0]), r1[:, 0])
    inverse = z0.clone()
    inverse[..., p[0]] += w
    assert (outs[0].double() - inverse).abs().max() > 1e-2


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("case", [SMALL, SMALL_TRI, cases.CASES[-1]], ids=cases.case_id)
def test_bit_identical_repeats(case):
    assert cases.CASES[-1]["B"] == cases.BIG_B
    ins = cases.inputs(case, seed=21)
    o1, g1 = _device_run(ins)
    o2, g2 = _device_run(ins)
    for a, b in zip(o1 + g1, o2 + g2):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------------------ raw descriptors: sentinels, refusals
SENTINEL, PAD = -777.25, 64


class _Guarded:
    """A device buffer of n floats between two PAD-float guard zones, all filled with SENTINEL."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def body(self):
        return self.buf[PAD:PAD + self.n]

    def guards_intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _raw_desc(ins, args):
    from hode import _sylvester_lib as SL
    S, B, D = ins["z0"].shape
    K, M = ins["r1"].shape[1], ins["r1"].shape[2]
    d = SL.new_desc()
    d.batch, d.latent_dim, d.n_ortho, d.n_flows, d.n_samples = B, D, M, K, S
    d.z0, d.r1, d.r2, d.b = (a.data_ptr() for a in args[:4])
    d.q = 0 if args[4] is None else args[4].data_ptr()
    d.perm = 0 if args[5] is None else args[5].data_ptr()
    return d, (S, B, D, M, K)


def _raw_buffers(lib, d, dims, dense):
    S, B, D, M, K = dims
    sizes = {"z_out": S * B * D, "logdet": S * B, "log_diag": S * B * K * M, "workspace": lib.hode_sylvester_workspace_bytes(d) // 4,
             "grad_z0": S * B * D, "grad_r1": B * K * M * M, "grad_r2": B * K * M * M, "grad_b": B * K * M}
    if dense:
        sizes["grad_q"] = B * K * D * M
    bufs = {k: _Guarded(n) for k, n in sizes.items()}
    for k, g in bufs.items():
        setattr(d, k, g.ptr)
    d.workspace_bytes = 4 * sizes["workspace"]
    return bufs


@pytest.mark.parametrize("case", [cases._case("dense", 5, 3, 3, 5, 7), cases._case("tri", 9, 9, 2, 65, 3, "random"),
                                  cases._case("dense", 17, 9, 2, 3, 5), cases._case("dense", 4, 4, 1, 1, 1)], ids=cases.case_id)
def test_sentinels_around_every_buffer(case):
    """The library's own writes, through raw descriptors: every output, gradient and the tape sit between guard zones that
    stay intact, every element inside is written, and the values are the wrapper's bit for bit."""
    from hode import _sylvester_lib as SL
    from hode.solver import _f32c, _i32c
    lib = SL.lib()
    ins = cases.inputs(case)
    args = [None if a is None else _f32c(a) for a in _args(ins)[:5]] + [None if ins["perm"] is None else _i32c(ins["perm"].to(DEV), "perm")]
    cots = [ins[k].to(DEV) for k in ("gz", "gl", "gd")]
    d, dims = _raw_desc(ins, args)
    bufs = _raw_buffers(lib, d, dims, case["mode"] == "dense")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.hode_sylvester_fwd(d, stream) == 0, lib.hode_sylvester_last_error_string()
    d.grad_z_out, d.grad_logdet, d.grad_log_diag = (c.data_ptr() for c in cots)
    assert lib.hode_sylvester_bwd(d, stream) == 0, lib.hode_sylvester_last_error_string()
    torch.cuda.synchronize()
    for name, g in bufs.items():
        assert g.guards_intact(), name
        if name == "workspace":   # the tape: (K - 1) S B D floats, then padding up to 256 bytes that nobody writes
            used = (dims[4] - 1) * dims[0] * dims[1] * dims[2]
            assert bool((g.body()[:used] != SENTINEL).all()) and bool((g.body()[used:] == SENTINEL).all())
        else:
            assert bool((g.body() != SENTINEL).all()), name
    outs, grads = _device_run(ins)
    for name, ref in zip(("z_out", "logdet", "log_diag"), outs):
        assert torch.equal(bufs[name].body().cpu().reshape(ref.shape), ref), name
    for name, ref in zip(GRADS, grads):
        if ref is not None:
            assert torch.equal(bufs["grad_" + name].body().cpu().reshape(ref.shape), ref), name


def test_refused_descriptors_leave_the_outputs_untouched():
    from hode import _sylvester_lib as SL
    lib = SL.lib()
    ins = cases.inputs(cases._case("dense", 6, 4, 3, 5, 7))
    args = _args(ins)
    assert all(a is None or a.is_contiguous() for a in args)
    gz = ins["gz"].to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    refusals = (({"n_flows": 17}, SL.E_SIZE), ({"n_samples": 257}, SL.E_SIZE), ({"latent_dim": 33}, SL.E_SIZE),
                ({"n_ortho": 0}, SL.E_SIZE), ({"batch": 0}, SL.E_SIZE), ({"struct_size": 8}, SL.E_SIZE), ({"q": 0}, SL.E_SIZE),
                ({"z0": 0}, SL.E_NULL), ({"workspace_bytes": 16}, SL.E_WORKSPACE), ({"perm": args[0].data_ptr()}, SL.E_SIZE))
    for change, code in refusals:
        d, dims = _raw_desc(ins, args)
        bufs = _raw_buffers(lib, d, dims, True)
        d.grad_z_out = gz.data_ptr()
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.hode_sylvester_fwd(d, stream) == code, (change, lib.hode_sylvester_last_error_string())
        assert lib.hode_sylvester_bwd(d, stream) == code, (change, lib.hode_sylvester_last_error_string())
        torch.cuda.synchronize()
        assert all(g.untouched() for g in bufs.values()), change
    d, dims = _raw_desc(ins, args)   # a backward without the tape, and a forward without its required outputs
    bufs = _raw_buffers(lib, d, dims, True)
    d.workspace = 0
    assert lib.hode_sylvester_bwd(d, stream) == SL.E_WORKSPACE
    d.z_out = 0
    assert lib.hode_sylvester_fwd(d, stream) == SL.E_NULL
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs.values())


def test_domain_refused_on_device():
    from hode import HodeConfigError
    ins = cases.inputs(SMALL)
    z0, r1, r2, b, q, _ = _args(ins)
    with pytest.raises(HodeConfigError, match="n_samples 257"):
        flow.sylvester_chain(torch.zeros(257, 10, 6, device=DEV), r1, r2, b, q)
    with pytest.raises(HodeConfigError, match="n_flows 17"):
        flow.sylvester_chain(z0, r1.repeat(1, 5, 1, 1)[:, :17], r2.repeat(1, 5, 1, 1)[:, :17], b.repeat(1, 5, 1)[:, :17], q.repeat(1, 5, 1, 1)[:, :17])
    with pytest.raises(HodeConfigError, match="latent_dim 33"):
        flow.sylvester_chain(torch.zeros(3, 10, 33, device=DEV), r1, r2, b, torch.zeros(10, 4, 33, 6, device=DEV))
    with pytest.raises(HodeConfigError, match="triangular mode"):
        flow.sylvester_chain(torch.zeros(3, 10, 7, device=DEV), r1, r2, b)
    with pytest.raises(HodeConfigError, match="perm belongs to triangular mode"):
        flow.sylvester_chain(z0, r1, r2, b, q, torch.arange(6).repeat(4, 1))
    with pytest.raises(HodeConfigError, match="perm entries must lie in 0..5"):
        flow.sylvester_chain(z0, r1, r2, b, None, torch.arange(1, 7).repeat(4, 1))
    with pytest.raises(HodeConfigError, match="integer tensor"):
        flow.sylvester_chain(z0, r1, r2, b, None, torch.arange(6.0).repeat(4, 1))
    with pytest.raises(HodeConfigError, match="shapes"):
        flow.sylvester_chain(z0, r1, r2[:, :3], b, q)


# ------------------------------------------------------------------------------------------- the binding contract
# flow._SylvesterChain lives outside hode/, so tests/binding_cases.py has no OPS entry for it; the same presentations are
# fed here.  `_OP` stands in for the entry where binding_cases.present() asks which inputs may be expanded.
class _OP:
    expand = ("z0",)


def _plain(ins, use=("gz", "gl", "gd")):
    return _device_run(ins, use)


def _presented(ins, pres):
    """Outputs and gradients with every float input in presentation `pres`."""
    plain = dict(ins)
    if pres == "expanded":   # draws constant along S: a stride-0 expand against the same values laid out densely
        plain["z0"] = ins["z0"][:1].expand(ins["z0"].shape).contiguous()
    views = {k: bc.present(_OP, pres, k, plain[k], DEV) for k in ("z0", "r1", "r2", "b", "q")}
    for k, v in views.items():
        if v is not None and pres in ("offset4", "offset8"):
            assert v.data_ptr() % 16 == (4 if pres == "offset4" else 8), k
        if v is not None and pres == "strided" and v.numel() > v.shape[-1]:
            assert not v.is_contiguous(), k
    leaves = [v.requires_grad_(True) for v in views.values() if v is not None]
    perm = None if ins["perm"] is None else ins["perm"].to(DEV)
    outs = flow.sylvester_chain(views["z0"], views["r1"], views["r2"], views["b"], views["q"], perm, want_log_diag=True)
    grads = torch.autograd.grad(_objective(outs, ins, ("gz", "gl", "gd")), leaves)
    torch.cuda.synchronize()
    for g, leaf in zip(grads, leaves):
        assert g.dtype == leaf.dtype and g.shape == leaf.shape
    return [o.detach().float().cpu() for o in outs], [g.float().cpu() for g in grads] + ([None] if ins["q"] is None else []), plain


@pytest.mark.parametrize("case", [SMALL, SMALL_TRI], ids=cases.case_id)
@pytest.mark.parametrize("pres", ["offset4", "offset8", "strided", "expanded", "fp64"])
def test_input_presentations(case, pres):
    """Offset, strided, expanded and float64 inputs: against float64, and bit for bit against the plain call (float32
    values throughout: a float64 presentation carries the same numbers)."""
    ins = cases.inputs(case, seed=31)
    outs, grads, plain = _presented(ins, pres)
    ref_outs, ref_grads = _check(plain)
    for a, b in zip(outs + grads, ref_outs + ref_grads):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("case", [SMALL, SMALL_TRI], ids=cases.case_id)
def test_cotangents_autograd_really_produces(case):
    """Expanded (sum), non-contiguous (transpose), offset (stack / cat halves), float64 and absent cotangents."""
    ins = cases.inputs(case, seed=32)
    ref_outs, ref_grads = _check(dict(ins, gz=torch.ones_like(ins["gz"]), gl=torch.ones_like(ins["gl"])), use=("gz", "gl"))

    def run(objective):
        args = _args(ins)
        leaves = [a.requires_grad_(True) for a in args[:5] if a is not None]
        outs = flow.sylvester_chain(*args, want_log_diag=True)
        grads = torch.autograd.grad(objective(*outs), leaves, allow_unused=True)
        torch.cuda.synchronize()
        return [g.cpu() for g in grads] + ([None] if ins["q"] is None else [])

    # .sum() hands the backward stride-0 expanded cotangents; log_diag's is absent (None)
    same = lambda got: all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, ref_grads))   # noqa: E731
    assert same(run(lambda z, ld, dg: z.sum() + ld.sum()))
    # through a transpose: a non-contiguous cotangent with the same values
    assert same(run(lambda z, ld, dg: z.transpose(0, 1).contiguous().sum() + ld.t().sum()))
    # stack / cat: each output is one half of a larger gradient buffer, at an offset
    assert same(run(lambda z, ld, dg: torch.stack([z, z.detach()]).sum() + torch.cat([ld.detach(), ld]).sum()))
    # a float64 consumer
    assert same(run(lambda z, ld, dg: z.double().sum() + ld.double().sum()))
    # one cotangent only: the others arrive as None
    only_z = run(lambda z, ld, dg: z.sum())
    _, want = _check(dict(ins, gz=torch.ones_like(ins["gz"])), use=("gz",))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(only_z, want))


def test_side_stream_and_interleaved_calls():
    ins, other = cases.inputs(SMALL, seed=33), cases.inputs(SMALL_TRI, seed=34)
    ref_outs, ref_grads = _check(ins)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        args = _args(ins)
        leaves = [a.requires_grad_(True) for a in args[:5]]
        outs = flow.sylvester_chain(*args, want_log_diag=True)
        o_args = _args(other)   # a second call between this forward and its backward: the tapes are per call
        o_leaves = [a.requires_grad_(True) for a in o_args[:4]]
        o_outs = flow.sylvester_chain(*o_args, want_log_diag=True)
        grads = torch.autograd.grad(_objective(outs, ins, ("gz", "gl", "gd")), leaves)
        o_grads = torch.autograd.grad(_objective(o_outs, other, ("gz", "gl", "gd")), o_leaves)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip([o.detach().cpu() for o in outs] + [g.cpu() for g in grads], ref_outs + ref_grads):
        assert torch.equal(a, b)
    want_outs, want_grads = _device_run(other)
    for a, b in zip([o.detach().cpu() for o in o_outs] + [g.cpu() for g in o_grads], want_outs + want_grads[:4]):
        assert torch.equal(a, b)


def test_one_gradient_at_a_time_and_no_grad():
    ins = cases.inputs(SMALL, seed=35)
    ref_outs, ref_grads = _device_run(ins)
    for i in range(5):
        args = _args(ins)
        args[i].requires_grad_(True)
        outs = flow.sylvester_chain(*args, want_log_diag=True)
        g, = torch.autograd.grad(_objective(outs, ins, ("gz", "gl", "gd")), [args[i]])
        assert torch.equal(g.cpu(), ref_grads[i]), GRADS[i]
    with torch.no_grad():
        outs = flow.sylvester_chain(*_args(ins), want_log_diag=True)
    assert not any(o.requires_grad for o in outs) and all(torch.equal(o.cpu(), r) for o, r in zip(outs, ref_outs))


# ------------------------------------------------------------------------------------------------------------ G19
@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_sylvester.npz"), allow_pickle=False)


def _rec(g, name):
    pre = "f32_%s_" % name
    return {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("name", ["syl_sum", "syl_terms", "tri_none", "tri_flip", "tri_perm", "tri_quirk"])
def test_g19_modules_on_device(g19, name):
    """The modules on HIP tensors (the kernel at K = 1, S = 1) give the reference's outputs and gradients."""
    r = _rec(g19, name)
    dense = name.startswith("syl")
    names = ("zk", "r1", "r2", "q", "b") if dense else ("zk", "r1", "r2", "b")
    leaves = [r["in_" + n].to(DEV).requires_grad_(True) for n in names]
    if dense:
        z, ldj = flow.Sylvester(4).to(DEV)(*leaves, name == "syl_sum")
    else:
        tri, perm = flow.TriangularSylvester(5).to(DEV), (r["perm"].to(DEV) if "perm" in r else None)
        z, ldj = tri(*leaves, perm, True) if name == "tri_quirk" else tri._forward(*leaves, perm, name != "tri_flip")
    assert z.shape == r["z"].shape and ldj.shape == r["ldj"].shape and z.is_cuda
    grads = torch.autograd.grad((z * r["gz"].to(DEV)).sum() + (ldj * r["gl"].to(DEV)).sum(), leaves)
    torch.cuda.synchronize()
    _close(z.detach().cpu(), r["z"], TOL, "z")
    _close(ldj.detach().cpu(), r["ldj"], TOL, "ldj")
    for n, g in zip(names, grads):
        assert g.shape == r["grad_" + n].shape, n
        _close(g.cpu(), r["grad_" + n], GTOL, "grad_" + n)


def test_g19_chain_equals_three_module_calls_bit_for_bit(g19):
    """A K = 3 chain against three module calls on the device.  The kernel forms every flow's A, C and diagonal products
    by the same prologue whatever K is and hands z from flow to flow as float32 (through the tape), exactly what three
    K = 1 launches do: z_3 and the per-flow log_diag terms are equal bit for bit.  logdet is the kernel's running sum over
    the flows, the three calls' terms added on the host in the same order: equal too."""
    r = _rec(g19, "chain3")
    zk, r1, r2, q, b = (r["in_" + n].to(DEV) for n in ("zk", "r1", "r2", "q", "b"))
    z, logdet, log_diag = flow.sylvester_chain(zk.unsqueeze(0), r1, r2, b, q, want_log_diag=True)
    syl = flow.Sylvester(4).to(DEV)
    step, terms, sums = zk, [], []
    for k in range(3):
        prev = step
        step, t = syl(prev, r1[:, k], r2[:, k], q[:, k], b[:, k].unsqueeze(1), False)
        terms.append(t)
        sums.append(syl(prev, r1[:, k], r2[:, k], q[:, k], b[:, k].unsqueeze(1), True)[1])
    torch.cuda.synchronize()
    assert torch.equal(z[0], step) and torch.equal(log_diag[0], torch.stack(terms, dim=1))
    assert torch.equal(logdet[0], (sums[0] + sums[1]) + sums[2])
    _close(z[0].cpu(), r["z"], TOL, "z")
    _close(log_diag[0].cpu(), r["ldj"], TOL, "log_diag")
