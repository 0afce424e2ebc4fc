"""The Sylvester-flow posterior on the device (libhode_snf.so: hode_snf_fwd / hode_snf_bwd through hode.snf and
flow.sylvester_posterior_sample) against the float64 restatement (tests/snf_eager.py): the case table of
tests/snf_cases.py forward and every gradient, the composed path (the sylvester_chain kernel plus torch ops), the
cotangent modes, saturated inputs, bit-identical repeats, sentinels around every buffer the library writes, refused
descriptors, the presentations and cotangents autograd hands the binding (tests/binding_cases.py's views; the wrapper
lives in flow.py, outside that file's OPS table), and the model-level paths with model.EncoderSylvesterLSTM."""
import numpy as np
import pytest
import torch

import binding_cases as bc
import flow
import model
import snf_cases as cases
import snf_eager as se
from oracle.solvers import odeint as oracle_odeint
from reference_checks import FLOW_GTOL as GTOL, FLOW_TOL as TOL, close as _close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = cases.HEADS
SMALL_TRI = cases._case("tri", 6, 4, 51, 10)
SMALL_HH = cases._case("hh", 6, 4, 51, 10, 3)
SMALLS = [SMALL_TRI, SMALL_HH]


def _heads(ins, dev=DEV):
    return [None if ins[k] is None else ins[k].to(dev) for k in HEADS]


def _objective(outs, ins, use, dev=DEV):
    obj = 0.0
    for out, key in zip(outs, ("gz", "gk")):
        if key in use:
            obj = obj + (out * ins[key].to(dev)).sum()
    return obj


def _device_run(ins, use=("gz", "gk")):
    """z_out, kl and the gradients of sum(outputs x cotangents in `use`) for the seven heads, on the CPU."""
    heads = _heads(ins)
    leaves = [h.requires_grad_(True) for h in heads if h is not None]
    outs = flow.sylvester_posterior_sample(*heads, ins["noise"].to(DEV), ins["s_kl"])
    obj = _objective(outs, ins, use)
    grads = torch.autograd.grad(obj, leaves, allow_unused=True) if torch.is_tensor(obj) else (None,) * len(leaves)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in outs], [g.cpu() for g in grads] + ([None] if ins["v"] is None else [])


def _reference(ins, use, idx=None, dtype=torch.float64):
    pick = lambda t, dim: t if (t is None or idx is None) else t.index_select(dim, idx)   # noqa: E731
    return se.forward_backward(*(pick(ins[k], 0) for k in HEADS), pick(ins["noise"], 1), ins["s_kl"],
                               grad_z=pick(ins["gz"], 1) if "gz" in use else None,
                               grad_kl=pick(ins["gk"], 0) if "gk" in use else None, dtype=dtype)


def _compare(outs, grads, ref, tol, gtol):
    rz, rk, rgrads = ref
    for n, got, want in zip(("z_out", "kl"), outs, (rz, rk)):
        assert got.shape == want.shape and got.dtype == torch.float32, n
        _close(got, want, tol, n)
    # A gradient that is identically zero (v at D = 1, where Q = +-1 whatever v is) comes out of the float64 yardstick as
    # its own rounding noise, ~1e-16 of the terms that cancel; relative to that noise no bound means anything.  (The same
    # holds for a raw diagonal of +-20, whose 1 - tanh^2 = 1.7e-17 float64 autograd rounds to exactly 0.)  Entries below
    # 1e-12 of the case's largest gradient are the yardstick's error: there the kernel must be as small.
    floor = 1e-12 * max(r.abs().max().item() for r in rgrads if r is not None)
    for n, got, want in zip(HEADS, grads, rgrads):
        assert (got is None) == (want is None), n
        if got is not None:
            assert got.shape == want.shape, n
            if want.abs().max().item() < floor:
                assert torch.isfinite(got).all() and got.abs().max().item() <= gtol * floor, "grad_" + n
            else:
                _close(got, want, gtol, "grad_" + n)


def _check(ins, use=("gz", "gk"), tol=TOL, gtol=GTOL, idx=None):
    outs, grads = _device_run(ins, use)
    sel_outs, sel_grads = outs, grads
    if idx is not None:   # large B: the fp64 yardstick on a subset of patients (each patient's sums are its own)
        sel_outs = [outs[0].index_select(1, idx), outs[1].index_select(0, idx)]
        sel_grads = [None if g is None else g.index_select(0, idx) for g in grads]
    _compare(sel_outs, sel_grads, _reference(ins, use, idx), tol, gtol)
    return outs, grads


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_kernel_against_fp64(case):
    tol, gtol = cases.OWN_BOUNDS.get(cases.case_id(case), (TOL, GTOL))
    _check(cases.inputs(case), tol=tol, gtol=gtol, idx=cases.subset(case["B"]))


def _composed(heads, noise, s_kl):
    """The posterior from what libhode_sylvester.so offers: torch ops around the sylvester_chain kernel."""
    mu, log_var, full_d, diag1, diag2, bias, v = heads
    r1, r2, q, perm = flow.sylvester_flow_parameters(full_d, diag1, diag2, v)
    sigma = torch.exp(0.5 * log_var)
    z0 = noise * sigma + mu
    z, logdet = flow.sylvester_chain(z0, r1, r2, bias, q, perm)
    z_out = torch.exp(z - 5.0)
    log_q = model.GaussianReparam.log_density(mu, log_var, z0) - logdet - torch.sum(z - 5.0, dim=-1)
    return z_out, torch.mean((log_q - model.ExponentialPrior.log_density(z_out))[s_kl:], dim=0)


@pytest.mark.parametrize("case", SMALLS, ids=cases.case_id)
def test_composed_path_holds_the_same_bounds(case):
    """The same inputs through the sylvester_chain kernel and torch ops: the same float64 numbers within the same bounds,
    so the two device paths are interchangeable."""
    ins = cases.inputs(case, seed=3)
    heads = _heads(ins)
    leaves = [h.requires_grad_(True) for h in heads if h is not None]
    outs = _composed(heads, ins["noise"].to(DEV), ins["s_kl"])
    grads = torch.autograd.grad(_objective(outs, ins, ("gz", "gk")), leaves)
    torch.cuda.synchronize()
    grads = [g.cpu() for g in grads] + ([None] if ins["v"] is None else [])
    _compare([o.detach().cpu() for o in outs], grads, _reference(ins, ("gz", "gk")), TOL, GTOL)
    _check(ins)


# ------------------------------------------------------------------------------------------------ cotangent modes
@pytest.mark.parametrize("case", SMALLS, ids=cases.case_id)
@pytest.mark.parametrize("use", [("gk",), ("gz",), ("gz", "gk")], ids=["kl", "z", "both"])
def test_cotangent_modes(case, use):
    _check(cases.inputs(case), use=use)


def test_no_cotangent_launches_no_backward(monkeypatch):
    import hode.snf as hs
    ins = cases.inputs(SMALL_HH)
    heads = _heads(ins)
    leaves = [h.requires_grad_(True) for h in heads]
    outs = flow.sylvester_posterior_sample(*heads, ins["noise"].to(DEV), 1)
    other = torch.ones(3, device=DEV, requires_grad=True)
    monkeypatch.setattr(hs, "snf_backward", lambda *a, **k: pytest.fail("the backward was launched"))
    grads = torch.autograd.grad((other * 2).sum() + 0 * len(outs), leaves + [other], allow_unused=True)
    assert all(g is None for g in grads[:7]) and torch.equal(grads[7].cpu(), torch.full((3,), 2.0))
    with torch.no_grad():   # and without z_out
        none, kl = flow.sylvester_posterior_sample(*_heads(ins), ins["noise"].to(DEV), 1, want_z=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(kl.cpu(), outs[1].detach().cpu())


# ------------------------------------------------------------------------------------------------ saturated inputs
def test_saturated_tanh_in_the_flow():
    for case in SMALLS:
        ins = cases.inputs(case, seed=12)
        ins["bias"] = ins["bias"] + 40.0 * torch.sign(ins["bias"])   # |a| ~ 40: tanh = +-1, 1 - tanh^2 = 0
        _check(ins)


@pytest.mark.parametrize("which", ["diag1", "diag2"])
def test_saturated_diagonals_have_finite_tiny_gradients(which):
    """Raw +-20: tanh is +-1 in float32 and 1 - tanh^2 = 4 e^-40 / (1 + e^-40)^2 ~ 1.7e-17, which the kernels form from
    the exponential, not as 1 - t^2 = 0: the gradient is tiny and right, not zero.  In float64 tanh(20) is 1 too and
    autograd's 1 - t^2 is exactly 0, so here the yardstick is the float64 gradient for the diagonal of r1 / r2 itself times
    the closed form of 1 - tanh^2 (the table check holds these entries to its floor, see _compare)."""
    e = torch.exp(torch.tensor(-40.0, dtype=torch.float64))
    sech2 = (4.0 * e / (1.0 + e) ** 2).item()
    for case in SMALLS:
        ins = cases.inputs(case, seed=13)
        ins[which] = 20.0 * torch.sign(ins[which])
        outs, grads = _check(ins)
        g = grads[HEADS.index(which)]
        assert torch.isfinite(g).all() and 0 < g.abs().max() < 1e-12
        h64 = {k: None if ins[k] is None else ins[k].double() for k in HEADS}
        r1, r2, q = se.parameters(h64["full_d"], h64["diag1"], h64["diag2"], h64["v"])
        r1, r2 = r1.requires_grad_(True), r2.requires_grad_(True)
        z_out, kl, _, _ = se.posterior(h64["mu"], h64["log_var"], r1, r2, q, h64["bias"], ins["noise"].double(), ins["s_kl"])
        obj = (z_out * ins["gz"].double()).sum() + (kl * ins["gk"].double()).sum()
        g_r, = torch.autograd.grad(obj, [r1 if which == "diag1" else r2])
        _close(g, torch.diagonal(g_r, dim1=-2, dim2=-1) * sech2, GTOL, "grad_" + which)   # tiny, and right


def test_large_and_tiny_householder_vectors():
    """Q depends on the direction of v only: |v| ~ 1e18 and |v| ~ 1e-20 give the same draws, and gradients of size
    1 / |v| that stay finite (the norm is taken after scaling by max|v|)."""
    ins = cases.inputs(SMALL_HH, seed=14)
    base, _ = _device_run(ins)
    for scale in (1e18, 1e-20):
        scaled = dict(ins, v=ins["v"] * scale)
        outs, grads = _check(scaled)
        assert all(torch.isfinite(g).all() for g in grads)
        _close(outs[0], base[0], 1e-5, "z_out under a rescaled v")
        assert grads[6].abs().max() > 0


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("case", SMALLS + [cases.CASES[-1]], ids=cases.case_id)
def test_bit_identical_repeats(case):
    assert cases.CASES[-1]["B"] == cases.BIG_B
    ins = cases.inputs(case, seed=21)
    o1, g1 = _device_run(ins)
    o2, g2 = _device_run(ins)
    for a, b in zip(o1 + g1, o2 + g2):
        assert (a is None and b is None) or torch.equal(a, b)


def test_backward_may_be_repeated_on_one_forward():
    """The backward writes only the cotangent part of the workspace: a second backward of the same graph gives the same bits."""
    ins = cases.inputs(SMALL_HH, seed=22)
    heads = _heads(ins)
    leaves = [h.requires_grad_(True) for h in heads]
    outs = flow.sylvester_posterior_sample(*heads, ins["noise"].to(DEV), 1)
    obj = _objective(outs, ins, ("gz", "gk"))
    g1 = torch.autograd.grad(obj, leaves, retain_graph=True)
    g2 = torch.autograd.grad(obj, leaves)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


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


def _raw_desc(ins, heads, noise):
    from hode import _snf_lib as NL
    S, B, D = ins["noise"].shape
    K, H = ins["full_d"].shape[1], (0 if ins["v"] is None else ins["v"].shape[2])
    d = NL.new_desc()
    d.batch, d.latent_dim, d.n_flows, d.n_samples, d.s_kl, d.n_householder = B, D, K, S, ins["s_kl"], H
    for name, h in zip(HEADS, heads):
        setattr(d, name, 0 if h is None else h.data_ptr())
    d.noise = noise.data_ptr()
    return d, (S, B, D, K, H)


def _raw_buffers(lib, d, dims):
    S, B, D, K, H = dims
    sizes = {"z_out": S * B * D, "kl": B, "workspace": lib.hode_snf_workspace_bytes(d) // 4, "grad_mu": B * D, "grad_log_var": B * D,
             "grad_full_d": B * K * D * D, "grad_diag1": B * K * D, "grad_diag2": B * K * D, "grad_bias": B * K * D}
    if H:
        sizes["grad_v"] = B * K * H * D
    bufs = {k: _Guarded(n) for k, n in sizes.items()}
    for k, g in bufs.items():
        setattr(d, k, g.ptr)
    d.workspace_bytes = 4 * sizes["workspace"]
    return bufs


@pytest.mark.parametrize("case", [cases._case("hh", 5, 3, 5, 7, 2), cases._case("tri", 9, 2, 65, 3), cases._case("hh", 17, 2, 3, 5, 8),
                                  cases._case("tri", 4, 1, 1, 1)], ids=cases.case_id)
def test_sentinels_around_every_buffer(case):
    """The library's own writes, through raw descriptors: every output, gradient and the workspace sit between guard zones
    that stay intact, every element inside is written, and the values are the wrapper's bit for bit."""
    from hode import _snf_lib as NL
    from hode.solver import _f32c
    lib = NL.lib()
    ins = cases.inputs(case)
    heads = [None if h is None else _f32c(h) for h in _heads(ins)]
    noise, gz, gk = (_f32c(ins[k].to(DEV)) for k in ("noise", "gz", "gk"))
    d, dims = _raw_desc(ins, heads, noise)
    bufs = _raw_buffers(lib, d, dims)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.hode_snf_fwd(d, stream) == 0, lib.hode_snf_last_error_string()
    torch.cuda.synchronize()
    S, B, D, K, H = dims
    tape = (K + 1) * S * B * D
    ws = bufs["workspace"].body()
    assert bool((ws[:tape] != SENTINEL).all()) and bool((ws[tape:] == SENTINEL).all())   # the forward writes z_0 .. z_K only
    d.grad_z_out, d.grad_kl = gz.data_ptr(), gk.data_ptr()
    assert lib.hode_snf_bwd(d, stream) == 0, lib.hode_snf_last_error_string()
    torch.cuda.synchronize()
    for name, g in bufs.items():
        assert g.guards_intact(), name
        if name == "workspace":   # (K + 2) S B D floats, then padding up to 256 bytes that nobody writes
            used = (K + 2) * S * B * D
            assert bool((g.body()[:used] != SENTINEL).all()) and bool((g.body()[used:] == SENTINEL).all())
        else:
            assert bool((g.body() != SENTINEL).all()), name
    outs, grads = _device_run(ins)
    for name, ref in zip(("z_out", "kl"), outs):
        assert torch.equal(bufs[name].body().cpu().reshape(ref.shape), ref), name
    for name, ref in zip(("mu", "log_var", "full_d", "diag1", "diag2", "bias", "v"), grads):
        if ref is not None:
            assert torch.equal(bufs["grad_" + name].body().cpu().reshape(ref.shape), ref), name


def test_refused_descriptors_leave_the_outputs_untouched():
    from hode import _snf_lib as NL
    lib = NL.lib()
    ins = cases.inputs(cases._case("hh", 6, 3, 5, 7, 2))
    heads = _heads(ins)
    noise, gz = ins["noise"].to(DEV), ins["gz"].to(DEV)
    assert all(h.is_contiguous() for h in heads)
    stream = torch.cuda.current_stream().cuda_stream
    refusals = (({"n_flows": 17}, NL.E_SIZE), ({"n_samples": 257}, NL.E_SIZE), ({"latent_dim": 33}, NL.E_SIZE),
                ({"n_householder": 9}, NL.E_SIZE), ({"n_householder": -1}, NL.E_SIZE), ({"batch": 0}, NL.E_SIZE),
                ({"struct_size": 8}, NL.E_SIZE), ({"s_kl": 5}, NL.E_SIZE), ({"s_kl": -1}, NL.E_SIZE), ({"v": 0}, NL.E_NULL),
                ({"mu": 0}, NL.E_NULL), ({"noise": 0}, NL.E_NULL), ({"workspace_bytes": 16}, NL.E_WORKSPACE),
                ({"workspace": 0}, NL.E_WORKSPACE))
    for change, code in refusals:
        d, dims = _raw_desc(ins, heads, noise)
        bufs = _raw_buffers(lib, d, dims)
        d.grad_z_out = gz.data_ptr()
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.hode_snf_fwd(d, stream) == code, (change, lib.hode_snf_last_error_string())
        assert lib.hode_snf_bwd(d, stream) == code, (change, lib.hode_snf_last_error_string())
        torch.cuda.synchronize()
        assert all(g.untouched() for g in bufs.values()), change
    d, dims = _raw_desc(ins, heads, noise)   # a misaligned workspace, a forward without kl, a backward without grad_v
    bufs = _raw_buffers(lib, d, dims)
    d.workspace = bufs["workspace"].ptr + 4
    assert lib.hode_snf_fwd(d, stream) == NL.E_WORKSPACE and lib.hode_snf_bwd(d, stream) == NL.E_WORKSPACE
    d.workspace, d.kl, d.grad_v = bufs["workspace"].ptr, 0, 0
    assert lib.hode_snf_fwd(d, stream) == NL.E_NULL and lib.hode_snf_bwd(d, stream) == NL.E_NULL
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs.values())


def test_domain_refused_on_device():
    from hode import HodeConfigError
    ins = cases.inputs(SMALL_HH)
    mu, lv, fd, d1, d2, b, v = _heads(ins)
    noise = ins["noise"].to(DEV)
    with pytest.raises(HodeConfigError, match="n_samples 257"):
        flow.sylvester_posterior_sample(mu, lv, fd, d1, d2, b, v, torch.zeros(257, 10, 6, device=DEV))
    with pytest.raises(HodeConfigError, match="s_kl"):
        flow.sylvester_posterior_sample(mu, lv, fd, d1, d2, b, v, noise[:1], s_kl=1)
    with pytest.raises(HodeConfigError, match="n_householder 9"):
        flow.sylvester_posterior_sample(mu, lv, fd, d1, d2, b, v.repeat(1, 1, 3, 1), noise)
    with pytest.raises(HodeConfigError, match="n_flows 17"):
        flow.sylvester_posterior_sample(mu, lv, fd.repeat(1, 5, 1, 1)[:, :17], d1.repeat(1, 5, 1)[:, :17], d2.repeat(1, 5, 1)[:, :17],
                                        b.repeat(1, 5, 1)[:, :17], None, noise)
    with pytest.raises(HodeConfigError, match="shapes"):
        flow.sylvester_posterior_sample(mu, lv, fd, d1, d2[:, :3], b, v, noise)


# ------------------------------------------------------------------------------------------- the binding contract
# flow._SylvesterPosterior lives outside hode/, so tests/binding_cases.py has no OPS entry for it; the same presentations are
# fed here.  `_OP` stands in for the entry where binding_cases.present() asks which inputs may be expanded.
class _OP:
    expand = ("noise",)


def _presented(ins, pres):
    """Outputs and gradients with every float input in presentation `pres`."""
    plain = dict(ins)
    if pres == "expanded":   # draws constant along S: a stride-0 expand against the same values laid out densely
        plain["noise"] = ins["noise"][:1].expand(ins["noise"].shape).contiguous()
    views = {k: bc.present(_OP, pres, k, plain[k], DEV) for k in HEADS + ("noise",)}
    for k, v in views.items():
        if v is not None and pres in ("offset4", "offset8"):
            assert v.data_ptr() % 16 == (4 if pres == "offset4" else 8), k
        if v is not None and pres == "strided" and v.numel() > v.shape[-1]:
            assert not v.is_contiguous(), k
    leaves = [views[k].requires_grad_(True) for k in HEADS if views[k] is not None]
    outs = flow.sylvester_posterior_sample(*(views[k] for k in HEADS), views["noise"], ins["s_kl"])
    grads = torch.autograd.grad(_objective(outs, ins, ("gz", "gk")), leaves)
    torch.cuda.synchronize()
    for g, leaf in zip(grads, leaves):
        assert g.dtype == leaf.dtype and g.shape == leaf.shape
    return [o.detach().float().cpu() for o in outs], [g.float().cpu() for g in grads] + ([None] if ins["v"] is None else []), plain


@pytest.mark.parametrize("case", SMALLS, ids=cases.case_id)
@pytest.mark.parametrize("pres", ["offset4", "offset8", "strided", "expanded", "fp64"])
def test_input_presentations(case, pres):
    """Offset, strided, expanded and float64 inputs: against float64, and bit for bit against the plain call (float32
    values throughout: a float64 presentation carries the same numbers)."""
    ins = cases.inputs(case, seed=31)
    outs, grads, plain = _presented(ins, pres)
    ref_outs, ref_grads = _check(plain)
    for a, b in zip(outs + grads, ref_outs + ref_grads):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("case", SMALLS, ids=cases.case_id)
def test_cotangents_autograd_really_produces(case):
    """Expanded (sum), non-contiguous (transpose), offset (stack / cat halves), float64 and absent cotangents."""
    ins = cases.inputs(case, seed=32)
    _, ref_grads = _check(dict(ins, gz=torch.ones_like(ins["gz"]), gk=torch.ones_like(ins["gk"])))

    def run(objective):
        heads = _heads(ins)
        leaves = [h.requires_grad_(True) for h in heads if h is not None]
        outs = flow.sylvester_posterior_sample(*heads, ins["noise"].to(DEV), ins["s_kl"])
        grads = torch.autograd.grad(objective(*outs), leaves, allow_unused=True)
        torch.cuda.synchronize()
        return [g.cpu() for g in grads] + ([None] if ins["v"] is None else [])

    same = lambda got, want=ref_grads: all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, want))   # noqa: E731
    assert same(run(lambda z, kl: z.sum() + kl.sum()))                                        # stride-0 expanded
    assert same(run(lambda z, kl: z.transpose(0, 1).contiguous().sum() + kl.sum()))
    assert same(run(lambda z, kl: torch.stack([z, z.detach()]).sum() + torch.cat([kl.detach(), kl]).sum()))   # at an offset
    assert same(run(lambda z, kl: z.double().sum() + kl.double().sum()))
    only_kl = run(lambda z, kl: kl.sum())                                                      # grad_z arrives as None
    _, want = _check(dict(ins, gk=torch.ones_like(ins["gk"])), use=("gk",))
    assert same(only_kl, want)


def test_side_stream_and_interleaved_calls():
    ins, other = cases.inputs(SMALL_HH, seed=33), cases.inputs(SMALL_TRI, seed=34)
    ref_outs, ref_grads = _check(ins)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        heads = _heads(ins)
        leaves = [h.requires_grad_(True) for h in heads]
        outs = flow.sylvester_posterior_sample(*heads, ins["noise"].to(DEV), 1)
        o_heads = _heads(other)   # a second call between this forward and its backward: the workspaces are per call
        o_leaves = [h.requires_grad_(True) for h in o_heads[:6]]
        o_outs = flow.sylvester_posterior_sample(*o_heads, other["noise"].to(DEV), 1)
        grads = torch.autograd.grad(_objective(outs, ins, ("gz", "gk")), leaves)
        o_grads = torch.autograd.grad(_objective(o_outs, other, ("gz", "gk")), o_leaves)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip([o.detach().cpu() for o in outs] + [g.cpu() for g in grads], ref_outs + ref_grads):
        assert torch.equal(a, b)
    want_outs, want_grads = _device_run(other)
    for a, b in zip([o.detach().cpu() for o in o_outs] + [g.cpu() for g in o_grads], want_outs + want_grads[:6]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- model-level paths
OBS, ACT, HIDDEN, STEP = 20, 1, 40, 0.5


def _vi_pair(flow_type, mc, seed=5, normalize=False):
    """The same weights on the device (float32) and on the CPU in float64 with the oracle solver."""
    torch.manual_seed(seed)
    cpu = torch.device("cpu")
    enc = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 4, flow_type=flow_type, num_householder=3, normalize=normalize, device=DEV)
    dec = model.RocheExpertDecoder(OBS, 6, ACT, 14 * STEP, STEP, roche=True, method="rk4", device=DEV)
    enc_c = model.EncoderSylvesterLSTM(OBS + ACT, HIDDEN, 6, 4, flow_type=flow_type, num_householder=3, normalize=normalize, device=cpu)
    dec_c = model.RocheExpertDecoder(OBS, 6, ACT, 14 * STEP, STEP, roche=True, method="rk4", device=cpu)
    dec_c._odeint = oracle_odeint
    enc_c.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    dec_c.load_state_dict({k: v.cpu() for k, v in dec.state_dict().items()})
    enc_c.double()
    dec_c.double()
    prior = model.ExponentialPrior.log_density
    return (model.VariationalInferenceFlow(enc, dec, prior_log_pdf=prior, mc_size=mc),
            model.VariationalInferenceFlow(enc_c, dec_c, prior_log_pdf=prior, mc_size=mc))


@pytest.mark.parametrize("flow_type", model.EncoderSylvesterLSTM.FLOW_TYPES)
def test_loss_and_backward_against_the_float64_cpu_run(flow_type):
    """B 10, D 6, K 4, mc_size 50.  Bounds: those of test_hip_flow.test_loss_and_backward_against_cpu_mirror (loss 1e-3,
    gradients 1e-2 of the largest entry): the LSTM and solver kernels in front of and behind the posterior set them."""
    vi, vi_c = _vi_pair(flow_type, 50)
    B, T = 10, 15
    g = torch.Generator().manual_seed(3)
    x = 0.5 * torch.randn(T, B, OBS, generator=g)
    a = torch.zeros(T, B, 1)
    a[torch.randint(0, T - 1, (B,), generator=g), torch.arange(B), 0] = torch.rand(B, generator=g) * 10
    m = (torch.rand(T, B, OBS, generator=g) < 0.5).float()
    noise = 0.5 * torch.randn(51, B, 6, generator=g)
    vi.noise = lambda n, like: noise[:n].to(DEV)
    vi_c.noise = lambda n, like: noise[:n].double()
    loss = vi.loss({"measurements": x.to(DEV), "actions": a.to(DEV), "masks": m.to(DEV)})
    loss.backward()
    loss_c = vi_c.loss({"measurements": x.double(), "actions": a.double(), "masks": m.double()})
    loss_c.backward()
    assert loss_c.dtype == torch.float64
    np.testing.assert_allclose(loss.item(), loss_c.item(), rtol=1e-3)
    for (n, p), (_, pc) in zip(list(vi.encoder.named_parameters()) + list(vi.decoder.named_parameters()),
                               list(vi_c.encoder.named_parameters()) + list(vi_c.decoder.named_parameters())):
        got = p.grad.cpu().double() if p.grad is not None else torch.zeros_like(pc)
        ref = pc.grad if pc.grad is not None else torch.zeros_like(pc)
        fin = torch.isfinite(ref)   # the decoder's Hill-exponent gradients can be NaN in the CPU run itself: not compared
        assert n.startswith("ode.") or fin.all(), n
        assert torch.isfinite(got[fin]).all(), n
        if fin.any():
            assert (got[fin] - ref[fin]).abs().max().item() <= 1e-2 * (ref[fin].abs().max().item() + 1e-6), n


@pytest.mark.parametrize("flow_type", model.EncoderSylvesterLSTM.FLOW_TYPES)
def test_training_loop_and_evaluate_flow(flow_type, tmp_path, capsys):
    import training_utils
    from hode.batches import DeviceFolds
    vi, _ = _vi_pair(flow_type, 50, seed=9, normalize=True)   # the encoder's default: latents in the solver's range
    folds = DeviceFolds.synthetic(60, 15, OBS, 6, 10, 20, DEV, seed=4, step=STEP)
    params = list(vi.encoder.parameters()) + list(vi.decoder.output_function.parameters()) + list(vi.decoder.ode.ml_net.parameters())
    before = [p.detach().clone() for p in vi.encoder.parameters()]
    vi, best, _ = training_utils.variational_training_loop(2, folds, vi, 10, torch.optim.Adam(params, lr=1e-3), 1,
                                                           path=str(tmp_path) + "/")
    assert np.isfinite(best) and best < 1e9
    assert all(not torch.equal(p.detach(), q) for p, q in zip(vi.encoder.parameters(), before))   # every head was reached
    capsys.readouterr()
    out = training_utils.evaluate_flow(vi, folds, 10, 5, mc_itr=50)
    lines = capsys.readouterr().out.splitlines()
    assert [line.split(",")[0] for line in lines[-4:]] == ["rmse_z0", "rmse_x", "cprs_z0", "cprs_x"]
    assert len(out) == 6 and all(np.isfinite(v) for v in out)
