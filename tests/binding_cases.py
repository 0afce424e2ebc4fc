"""The layer above the kernels: what the autograd functions and plain launchers of ``hode/`` accept.  A plain helper
module, not a conftest.

* OPS: one entry per binding -- a small ragged shape, a builder of plain inputs (fresh, contiguous, fp32, from a seeded
  CPU generator), the call, and the float64 reference of the same operation (oracle/, tests/seqdec_eager.py,
  tests/neural_real_eager.py, tests/flow_eager.py, oracle.vi's densities in the reference's MC-KL loop).
* PRESENTATIONS: equivalent calls -- the same values somewhere else in memory (offset, strided, expanded, fp64), the
  output consumed another way (cot_*), another set of inputs requiring a gradient, two backwards, two interleaved calls,
  a side stream, mistyped index tables, an input changed between forward and backward.
* INAPPLICABLE[(op, presentation)] = why the pair cannot exist.
* DETERMINISTIC: ops whose results are bit-identical from run to run, so the presented call must equal the plain call
  bit for bit.

tests/test_hip_binding_contract.py (GPU) runs OPS x PRESENTATIONS minus INAPPLICABLE; tests/test_binding_case_coverage.py
(no GPU) checks the table against the source of hode/ and the presentation builders against the normalising helper.

Shapes: D = 6 with B = 5 and T = 15 for the Roche / NeuralODE / linear-readout entries (T B D = 450 floats: one solve's
share of a stacked cotangent starts 8 bytes off a 16-byte boundary, a dropped first row B D = 30 floats likewise);
obs = 20 for the LSTM (obs % 4 == 0 selects the VEC4 kernels); D = 20, H = 16 for `real` (the matrix-core path)."""
import collections

import torch

DOPRI5_RTOL, DOPRI5_ATOL = 1e-7, 1e-8         # tests/test_hip_kernel_variants.py test_dopri5_backward
NEURAL_DOPRI5_RTOL, NEURAL_DOPRI5_ATOL = 1e-6, 1e-8  # tests/test_hip_kernel_variants.py test_neural_dopri5
MCKL_RATE, MCKL_CLAMP = 100.0, float(torch.finfo(torch.float32).eps)


# ---------------------------------------------------------------------------------------------------- plain inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _roche_inputs(seed, D=6, B=5, T=15):
    from hode import synth
    from oracle.rhs import THETA_DEFAULT, dose_schedule
    g = _gen(seed)
    inp = synth.solver_inputs(B, T, D, seed=seed)
    dosage, times = dose_schedule(inp["actions"], synth.STEP)
    theta = torch.zeros(16)
    theta[:13] = torch.tensor(THETA_DEFAULT)
    return collections.OrderedDict(y0=inp["z0"], theta=theta, w=torch.randn(D - 4, D, generator=g) * 0.6,
                                   b=torch.randn(D - 4, generator=g) * 0.1, t=inp["t"], dosage=dosage,
                                   dose_times=times.to(torch.float32))


def _mlp(g, n_in, n_hid, n_out, scale=1.0):
    return (torch.randn(n_hid, n_in, generator=g) * scale / n_in ** 0.5, torch.randn(n_hid, generator=g) * 0.1,
            torch.randn(n_out, n_hid, generator=g) * scale / n_hid ** 0.5, torch.randn(n_out, generator=g) * 0.1)


def _neural_inputs(seed, D=6, B=5, T=15, step=0.375, y_scale=0.5):
    g = _gen(seed)
    w1, b1, w2, b2 = _mlp(g, D + 1, 10 * D, D, 2.0)
    t = torch.arange(T, dtype=torch.float32) * step
    return collections.OrderedDict(y0=torch.randn(B, D, generator=g) * y_scale, w1=w1, b1=b1, w2=w2, b2=b2, t=t,
                                   dosage=0.5 + torch.rand(B, generator=g) * 2,
                                   dose_times=t[torch.randint(0, T, (B, 1), generator=g)].clone())


def _neural_dopri5_inputs(seed):
    from hode import synth
    return _neural_inputs(seed, step=synth.STEP, y_scale=1.0)


def _real_inputs(seed, D=20, H=16, B=5, Ta=12, t0=4):
    g = _gen(seed)
    M = D - 4
    wflat = torch.randn(9 * H + 2 + 3 * M * M, generator=g) * 0.3
    return collections.OrderedDict(y0=torch.randn(B, D, generator=g) * 0.3, theta=torch.tensor([1.0, 0.2, 0.2]),
                                   wflat=wflat, t=torch.arange(t0 - 1, Ta, 1, dtype=torch.float32),
                                   act=(torch.rand(Ta, B, generator=g) < 0.2).float() * torch.rand(Ta, B, generator=g))


def _neural_real_inputs(seed, D=6, H=16, B=5, Ta=7, t0=3, t_end=9, m_out=None):
    g = _gen(seed)
    w1, b1, w2, b2 = _mlp(g, D + 1, H, D if m_out is None else m_out)
    return collections.OrderedDict(y0=torch.randn(B, D, generator=g) * 0.5, w1=w1, b1=b1, w2=w2, b2=b2,
                                   t=torch.arange(t0 - 1, t_end, 1.0),
                                   a=(torch.rand(Ta, B, 1, generator=g) < 0.4).float() * torch.rand(Ta, B, 1, generator=g) * 2)


def _neural_real_2nd_inputs(seed):
    return _neural_real_inputs(seed, m_out=3)


def _seqdec_common(g, D, B, Ta, t0):
    rows = list(range(t0 + 1, Ta))  # T' = Ta - t0 - 1 steps
    idx = torch.tensor(rows, dtype=torch.int32)
    tau = torch.ones(len(rows), dtype=torch.float32) * idx.to(torch.float32) / Ta
    a = (torch.rand(Ta, B, 1, generator=g) < 0.3).float() * torch.rand(Ta, B, 1, generator=g) * 2
    return torch.randn(B, D, generator=g) * 0.5, a, idx, tau


def _tlstm_inputs(seed, D=6, B=5, Ta=20, t0=8):
    g = _gen(seed)
    init, a, idx, tau = _seqdec_common(g, D, B, Ta, t0)
    k = 1.0 / D ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731  (nn.LSTM's init range)
    return collections.OrderedDict(init=init, w_ih=u(4 * D, 2), w_hh=u(4 * D, D), b_ih=u(4 * D), b_hh=u(4 * D), a=a, idx=idx,
                                   tau=tau)


def _gruode_inputs(seed, D=6, B=5, Ta=20, t0=8):
    g = _gen(seed)
    init, a, idx, tau = _seqdec_common(g, D, B, Ta, t0)
    return collections.OrderedDict(init=init, w_z=torch.randn(D + 2, D + 2, generator=g) * 0.4,
                                   w_n=torch.randn(D, D + 2, generator=g) * 0.4, a=a, idx=idx, tau=tau)


def _lstm_inputs(seed, T=7, B=5, obs=20, H=13):
    g = _gen(seed)
    k = 1.5 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    return collections.OrderedDict(
        w_ih=u(4 * H, obs + 1), w_hh=u(4 * H, H), b_ih=u(4 * H), b_hh=u(4 * H), x=torch.randn(T, B, obs, generator=g),
        a=torch.rand(T, B, 1, generator=g) * (torch.rand(T, B, 1, generator=g) < 0.3).float(),
        mask=(torch.rand(T, B, obs, generator=g) < 0.5).float())


def _readout_inputs(seed, D=6, obs=20, T=15, B=5):
    g = _gen(seed)
    return collections.OrderedDict(
        h=torch.randn(T, B, D, generator=g), w=torch.randn(obs, D, generator=g) / D ** 0.5, b=torch.randn(obs, generator=g) * 0.1,
        x=torch.randn(T, B, obs, generator=g),
        mask=torch.rand(T, B, obs, generator=g) * (torch.rand(T, B, obs, generator=g) < 0.6).float())


def _readout_mlp_inputs(seed, D=20, obs=24, T=7, B=5, skip=1):
    g = _gen(seed)
    w1, b1, w2, b2 = _mlp(g, D, D + 1, obs)
    return collections.OrderedDict(
        h=torch.randn(T + skip, B, D, generator=g), w1=w1, b1=b1, w2=w2, b2=b2, x=torch.randn(T, B, obs, generator=g),
        mask=(torch.rand(T, B, obs, generator=g) < 0.5).float(), time_weight=0.5 + torch.rand(T, generator=g))


def _mckl_inputs(seed, B=5, D=6, S=7):
    g = _gen(seed)
    return collections.OrderedDict(mu=torch.randn(B, D, generator=g) * 0.02 + 0.01, log_var=torch.randn(B, D, generator=g) * 0.5 - 8.0,
                                   noise=torch.randn(S, B, D, generator=g))


def _flow_inputs(seed, B=5, D=6, K=4, S=15):
    g = _gen(seed)
    w = torch.randn(B, K, D, generator=g)
    w = w / w.norm(dim=-1, keepdim=True) * (0.5 + 0.5 * torch.rand(B, K, 1, generator=g))
    return collections.OrderedDict(mu=0.3 * torch.randn(B, D, generator=g), log_var=-1.0 + 0.3 * torch.randn(B, D, generator=g),
                                   u=0.5 * torch.randn(B, K, D, generator=g), w=w, b=0.3 * torch.randn(B, K, generator=g),
                                   noise=torch.randn(S, B, D, generator=g))


CRPS_MEMBERS = 4


def _crps_inputs(seed, Tn=3, B=5, M=CRPS_MEMBERS, Dv=6, obs=4):
    g = _gen(seed)
    return collections.OrderedDict(h=torch.randn(Tn, M * B, Dv, generator=g), truth=torch.randn(Tn, B, obs, generator=g) * 2,
                                   weight=torch.randn(obs, Dv, generator=g) * 0.5, bias=torch.randn(obs, generator=g))


# ---------------------------------------------------------------------------------------------------- the calls
# Each takes the inputs by name (device tensors, however presented) and returns (tuple of outputs, aux for the reference).
def _call_roche_fixed(i):
    from hode.solver import roche_solve
    return (roche_solve(i["y0"], i["theta"], i["w"], i["b"], i["t"], i["dosage"], i["dose_times"], method="rk4"),), None


def _with_tape(fn):
    """A dopri5 call with its accepted-step tape (hode.adaptive.read_tape): the reference replays the same steps.
    Reading the tape needs adaptive.keep_workspace = True, so these ops never run with the production setting (False),
    and _last_ws is cleared after every call: `interleaved` therefore interleaves over the workspaces the two autograd
    nodes saved, not over that module variable (the backward never reads it)."""
    from hode import adaptive
    adaptive.keep_workspace = True
    try:
        h = fn()
        return (h,), adaptive.read_tape()
    finally:
        adaptive.keep_workspace = False
        adaptive._last_ws = None


def _call_roche_dopri5(i):
    from hode.adaptive import roche_dopri5
    return _with_tape(lambda: roche_dopri5(i["y0"], i["theta"], i["w"], i["b"], i["t"], i["dosage"], i["dose_times"],
                                           rtol=DOPRI5_RTOL, atol=DOPRI5_ATOL, detach_first_step=True))


def _call_neural_dopri5(i):
    from hode.adaptive import neural_dopri5
    return _with_tape(lambda: neural_dopri5(i["y0"], i["w1"], i["b1"], i["w2"], i["b2"], i["t"], i["dosage"], i["dose_times"],
                                            rtol=NEURAL_DOPRI5_RTOL, atol=NEURAL_DOPRI5_ATOL, detach_first_step=True))


def _call_neural_fixed(i):
    from hode.neural import neural_solve
    return (neural_solve(i["y0"], i["w1"], i["b1"], i["w2"], i["b2"], i["t"], i["dosage"], i["dose_times"], method="rk4"),), None


def _call_real(i):
    from hode.real import real_solve
    return (real_solve(i["y0"], i["theta"], i["wflat"], i["t"], i["act"], 16, method="midpoint", perturb=True),), None


def _call_neural_real(kind):
    def call(i):
        from hode import neural_real as nr
        Ta = i["a"].shape[0]
        index = nr.table_index(nr.stage_rows(i["t"], "rk4", True, Ta), Ta).reshape(-1).to(i["a"].device)
        return (nr.neural_real_solve(kind, i["y0"], i["w1"], i["b1"], i["w2"], i["b2"], i["t"], i["a"], index, "rk4"),), None
    return call


def _call_tlstm(i):
    from hode.seqdec import tlstm
    return (tlstm(i["init"], i["a"], i["idx"], i["tau"], 19, i["w_ih"], i["w_hh"], i["b_ih"], i["b_hh"]),), None


def _call_gruode(i):
    from hode.seqdec import gruode
    return (gruode(i["init"], i["a"], i["idx"], i["tau"], 19, i["w_z"], i["w_n"]),), None


def _call_lstm_encode(i):
    from hode.lstm import lstm_encode
    return (lstm_encode(i["x"], i["a"], i["mask"], i["w_ih"], i["w_hh"], i["b_ih"], i["b_hh"], reverse=True),), None


def _call_lstm_final(i):
    from hode.lstm import lstm_final_state
    return tuple(lstm_final_state(i["x"], i["a"], i["mask"], i["w_ih"], i["w_hh"], i["b_ih"], i["b_hh"], reverse=True)), None


def _call_readout(i):
    from hode.readout import masked_sse_readout
    return (masked_sse_readout(i["h"], i["x"], i["mask"], i["w"], i["b"]),), None


def _call_readout_mlp(i):
    from hode.readout import masked_sse_readout_mlp
    return (masked_sse_readout_mlp(i["h"], i["x"], i["mask"], i["w1"], i["b1"], i["w2"], i["b2"], i["time_weight"], skip_rows=1),), None


def _call_mckl(i):
    from hode.mckl import mc_kl_exponential
    return (mc_kl_exponential(i["mu"], i["log_var"], i["noise"], MCKL_RATE, MCKL_CLAMP),), None


def _call_flow(i):
    from hode.flow import planar_flow_sample
    return tuple(planar_flow_sample(i["mu"], i["log_var"], i["u"], i["w"], i["b"], i["noise"], s_kl=1)), None


def _call_crps(i):
    from hode.crps import ensemble_crps
    return (ensemble_crps(i["h"], i["truth"], CRPS_MEMBERS, i["weight"], i["bias"], per_component=True),), None


# ---------------------------------------------------------------------------------------- float64 references (CPU)
# Each takes the same inputs as float64 CPU tensors (the differentiable ones are leaves) and the call's aux, and returns
# the outputs as float64 tensors autograd can differentiate.
def _roche_func(i):
    from oracle.rhs import THETA_NAMES, RocheRHS
    f = RocheRHS(i["y0"].shape[1], 1.0).double()
    f.dosage, f.times = i["dosage"], i["dose_times"]
    prm = {n: i["theta"][k] for k, n in enumerate(THETA_NAMES)}
    prm["ml_net.0.weight"], prm["ml_net.0.bias"] = i["w"], i["b"]
    return lambda t, y: torch.func.functional_call(f, prm, (t, y))


def _neural_func(i):
    from oracle.rhs import NeuralRHS
    f = NeuralRHS(i["y0"].shape[1], 1.0).double()
    f.dosage, f.times = i["dosage"], i["dose_times"]
    prm = {"ml_net.0.weight": i["w1"], "ml_net.0.bias": i["b1"], "ml_net.2.weight": i["w2"], "ml_net.2.bias": i["b2"]}
    return lambda t, y: torch.func.functional_call(f, prm, (t, y))


def ref_roche_fixed(i, aux):
    from oracle.solvers import odeint
    return (odeint(_roche_func(i), i["y0"], i["t"], method="rk4"),)


def ref_neural_fixed(i, aux):
    from oracle.solvers import odeint
    return (odeint(_neural_func(i), i["y0"], i["t"], method="rk4"),)


def _replay(func, i, aux, rtol, atol):
    from oracle.solvers import odeint_dopri5_replay
    return (odeint_dopri5_replay(func, i["y0"], i["t"], rtol, atol, list(zip(aux["t"], aux["dt"])), False),)


def ref_roche_dopri5(i, aux):
    return _replay(_roche_func(i), i, aux, DOPRI5_RTOL, DOPRI5_ATOL)


def ref_neural_dopri5(i, aux):
    return _replay(_neural_func(i), i, aux, NEURAL_DOPRI5_RTOL, NEURAL_DOPRI5_ATOL)


def ref_real(i, aux):
    from oracle.rhs import RocheRealRHS
    from oracle.solvers import odeint
    D, H = i["y0"].shape[1], 16
    M = D - 4
    f = RocheRealRHS(D, H).double()
    f.set_action_static(i["act"][..., None])
    names = [("dx1_net.0.weight", (H, 3)), ("dx1_net.0.bias", (H,)), ("dx1_net.2.weight", (1, H)), ("dx1_net.2.bias", (1,)),
             ("dx2_net.0.weight", (H, 2)), ("dx2_net.0.bias", (H,)), ("dx2_net.2.weight", (1, H)), ("dx2_net.2.bias", (1,)),
             ("lin_hh.weight", (M, M)), ("lin_hz.weight", (M, M)), ("lin_hr.weight", (M, M))]
    prm, o = {"k_immunity": i["theta"][0], "kel": i["theta"][1], "kel2": i["theta"][2]}, 0
    for n, shape in names:  # the flat buffer in parameter creation order (include/hode.h, w1 of HODE_RHS_ROCHE_REAL)
        k = int(torch.Size(shape).numel())
        prm[n] = i["wflat"][o:o + k].view(shape)
        o += k
    func = lambda t, y: torch.func.functional_call(f, prm, (t, y))  # noqa: E731
    return (odeint(func, i["y0"], i["t"], method="midpoint", options={"perturb": True, "step_size": 1.0}),)


def _ref_neural_real(kind):
    def ref(i, aux):
        import warnings

        import neural_real_eager
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            h, _ = neural_real_eager.solve(kind, i["y0"], i["w1"], i["b1"], i["w2"], i["b2"], i["a"], i["t"], "rk4",
                                           step_size=1.0, perturb=True)
        return (h,)
    return ref


def ref_tlstm(i, aux):
    import seqdec_eager
    return (seqdec_eager.tlstm(i["init"], i["a"], i["idx"].tolist(), i["tau"], i["w_ih"], i["w_hh"], i["b_ih"], i["b_hh"]),)


def ref_gruode(i, aux):
    import seqdec_eager
    return (seqdec_eager.gruode(i["init"], i["a"], i["idx"].tolist(), i["tau"], i["w_z"], i["w_n"]),)


def _lstm_final(i):
    from oracle.encoder import EncoderLSTMOracle
    H = i["w_hh"].shape[1]
    enc = EncoderLSTMOracle(i["w_ih"].shape[1], H, 1).double()
    enc.forward = enc.final_hidden  # functional_call runs forward()
    prm = {"lstm.weight_ih_l0": i["w_ih"], "lstm.weight_hh_l0": i["w_hh"], "lstm.bias_ih_l0": i["b_ih"], "lstm.bias_hh_l0": i["b_hh"]}
    return torch.func.functional_call(enc, prm, (i["x"], i["a"], i["mask"]))


def ref_lstm_encode(i, aux):
    return (_lstm_final(i)[0],)


def ref_lstm_final(i, aux):
    return tuple(_lstm_final(i))


def ref_readout(i, aux):
    from oracle.vi import masked_sse
    return (masked_sse(i["x"], i["h"] @ i["w"].t() + i["b"], i["mask"]),)


def ref_readout_mlp(i, aux):
    h = i["h"][1:]  # skip_rows = 1
    x_hat = torch.nn.functional.elu(h @ i["w1"].t() + i["b1"]) @ i["w2"].t() + i["b2"]
    return (torch.sum((i["x"] - x_hat) ** 2 * i["mask"] * i["time_weight"][:, None, None]) / h.shape[1],)


def ref_mckl(i, aux):
    """tests/test_hip_mckl.py's literal loop builds its own leaves: its formula is run on the given leaves here through
    the same oracle densities (oracle.vi)."""
    from oracle.vi import exponential_log_density, gaussian_log_density
    std = torch.exp(0.5 * i["log_var"])
    terms = []
    for s in range(i["noise"].shape[0]):
        z = i["noise"][s] * std + i["mu"]
        z = torch.where(z <= 0.0, torch.full_like(z, MCKL_CLAMP), z)[..., None]  # per element: the densities sum a last axis of 1
        terms.append(gaussian_log_density(i["mu"][..., None], i["log_var"][..., None], z) - exponential_log_density(z, MCKL_RATE))
    return (torch.stack(terms, dim=-1).mean(dim=-1),)


def ref_flow(i, aux):
    import flow_eager
    z_out, kl, _, _ = flow_eager.forward(i["mu"], i["log_var"], i["u"], i["w"], i["b"], i["noise"], 1)
    return (z_out, kl)


def ref_crps(i, aux):
    from oracle.evalmetrics import crps_sorted
    Tn, MB, Dv = i["h"].shape
    B = MB // CRPS_MEMBERS
    vals = i["h"].view(Tn, CRPS_MEMBERS, B, Dv) @ i["weight"].t() + i["bias"]          # (Tn, M, B, obs)
    return (torch.from_numpy(crps_sorted(i["truth"].numpy(), vals.permute(0, 2, 3, 1).numpy())),)


# ------------------------------------------------------------------------------------------------------- the table
Op = collections.namedtuple("Op", "name binds build call ref diff nondiff expand tol mutated")
"""binds: the bindings of hode/ the entry covers (`module.name`); diff: differentiable inputs, in order; nondiff: float
tensor inputs the binding gives no gradient for; expand: inputs that are constant along time under `expanded`;
tol: the family whose bounds apply (tests/test_hip_binding_contract.py TOLERANCES); mutated: (input, "raises") when the
backward re-reads that input -- autograd's version counter must refuse a change between forward and backward -- or
(input, "copy") when the binding formed everything the backward needs during the forward."""

_W4 = ("w1", "b1", "w2", "b2")
OPS = collections.OrderedDict((op.name, op) for op in (
    Op("roche_fixed", ("solver._RocheFixedGrid",), _roche_inputs, _call_roche_fixed, "ref_roche_fixed",
       ("y0", "theta", "w", "b"), ("t", "dosage", "dose_times"), (), "roche", ("theta", "raises")),
    Op("roche_dopri5", ("adaptive._RocheDopri5",), _roche_inputs, _call_roche_dopri5, "ref_roche_dopri5",
       ("y0", "theta", "w", "b"), ("t", "dosage", "dose_times"), (), "roche", ("theta", "raises")),
    Op("neural_dopri5", ("adaptive._NeuralDopri5",), _neural_dopri5_inputs, _call_neural_dopri5, "ref_neural_dopri5",
       ("y0",) + _W4, ("t", "dosage", "dose_times"), (), "neural_dopri5", ("w1", "raises")),
    Op("neural_fixed", ("neural._NeuralFixedGrid",), _neural_inputs, _call_neural_fixed, "ref_neural_fixed",
       ("y0",) + _W4, ("t", "dosage", "dose_times"), (), "roche", ("w1", "raises")),
    Op("real", ("real._RealFixedGrid",), _real_inputs, _call_real, "ref_real",
       ("y0", "theta", "wflat"), ("t", "act"), ("act",), "roche", ("wflat", "raises")),
    Op("neural_real", ("neural_real._NeuralRealFixedGrid",), _neural_real_inputs, _call_neural_real("neural"),
       "ref_neural_real", ("y0",) + _W4, ("t", "a"), ("a",), "neural_real", ("w1", "raises")),
    Op("neural_real_2nd", ("neural_real._NeuralRealFixedGrid",), _neural_real_2nd_inputs, _call_neural_real("2nd"),
       "ref_neural_real_2nd", ("y0",) + _W4, ("t", "a"), ("a",), "neural_real", ("w1", "raises")),
    Op("tlstm", ("seqdec._Tlstm", "seqdec._forward", "seqdec._backward"), _tlstm_inputs, _call_tlstm, "ref_tlstm",
       ("init", "w_ih", "w_hh", "b_ih", "b_hh"), ("a", "tau"), ("a",), "roche", ("init", "raises")),
    Op("gruode", ("seqdec._GruOde", "seqdec._forward", "seqdec._backward"), _gruode_inputs, _call_gruode, "ref_gruode",
       ("init", "w_z", "w_n"), ("a", "tau"), ("a",), "roche", ("init", "raises")),
    Op("lstm_encode", ("lstm._LstmEncode",), _lstm_inputs, _call_lstm_encode, "ref_lstm_encode",
       ("w_ih", "w_hh", "b_ih", "b_hh"), ("x", "a", "mask"), ("a",), "lstm", ("w_hh", "raises")),
    Op("lstm_final_state", ("lstm.lstm_final_state",), _lstm_inputs, _call_lstm_final, "ref_lstm_final",
       (), ("w_ih", "w_hh", "b_ih", "b_hh", "x", "a", "mask"), ("a",), "lstm", None),
    Op("readout", ("readout._ReadoutSSE",), _readout_inputs, _call_readout, "ref_readout",
       ("h", "w", "b"), ("x", "mask"), ("mask",), "readout", ("h", "copy")),
    Op("readout_mlp", ("readout._ReadoutMlpSSE",), _readout_mlp_inputs, _call_readout_mlp, "ref_readout_mlp",
       ("h",) + _W4, ("x", "mask", "time_weight"), ("time_weight",), "readout_mlp", ("h", "copy")),
    Op("mckl", ("mckl._McKlExp", "mckl._launch"), _mckl_inputs, _call_mckl, "ref_mckl",
       ("mu", "log_var"), ("noise",), (), "mckl", ("mu", "copy")),
    Op("mckl_forward", ("mckl._launch",), _mckl_inputs, _call_mckl, "ref_mckl",
       (), ("mu", "log_var", "noise"), (), "mckl", None),
    Op("flow", ("flow._PlanarFlowKL",), _flow_inputs, _call_flow, "ref_flow",
       ("mu", "log_var", "u", "w", "b"), ("noise",), (), "flow", ("mu", "raises")),
    Op("crps", ("crps.ensemble_crps",), _crps_inputs, _call_crps, "ref_crps",
       (), ("h", "truth", "weight", "bias"), ("truth",), "crps", None),
))
ref_neural_real, ref_neural_real_2nd = _ref_neural_real("neural"), _ref_neural_real("2nd")

#: ops whose plain call gives the same bits every time.  Seeded from what the suite already asserts
#: (test_hip_flow.py test_bit_identical_repeats; test_hip_neural_real.py and test_hip_seqdec.py
#: test_backward_is_bitwise_reproducible; test_hip_metric_cases.py _same_bits); the others were added after two plain runs
#: of each on an MI355X came out equal (tests/test_hip_binding_contract.py::test_plain_call_repeats measures it).
DETERMINISTIC = ("flow", "neural_real", "neural_real_2nd", "tlstm", "gruode", "crps", "mckl", "mckl_forward",
                 "roche_fixed", "roche_dopri5", "neural_dopri5", "neural_fixed", "real", "lstm_encode", "lstm_final_state",
                 "readout", "readout_mlp")
#: ops left out of DETERMINISTIC -> why (they carry the float64 comparison only)
NONDETERMINISTIC = {}


# --------------------------------------------------------------------------------------------------- presentations
def _into(buf_view, x):
    buf_view.copy_(x)
    return buf_view


def offset_view(x, dev, k):
    """A contiguous view with the values of x that starts k elements into a larger buffer (NaN around it)."""
    buf = torch.full((x.numel() + 4,), float("nan") if x.is_floating_point() else -1, dtype=x.dtype).to(dev)
    return _into(buf[k:k + x.numel()].view(x.shape), x.to(dev))


def strided_view(x, dev):
    """A non-contiguous view with the values of x: 1-D as every other element of a doubled buffer; otherwise the last two
    dimensions as a transposed view of a transposed buffer, the batch dimension (dim 1 of a 3-D tensor, else dim 0) as
    every other row of a doubled buffer.  The gaps hold NaN."""
    if x.dim() == 0:
        return x.to(dev)
    if x.dim() == 1:
        return _into(torch.full((2 * x.numel(),), float("nan"), dtype=x.dtype).to(dev)[::2], x.to(dev))
    bd = 1 if x.dim() >= 3 else 0
    shape = list(x.shape)
    shape[bd] *= 2
    shape[-1], shape[-2] = shape[-2], shape[-1]
    buf = torch.full(shape, float("nan"), dtype=x.dtype).to(dev).transpose(-1, -2)
    view = buf[:, ::2] if bd == 1 else buf[::2]
    assert not view.is_contiguous() or x.numel() <= 1
    return _into(view, x.to(dev))


def expanded_view(x, dev):
    """Row 0 of x along time as a stride-0 expand (the plain call gets the same values as a dense tensor)."""
    return x[:1].to(dev).expand(x.shape)


PRESENTATIONS = (
    "offset4", "offset8", "strided", "expanded", "fp64",
    "cot_stack", "cot_cat", "cot_sum", "cot_transpose", "cot_fp64",
    "one_grad[0]", "one_grad[1]", "one_grad[2]", "one_grad[3]", "one_grad[4]", "no_grad_inputs", "no_grad_mode",
    "twice", "interleaved", "side_stream", "index_dtypes", "mutated", "nondiff_requires_grad",
)
#: presentations no op with a float tensor input may opt out of
ALWAYS = ("offset4", "offset8", "strided", "fp64")
#: presentations no differentiable op may opt out of (one_grad[i] for every i below its number of differentiable inputs)
ALWAYS_DIFF = ("cot_stack", "cot_cat", "cot_sum", "cot_transpose", "cot_fp64", "twice", "interleaved", "side_stream", "mutated")
_NEEDS_BACKWARD = ("cot_stack", "cot_cat", "cot_sum", "cot_transpose", "cot_fp64", "twice", "interleaved", "mutated",
                   "nondiff_requires_grad")


def _inapplicable():
    out = {}
    for op in OPS.values():
        has_idx = "idx" in op.build(0)
        for p in PRESENTATIONS:
            if p == "index_dtypes" and not has_idx:
                out[(op.name, p)] = "no index table: only the seqdec bindings take idx / tau"
            elif p == "expanded" and not op.expand:
                out[(op.name, p)] = "no input that is constant along time"
            elif p.startswith("one_grad[") and int(p[9:-1]) >= len(op.diff):
                out[(op.name, p)] = "the op has %d differentiable inputs" % len(op.diff)
            elif p in _NEEDS_BACKWARD and not op.diff:
                out[(op.name, p)] = "forward-only launch: no backward, no cotangent"
    return out


INAPPLICABLE = _inapplicable()


def pairs():
    return [(o, p) for o in OPS for p in PRESENTATIONS if (o, p) not in INAPPLICABLE]


def present(op, pres, name, x, dev):
    """Input `name` (a plain CPU tensor, or None) as the presentation hands it to the binding, on `dev`."""
    if x is None:
        return None
    if not x.is_floating_point():
        return (x.to(torch.int64) if pres == "index_dtypes" else x).to(dev)
    if pres == "offset4":
        return offset_view(x, dev, 1)
    if pres == "offset8":
        return offset_view(x, dev, 2)
    if pres == "strided":
        return strided_view(x, dev)
    if pres == "expanded" and name in op.expand:
        return expanded_view(x, dev)
    if pres == "fp64" or (pres == "index_dtypes" and name == "tau"):
        return x.double().to(dev)
    return x.to(dev)


def prepare(op, pres, inputs):
    """The plain inputs of the pair: `expanded` makes the time-constant inputs constant along time first."""
    if pres != "expanded":
        return inputs
    return collections.OrderedDict((k, v[:1].expand(v.shape).contiguous() if k in op.expand else v) for k, v in inputs.items())
