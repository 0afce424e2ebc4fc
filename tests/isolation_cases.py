"""The case table of the patient-isolation tests of the real-data and recurrent kernels: the ODE decoders (real_kernel,
real_mf_kernel, real_dims_kernel, real_step_kernel, neural_real_*), the recurrent decoders (tlstm_*, gruode_*), the LSTM
(lstm_fwd / lstm_bwd, final-state and all-steps) and the readouts, at small shapes with one floating-point value of one
patient poisoned (NaN, +inf, -inf).  None of these kernels has a status word: a non-finite value is silent, and the only
guarantee is that it stays inside the patient it came from.  tests/test_isolation_cases.py (CPU) holds the table against the
built kernel symbols and pins what a poisoned run must give with each family's float64 reference; tests/test_hip_isolation.py
(GPU) runs it.  A plain helper module.

The cases are the seqdec, neural_real, real, lstm and readout entries of tests/kernel_variants.py, tests/real_dims_cases.py,
tests/real_step_cases.py and tests/lstm_seq_cases.py with what selects the instantiation kept -- D, hidden, kind, method,
perturb, patient_tiles, intervals_per_wave, obs % 4, the readout variant -- and the shape shrunk: T (or T') = 6 with the
edges 1 and 2 rotating through the table (the one-step-ahead solve has no T' = 1: N = 5, and the edges N = 1, 2), B = 50 =
48 + 2 (a ragged fourth wave of the 16-patients-per-wave layouts) and B = 5; the LSTM runs B = 16 NT k + 2, so that the last
workgroup of every patient-tile variant is ragged.  The poisoned row (0, 15, 16, 47, 48, B - 1), column, value and the
output time that carries the poisoned cotangent (0, T // 2, T - 1) rotate through the table as tests/failure_cases.py's do;
no full product.  Two sharp cases per family and layout go in by name: the first patient of the ragged block with column 0
(the element every past-the-batch slot of the LSTM forward reads), and the last patient (the one every dead lane of the
recurrent decoders' backward aliases).

Only floating-point DATA is poisoned -- start states, measurements, actions, cotangents -- never an index table, a size, a
time grid or a weight: no kernel addresses memory it would not address on clean data.

CASES holds the cases whose float64 reference turns the poisoned patient non-finite, SATURATING those where it saturates
back to finite values (an infinite measurement or action into the LSTM gates: sigmoid -> 0 / 1, tanh -> +-1): there the
kernels are held to the reference within the family's own tolerance."""
import functools

import torch

import kernel_variants as kv
import lstm_seq_cases as lsc
import real_dims_cases as rdc
import real_step_cases as rsc

T_MAIN, T_EDGES = 6, (2, 1)
BATCHES = (50, 5)
ROWS = (0, 15, 16, 47, 48)               # and B - 1
VALUE_NAMES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
VALUES = tuple(VALUE_NAMES)
#: (T, B) of the cases beside each instantiation's first one, which keeps (T_MAIN, 50)
_SHAPES = ((6, 5), (2, 50), (6, 50), (1, 50), (2, 5), (6, 50), (1, 5))
#: kernel-name prefixes the table has to reach, per library (build_hip.LIBRARIES key -> prefixes)
FAMILIES = {
    "libhode.so": ("real_kernel", "real_mf_kernel", "real_grad_fold_kernel", "neural_real_fwd_kernel", "neural_real_bwd_kernel",
                   "neural_real_fold_kernel", "tlstm_fwd_kernel", "tlstm_bwd_kernel", "gruode_fwd_kernel", "gruode_bwd_kernel",
                   "seqdec_fold_kernel", "lstm_fwd_kernel", "lstm_bwd_kernel", "lstm_fill_operand_kernel", "readout_sse_kernel",
                   "readout_mf_kernel", "readout_fold_kernel", "readout_mlp_kernel", "readout_mlp_fold_kernel"),
    "libhode_real_dims.so": ("real_dims_kernel", "real_dims_fold_kernel"),
    "libhode_real_step.so": ("real_step_kernel", "real_step_dose_kernel", "real_step_fold_kernel"),
    "libhode_lstm_seq.so": ("lstm_seq_fwd_kernel", "lstm_seq_bwd_kernel", "lstm_fill_operand_kernel"),
}
TA_ODE = 12       # action rows of the ODE decoders (tests/real_dims_cases.py TA)
TA_SEQDEC = 10    # action rows of the recurrent decoders: the steps read rows TA - T' .. TA - 1


def base(name):
    """`hode::real_mf_kernel<1, 2, true, false>` -> `real_mf_kernel`."""
    return name.split("<")[0].replace("hode::", "")


def rows(B):
    return tuple(r for r in ROWS if r < B - 1) + (B - 1,)


def _axes(i, B, T, ncol):
    """The rotating axes of case number i: poisoned row, column, value and the output time of the poisoned cotangent."""
    r = rows(B)
    cols = sorted({0, 1 % ncol, 3 % ncol, ncol - 1})
    return dict(row=r[i % len(r)], col=cols[(i // 2 + i) % len(cols)], value=VALUES[(i // 3 + i) % 3], n=(0, T // 2, T - 1)[i % 3])


def _shaped(bases, inst, ncol, sharp_of):
    """The shapes and the rotating axes for a list of base cases: the first case of every instantiation (`inst(c)`) keeps
    (T_MAIN, 50), the others walk _SHAPES; then the two sharp cases of every layout `sharp_of(c)` names."""
    out, first, sharp = [], set(), {}
    for i, c in enumerate(bases):
        T, B = (T_MAIN, 50) if inst(c) not in first else _SHAPES[i % len(_SHAPES)]
        first.add(inst(c))
        out.append(dict(c, T=T, B=B, seed=900 + i, **_axes(i, B, T, ncol(c))))
        sharp.setdefault(sharp_of(c), c)
    for j, c in enumerate(sharp.values()):
        for row, col in ((48, 0), (49, ncol(c) - 1)):
            out.append(dict(c, T=T_MAIN, B=50, seed=800 + j, row=row, col=col, value="nan", n=T_MAIN - 1, sharp=True))
    # every layout at every edge shape, whatever the rotation above gave it: its bases in turn
    for j, key in enumerate(sharp):
        mine = [c for c in bases if sharp_of(c) == key]
        for k, (T, B) in enumerate(s for s in _SHAPES if s != (T_MAIN, 50)):
            c = mine[(j + 2 * k + 1) % len(mine)]
            out.append(dict(c, T=T, B=B, seed=500 + 7 * j + k, **_axes(j + k, B, T, ncol(c))))
    return out


# ------------------------------------------------------------------------------------------------------ ODE decoders
def _real_bases():
    """tests/kernel_variants.py's `real` entries (libhode.so: D = 20 on the matrix cores with the on-chip and the
    tape-writing backward, D = 20 with hidden > 64 and D = 4 a lane per patient), one per compiled real_dims_kernel
    (tests/real_dims_cases.py: HT x method, the latent size rotating through 5 .. 19) and one per compiled real_step_kernel
    (tests/real_step_cases.py: HT x method; S and C rotate)."""
    out = [dict(family="real", D=c["D"], H=c["H"], method=c["method"], onchip=c["onchip"], perturb=rdc.perturb(c["method"]))
           for c in kv.CASES if c["family"] == "real"]
    i = 0
    for ht, H in zip(rdc.HTS, (16, 17, 43, 64)):
        for method in rdc.METHODS:
            out.append(dict(family="real_dims", D=rdc.DIMS[(4 * i) % len(rdc.DIMS)], H=(H, 16 * ht - 15)[i % 2], method=method,
                            onchip=True, perturb=rdc.perturb(method)))
            i += 1
    for ht, H in zip(rsc.HTS, (16, 17, 43, 64)):
        for method in rsc.METHODS:
            out.append(dict(family="real_step", D=rsc.EDGE_D[i % len(rsc.EDGE_D)], H=(H, 16 * ht - 15)[i % 2], method=method,
                            onchip=True, perturb=rsc.perturb(method), S=rsc.EDGE_S[i % 3], C=(0, 1, 2, 3, 7)[i % 5]))
            i += 1
    return out


def _neural_real_bases():
    return [dict(family="neural_real", kind=c["kind"], D=c["D"], H=c["H"], method=c["method"], perturb=c["perturb"])
            for c in kv.CASES if c["family"] == "neural_real"]


def _ode_cases():
    def inst(c):
        return (c["family"], c.get("kind"), tuple(kernels(dict(c, T=6, B=50))[:2]))

    def lay(c):
        return (c["family"], c.get("kind"), base(kernels(dict(c, T=6, B=50))[0]))

    out = _shaped(_real_bases() + _neural_real_bases(), inst, lambda c: c["D"], lay)
    for c in out:
        if c["family"] == "real_step":   # N = T - 1 intervals; there is no solve without one: the edges are N = 1 and N = 2
            c["N"] = {6: 5, 2: 1, 1: 2}[c["T"]]
            c["T"] = c["N"] + 1
            c["n"] = min(c["n"], c["N"])
            c["interval"] = c["seed"] % c["N"]   # the interval whose start state is poisoned
    return out


# ------------------------------------------------------------------------------------------------- recurrent decoders
def _seqdec_cases():
    """tests/kernel_variants.py's seqdec entries: both kinds at both edges of every tile class <1,1>, <1,2>, <2,2>.  What is
    poisoned in the forward alternates between `init` and the action table `a`, at a row a step really reads."""
    bases, seen = [], set()
    for c in kv.CASES:
        if c["family"] == "seqdec" and (c["kind"], c["D"]) not in seen:
            seen.add((c["kind"], c["D"]))
            bases.append(dict(family="seqdec", kind=c["kind"], D=c["D"]))
    bases = [dict(c, what=w) for c in bases for w in ("init", "a")]
    out = _shaped(bases, lambda c: (c["kind"], kv.seqdec_tiles(c["D"]), c["what"]), lambda c: c["D"],
                  lambda c: (c["kind"], kv.seqdec_tiles(c["D"])))
    for c in out:
        c["k"] = (0, c["T"] // 2, c["T"] - 1)[(c["seed"] // 3) % 3]   # the step whose action row is poisoned
        if c["what"] == "a":
            c["col"] = 0
    return out


# --------------------------------------------------------------------------------------------------------------- LSTM
LSTM_WHATS = ("x1", "x0", "a")   # a measurement with mask 1, one with mask 0 (x * mask keeps the NaN), an action


def _lstm_case(lib, tpw, nt, vec4, flat, i, **over):
    """One LSTM case: `lib` "final" (libhode.so, h and c after the window) or "seq" (libhode_lstm_seq.so, h of every step);
    the batch is ragged against the patient tile 16 NT; `tx` is the time row of the poisoned input."""
    H = 16 * tpw - (0 if flat else 3)
    obs = lsc.OBS_VEC4 if vec4 else lsc.OBS_ODD
    T = over.get("T", (6, 6, 6, 2, 6, 6, 1, 6)[i % 8])
    B = 16 * nt * (1 + i % 2) + 2
    r = tuple(x for x in ROWS if x < B - 2) + (B - 2, B - 1)
    what = LSTM_WHATS[i % 3]
    # the main table: an infinite value only behind mask 0 (inf * 0 = NaN); in front of the gates it saturates (SATURATING)
    value = VALUES[(i // 3 + i) % 3] if what == "x0" else "nan"
    c = dict(family="lstm", lib=lib, H=H, obs=obs, B=B, T=T, nt=nt, tape=nt <= 3, reverse=(i // 2) % 2, what=what,
             row=r[i % len(r)], col=(0, obs - 1, 3, 4)[(i // 2 + i) % 4], tx=(0, T // 2, T - 1)[(i // 3) % 3], value=value,
             hcol=(0, H - 1, H // 2)[i % 3], n=(0, T // 2, T - 1)[i % 3], cvalue=VALUES[i % 3], seed=700 + i)
    c.update(over)
    if c["what"] == "a":
        c["col"] = 0
    return c


def _lstm_cases():
    """Every compiled forward (NT 1 .. 4, the wave tiling of every padded hidden size, VEC4 = obs % 4 == 0, PAD = padded
    hidden units) and backward (NT 1 .. 3, TPW, FLAT = no padded unit) of both libraries; NT = 4 has no tape (forward only)."""
    out, sat, i = [], [], 0
    for lib in ("final", "seq"):
        for tpw in kv.LSTM_TPWS:
            for nt in (1, 2, 3, 4):
                for vec4 in (True, False):
                    for flat in (True, False):   # FLAT of the backward, PAD (padded hidden units) of the forward
                        out.append(_lstm_case(lib, tpw, nt, vec4, flat, i))
                        i += 1
        # sharp: the first patient of the ragged block, observation 0 (what every past-the-batch slot reads), and B - 1
        for vec4 in (True, False):
            for row_back, col in ((2, 0), (1, 3)):
                c = _lstm_case(lib, 3, 2, vec4, False, i, T=6, what="x1", value="nan", col=col, tx=(0, 5)[vec4], sharp=True)
                out.append(dict(c, row=c["B"] - row_back))
                i += 1
        # saturating: +-inf in front of the gates, on padded hidden units (H = 16 TPW - 3, and the encoders' own 44 and 75)
        for j, tpw in enumerate(kv.LSTM_TPWS):
            sat.append(_lstm_case(lib, tpw, 1 + j % 3, j % 2 == 0, False, i, T=6, what=("x1", "a")[j % 2], value=("+inf", "-inf")[(j // 2) % 2]))
            i += 1
        for H, obs in ((44, 24), (75, 37)):
            sat.append(_lstm_case(lib, (H + 15) // 16, 2, obs % 4 == 0, False, i, T=6, what="x1", value="+inf", H=H, obs=obs,
                                  hcol=H - 1, col=obs - 1))
            i += 1
    return out, sat


# ----------------------------------------------------------------------------------------------------------- readouts
READOUT_WHATS = ("h", "x1", "x0")   # an entry of h, a measurement with mask 1, one with mask 0


def _readout_cases():
    """tests/kernel_variants.py's readout entries (the lane kernel at every latent size, both sides of the matrix-core
    windows, the lane kernel forced inside them, the two-layer readout at both sizes), each with every READOUT_WHATS."""
    bases, seen = [], set()
    for c in kv.CASES:
        if c["family"] not in ("readout", "readout_mlp"):
            continue
        key = (c["family"], c["D"], c["obs"], c.get("valu", False))
        if key not in seen:
            seen.add(key)
            bases.append(dict(family=c["family"], D=c["D"], obs=c["obs"], valu=bool(c.get("valu", False))))
    out = []
    for i, c in enumerate(dict(c, what=w) for c in bases for w in READOUT_WHATS):
        T, B = (((T_MAIN, 50),) + _SHAPES)[(i + i // 8) % 8]
        ncol = c["D"] if c["what"] == "h" else c["obs"]
        a = _axes(i, B, T, ncol)
        out.append(dict(c, T=T, B=B, seed=600 + i, row=a["row"], col=a["col"], value=a["value"], n=a["n"]))   # n: the time row
    for j, c in enumerate(b for b in bases if (b["D"], b["obs"]) in ((4, 20), (12, 80), (20, 24))):
        for row, col, what in ((48, 0, "x1"), (49, c["D"] - 1, "h")):
            out.append(dict(c, what=what, T=T_MAIN, B=50, seed=580 + j, row=row, col=col, value="nan", n=T_MAIN - 1, sharp=True))
    return out


# ------------------------------------------------------------------------------------------------------------- tables
def kernels(c):
    """The kernels one forward + backward of the case launches, by the rules of the tables the case came from."""
    f = c["family"]
    if f == "real":
        return kv.real_kernels(c["D"], c["H"], kv.METHODS[c["method"]], c["onchip"])
    if f == "real_dims":
        return rdc.kernels(c)[:3]
    if f == "real_step":
        return [k for k in rsc.kernels(c) if "fold_partials" not in k]
    if f == "neural_real":
        return kv.neural_real_kernels(c["kind"], c["D"], c["H"], kv.METHODS[c["method"]])
    if f == "seqdec":
        return kv.seqdec_kernels(c["kind"], c["D"])
    if f == "lstm":
        names = kv.lstm_kernels(c["H"], c["obs"], c["B"], c["tape"], c["nt"]) if c["lib"] == "final" else lsc.kernels(c)
        return [k for k in names if "pack" not in k]
    if f == "readout":
        v = int(c["valu"])
        return kv.readout_kernels(c["D"], c["obs"], True, v) + kv.readout_kernels(c["D"], c["obs"], False, v)[:1]
    if f == "readout_mlp":
        return kv.readout_mlp_kernels(c["D"], True) + kv.readout_mlp_kernels(c["D"], False)[:1]
    raise ValueError(f)


def library(c):
    """The build_hip.LIBRARIES key of the library that serves the case."""
    f = c["family"]
    if f == "lstm":
        return "libhode.so" if c["lib"] == "final" else "libhode_lstm_seq.so"
    return {"real_dims": "libhode_real_dims.so", "real_step": "libhode_real_step.so"}.get(f, "libhode.so")


def case_id(c):
    f = c["family"]
    poison = "p%d.%d=%s-n%d" % (c["row"], c["col"], c["value"], c["n"]) + ("-sharp" if c.get("sharp") else "")
    if f in ("real", "real_dims", "real_step", "neural_real"):
        s = "%s%s-D%d-H%d-%s%s" % (f, "-" + c["kind"] if "kind" in c else "", c["D"], c["H"], c["method"], "" if c.get("onchip", True) else "-tape")
        if f == "real_step":
            s += "-S%d-C%d-i%d" % (c["S"], c["C"], c["interval"])
        return "%s-T%d-B%d-%s" % (s, c["T"], c["B"], poison)
    if f == "seqdec":
        return "%s-D%d-T%d-B%d-%s-k%d-%s" % (c["kind"], c["D"], c["T"], c["B"], c["what"], c["k"], poison)
    if f == "lstm":
        return "lstm-%s-H%d-obs%d-nt%d-%s-T%d-B%d-%s-t%d-%s-h%d=%s" % (c["lib"], c["H"], c["obs"], c["nt"], "r" if c["reverse"] else "f",
                                                                      c["T"], c["B"], c["what"], c["tx"], poison, c["hcol"], c["cvalue"])
    return "%s-D%d-obs%d%s-T%d-B%d-%s-%s" % (f, c["D"], c["obs"], "-valu" if c["valu"] else "", c["T"], c["B"], c["what"], poison)


def value_of(c, key="value"):
    return VALUE_NAMES[c[key]]


# --------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    return torch.Generator().manual_seed(c["seed"])


def real_flat(f):
    """The flat weight buffer of an oracle.rhs.RocheRealRHS, in the parameter creation order the kernels read."""
    ps = [f.dx1_net[0].weight, f.dx1_net[0].bias, f.dx1_net[2].weight, f.dx1_net[2].bias,
          f.dx2_net[0].weight, f.dx2_net[0].bias, f.dx2_net[2].weight, f.dx2_net[2].bias]
    if f.ml_dim > 0:
        ps += [f.lin_hh.weight, f.lin_hz.weight, f.lin_hr.weight]
    return ps


def _problem(c):
    """The clean inputs of a case as fp32 CPU tensors (and the float64 reference's module where it has one)."""
    f, gen = c["family"], _gen(c)
    B, T = c["B"], c["T"]
    torch.manual_seed(c["seed"])
    if f in ("real", "real_dims", "real_step"):
        from oracle.rhs import RocheRealRHS
        D, H = c["D"], c["H"]
        rhs = RocheRealRHS(D, H)
        a = (torch.rand(TA_ODE, B, 1, generator=gen) < 0.2).float() * torch.rand(TA_ODE, B, 1, generator=gen)
        t = torch.arange(4, 4 + T, 1, dtype=torch.float32)   # doses before the window and inside it
        p = dict(rhs=rhs, a=a, act=a[..., 0].contiguous(), t=t, cot=torch.randn(T, B, D, generator=gen),
                 wflat=torch.cat([q.detach().reshape(-1) for q in real_flat(rhs)]),
                 theta=torch.stack([rhs.k_immunity, rhs.kel, rhs.kel2]).detach())
        if f == "real_step":
            p["y0"] = torch.randn(c["N"], B, D, generator=gen) * 0.3
        else:
            p["y0"] = torch.randn(B, D, generator=gen) * 0.3
        return p
    if f == "neural_real":
        from hode import neural_real as nr
        D, H = c["D"], c["H"]
        n_out = D // 2 if c["kind"] == "2nd" else D
        l1, l2 = torch.nn.Linear(D + 1, H), torch.nn.Linear(H, n_out)
        a = (torch.rand(TA_ODE, B, 1, generator=gen) < 0.4).float() * torch.rand(TA_ODE, B, 1, generator=gen) * 2
        t = torch.arange(2, 2 + T, 1, dtype=torch.float32)
        index = nr.table_index(nr.stage_rows(t, c["method"], c["perturb"], TA_ODE), TA_ODE).reshape(-1)
        return dict(a=a, t=t, dose=nr.dose_table(a, index).contiguous(), y0=torch.randn(B, D, generator=gen) * 0.5,
                    cot=torch.randn(T, B, D, generator=gen), w=[q.detach().clone() for q in (l1.weight, l1.bias, l2.weight, l2.bias)])
    if f == "seqdec":
        D = c["D"]
        if c["kind"] == "tlstm":
            r = torch.nn.LSTM(2, D)
            w = [q.detach().clone() for q in (r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)]
        else:
            w = [torch.nn.Linear(D + 2, D + 2, bias=False).weight.detach().clone(), torch.nn.Linear(D + 2, D, bias=False).weight.detach().clone()]
        idx = torch.arange(TA_SEQDEC - T, TA_SEQDEC, dtype=torch.int32)
        a = (torch.rand(TA_SEQDEC, B, 1, generator=gen) < 0.3).float() * torch.rand(TA_SEQDEC, B, 1, generator=gen) * 2
        return dict(init=torch.randn(B, D, generator=gen) * 0.5, a=a, idx=idx, tau=idx.to(torch.float32) / TA_SEQDEC,
                    cot=torch.randn(T, B, D, generator=gen), w=w)
    if f == "lstm":
        H, obs = c["H"], c["obs"]
        lstm = torch.nn.LSTM(obs + 1, H)
        x = torch.randn(T, B, obs, generator=gen)
        a = torch.rand(T, B, 1, generator=gen) * (torch.rand(T, B, 1, generator=gen) < 0.3).float()
        m = (torch.rand(T, B, obs, generator=gen) < 0.5).float()
        if c["what"] in ("x1", "x0"):
            m[c["tx"], c["row"], c["col"]] = 1.0 if c["what"] == "x1" else 0.0
        cot = torch.randn(*((T, B, H) if c["lib"] == "seq" else (B, H)), generator=gen)
        return dict(x=x, a=a, m=m, cot=cot, w=[q.detach().clone() * 1.5 for q in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)])
    if f in ("readout", "readout_mlp"):
        D, obs = c["D"], c["obs"]
        if f == "readout":
            lin = torch.nn.Linear(D, obs)
            w = [lin.weight.detach().clone(), lin.bias.detach().clone()]
        else:
            l1, l2 = torch.nn.Linear(D, D + 1), torch.nn.Linear(D + 1, obs)
            w = [q.detach().clone() for q in (l1.weight, l1.bias, l2.weight, l2.bias)]
        m = (torch.rand(T, B, obs, generator=gen) < 0.6).float()
        if c["what"] in ("x1", "x0"):
            m[c["n"], c["row"], c["col"]] = 1.0 if c["what"] == "x1" else 0.0
        return dict(h=torch.randn(T, B, D, generator=gen), x=torch.randn(T, B, obs, generator=gen), m=m, w=w)
    raise ValueError(f)


@functools.lru_cache(maxsize=None)
def _setup(items):
    return _problem(dict(items))


def setup(c):
    """The clean inputs of a case, computed once and shared (nothing may write into them)."""
    return _setup(tuple(sorted(c.items())))


def forward_target(c):
    """(key, index) of the input entry the forward poison goes to."""
    f = c["family"]
    if f == "real_step":
        return "y0", (c["interval"], c["row"], c["col"])
    if f in ("real", "real_dims", "neural_real"):
        return "y0", (c["row"], c["col"])
    if f == "seqdec":
        if c["what"] == "init":
            return "init", (c["row"], c["col"])
        return "a", (TA_SEQDEC - c["T"] + c["k"], c["row"], 0)   # the row step k reads
    if f == "lstm":
        return ("a", (c["tx"], c["row"], 0)) if c["what"] == "a" else ("x", (c["tx"], c["row"], c["col"]))
    return ("h" if c["what"] == "h" else "x"), (c["n"], c["row"], c["col"])


def cot_target(c):
    """(index, value) of the poisoned cotangent entry (the readouts have none: their loss is a scalar)."""
    if c["family"] == "lstm":
        idx = (c["n"], c["row"], c["hcol"]) if c["lib"] == "seq" else (c["row"], c["hcol"])
        return idx, VALUE_NAMES[c["cvalue"]]
    return (c["n"], c["row"], c["col"] if c["family"] != "seqdec" or c["what"] == "init" else c["D"] - 1), value_of(c)


def poisoned(c, p=None):
    """The case's inputs with the forward entry poisoned (a copy of the one tensor; everything else is shared)."""
    p = setup(c) if p is None else p
    key, idx = forward_target(c)
    x = p[key].clone()
    x[idx] = value_of(c)
    return dict(p, **{key: x})


def poisoned_cot(c, cot=None):
    cot = (setup(c)["cot"] if cot is None else cot).clone()
    idx, v = cot_target(c)
    cot[idx] = v
    return cot


def cot_reaches(c):
    """What a poisoned cotangent entry reaches, by the structure of each family ("steps": at least one step or layer lies
    between it and the inputs, so the batch-summed gradients are non-finite and so is the patient's own gradient;
    "start": it is the cotangent of the start state itself and reaches grad_y0[p] alone; "nothing": row 0 of the
    one-step-ahead solve is the constant zero row).  tests/test_isolation_cases.py holds this against float64 autograd."""
    f = c["family"]
    if f == "real_step":
        return "nothing" if c["n"] == 0 else "steps"
    if f in ("real", "real_dims", "neural_real"):
        return "start" if c["n"] == 0 else "steps"
    return "steps"   # every output row of the recurrent kernels lies behind a cell


# ------------------------------------------------------------------------------------------------ float64 references
def _d(x):
    return None if x is None else x.double()


def reference(c, p, cot=None):
    """The family's float64 reference on the inputs `p`: a dict of the forward outputs (out_axis names the patient axis of
    each).  With a cotangent `cot` of h: also "pp", the per-patient gradient (grad_y0 / grad_init; the LSTM's reference has
    none), and "summed", the list of the batch-summed parameter gradients of sum(h * cot)."""
    import copy
    import warnings
    f, grad = c["family"], cot is not None

    def leaf(x):
        return x.double().clone().requires_grad_(grad)

    with torch.set_grad_enabled(grad), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if f in ("real", "real_dims", "real_step"):
            from oracle.solvers import odeint
            rhs = copy.deepcopy(p["rhs"]).double()
            rhs.set_action_static(p["a"].double())
            y0 = leaf(p["y0"])
            if f == "real_step":
                opts = {"perturb": c["perturb"], "step_size": 1.0 / c["S"]}
                ends = [odeint(rhs, y0[i], p["t"][i:i + 2].double(), method=c["method"], options=opts)[-1] for i in range(c["N"])]
                h = torch.stack([torch.zeros_like(ends[0])] + ends)
            else:
                h = odeint(rhs, y0, p["t"].double(), method=c["method"], options={"perturb": c["perturb"], "step_size": 1.0})
            prm = real_flat(rhs) + [rhs.k_immunity, rhs.kel, rhs.kel2]
        elif f == "neural_real":
            import neural_real_eager
            y0, prm = leaf(p["y0"]), [leaf(w) for w in p["w"]]
            if c["T"] == 1:
                h = y0[None] * 1.0
            else:
                h, _ = neural_real_eager.solve(c["kind"], y0, *prm, p["a"].double(), p["t"].double(), c["method"], perturb=c["perturb"])
        elif f == "seqdec":
            import seqdec_eager
            y0, prm = leaf(p["init"]), [leaf(w) for w in p["w"]]
            fn = seqdec_eager.tlstm if c["kind"] == "tlstm" else seqdec_eager.gruode
            h = fn(y0, p["a"].double(), [int(v) for v in p["idx"].tolist()], p["tau"].double(), *prm)
        elif f == "lstm":
            # the gates written out (oracle.encoder.lstm_cell's order i, f, g, o) on cat([x * mask, a]): a product with the
            # mask, so a NaN behind mask 0 stays a NaN
            y0, prm = None, [leaf(w) for w in p["w"]]
            w_ih, w_hh, b_ih, b_hh = prm
            seq = torch.cat([p["x"].double() * p["m"].double(), p["a"].double()], dim=-1)
            T, B, H = seq.shape[0], seq.shape[1], w_hh.shape[1]
            hh, cc, rows_ = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64), [None] * T
            for t in (range(T - 1, -1, -1) if c["reverse"] else range(T)):
                g = seq[t] @ w_ih.t() + b_ih + hh @ w_hh.t() + b_hh
                i_, f_, g_, o_ = (g[:, q * H:(q + 1) * H] for q in range(4))
                cc = torch.sigmoid(f_) * cc + torch.sigmoid(i_) * torch.tanh(g_)
                hh = torch.sigmoid(o_) * torch.tanh(cc)
                rows_[t] = hh
            h = torch.stack(rows_) if c["lib"] == "seq" else hh
        else:
            raise ValueError(f)
        out = dict(h=h.detach())
        if f == "lstm":
            out["c"] = cc.detach()
        if grad:
            (h * cot.double()).sum().backward()
            out["pp"] = None if y0 is None else y0.grad
            out["summed"] = [torch.zeros_like(q) if q.grad is None else q.grad for q in prm]
    return out


def readout_reference(c, p):
    """float64: the masked SSE / B of the (two-layer) readout, grad_h (T, B, D) and the parameter gradients."""
    h = p["h"].double().clone().requires_grad_(True)
    w = [q.double().clone().requires_grad_(True) for q in p["w"]]
    if c["family"] == "readout":
        x_hat = h @ w[0].t() + w[1]
    else:
        x_hat = torch.nn.functional.elu(h @ w[0].t() + w[1]) @ w[2].t() + w[3]
    lik = torch.sum((p["x"].double() - x_hat) ** 2 * p["m"].double()) / c["B"]
    lik.backward()
    return dict(lik=lik.detach(), grad_h=h.grad, summed=[q.grad for q in w])


#: the patient axis of each forward output / per-patient gradient, by (family, name)
def out_axis(c, name):
    if c["family"] == "lstm":
        return 1 if (name == "h" and c["lib"] == "seq") or name == "grad_gates" else 0
    if name in ("h", "grad_h"):
        return 1
    return 1 if c["family"] == "real_step" else 0   # grad_y0 / grad_init: (B, D), the one-step-ahead solve's (N, B, D)


def patient(x, axis, row):
    return x.select(axis, row)


def bad_rows(c, ref):
    """Per forward output: which entries along the time axis (or the output as a whole) are non-finite for the poisoned
    patient in the reference -- a bool tensor over the leading axis for (T, B, .) outputs, a 0-dim bool for (B, .) ones."""
    out = {}
    for k in ("h", "c"):
        if k not in ref:
            continue
        x = patient(ref[k], out_axis(c, k), c["row"])
        out[k] = ~torch.isfinite(x).all(dim=-1) if x.dim() == 2 else ~torch.isfinite(x).all()
    return out


def _classify():
    """CASES / SATURATING: a case whose reference leaves every output of the poisoned patient finite saturates.  Known by
    construction for the ODE decoders (an infinite state stays infinite) and the LSTM table (built that way above; the
    guard checks both); computed here for the recurrent decoders, whose cell may or may not swallow an infinite value."""
    lstm_main, lstm_sat = _lstm_cases()
    main, sat = _ode_cases(), []
    for c in _seqdec_cases():
        if c["value"] == "nan":
            main.append(c)
            continue
        bad = bad_rows(c, reference(c, poisoned(c, _problem(c))))
        (main if bool(bad["h"].any()) else sat).append(c)
    return main + lstm_main, sat + lstm_sat


CASES, SATURATING = _classify()
READOUT_CASES = _readout_cases()
BY_ID = {case_id(c): c for c in CASES + SATURATING + READOUT_CASES}

#: one case per family and layout for the position-invariance test: a patient alone (B = 1) against the same patient at rows
#: 0, 15, 16 and B - 1 of the B = 50 batch, with patient_tiles / lanes_per_patient / intervals_per_wave pinned by the case
POSITION_ROWS = (0, 15, 16, 49)


def _position_cases():
    seen, out = set(), []
    for c in CASES:
        if c["T"] != T_MAIN or c.get("sharp"):
            continue
        f = c["family"]
        if f == "lstm":
            key = (f, c["lib"], c["nt"], c["H"] % 16 == 0) if c["H"] in (45, 48, 160, 157) else None
        else:
            key = (f, c.get("kind"), base(kernels(c)[0]), c.get("onchip", True), c["D"] if f == "seqdec" else None,
                   c["C"] if f == "real_step" else None)
        if key is not None and key not in seen and (f == "lstm" or c["B"] == 50):
            seen.add(key)
            out.append(dict(c, B=50, row=0) if f == "lstm" else c)
    return out


POSITION_CASES = _position_cases()


def _readout_position_cases():
    """One readout case per compiled GRAD = true kernel (the lane kernel at every latent size, both matrix-core windows,
    the two-layer readout at both sizes), at T = 6, B = 50."""
    seen, out = set(), []
    for c in READOUT_CASES:
        k = kernels(c)[0]
        if k not in seen:
            seen.add(k)
            out.append(dict(c, T=T_MAIN, B=50, row=0, n=0, col=0, what="h", value="nan", sharp=False))
    return out


READOUT_POSITION_CASES = _readout_position_cases()
