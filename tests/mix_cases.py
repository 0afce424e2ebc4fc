"""The two-model mixture CRPS (libhode_mix.so): the GPU test table (CASES), which compiled kernels each case reaches
(kernels(), read by the no-GPU coverage guard in tests/test_mix_host.py), seeded inputs, and the float64 yardsticks -- the
per-element reference with its tolerance scale (the recipe of reference_checks.crps_oracle for a mixture of two
readouts) and a CPU stand-in with hode.mix.mixture_crps' contract.  A plain helper module."""
import collections

import torch

from oracle.evalmetrics import crps_field, crps_sorted

Case = collections.namedtuple("Case", "obs De Dm M Tn B weights biases per_component")

SIM_SHAPES = ((20, 4, 6), (40, 4, 8), (80, 4, 12))   # (obs, expert D, NeuralODE D) of the simulation scripts
LARGEST = (128, 128, 128, 21)                         # (obs, De, Dm, M): 163 840 B of LDS, all a workgroup has
FIRST_REFUSED = (128, 128, 128, 22)                   # 165 376 B


def _table():
    cases = []
    # the simulation shapes x ensemble size x weights x biases x output mode; B = 7 is ragged against every packing
    # (6 rows per workgroup at obs 20, 3 at obs 40: 63 rows)
    for obs, De, Dm in SIM_SHAPES:
        for M in (50, 10):
            for weights in (False, True):
                for biases in (False, True):
                    for per_component in (False, True):
                        cases.append(Case(obs, De, Dm, M, 9, 7, weights, biases, per_component))
    cases.append(Case(20, 4, 6, 10, 3, 21846, True, True, False))     # Tn * B = 65 538 rows > 65 535
    cases.append(Case(20, 4, 6, 10, 3, 21846, True, True, True))
    cases.append(Case(20, 4, 6, 1, 9, 7, True, True, False))          # M = 1: the absolute error
    cases.append(Case(20, 4, 6, 1, 9, 7, False, False, True))
    for obs in (1, 64, 65, 128):                                      # 8 rows / 2 rows / 1 row / 1 row per workgroup
        for per_component in (False, True):
            cases.append(Case(obs, 4, 6, 10, 5, 7, True, True, per_component))
    cases.append(Case(20, 4, 6, 128, 2, 7, True, True, False))        # M = 128: packing gives way to the LDS bound
    cases.append(Case(*LARGEST[:3], LARGEST[3], 2, 3, True, True, False))
    cases.append(Case(*LARGEST[:3], LARGEST[3], 2, 3, True, True, True))
    return cases


CASES = _table()


def case_id(c):
    return "obs%d_De%d_Dm%d_M%d_T%d_B%d_w%d_b%d_%s" % (c.obs, c.De, c.Dm, c.M, c.Tn, c.B, c.weights, c.biases,
                                                      "field" if c.per_component else "sum")


def kernels(case):
    return {"hode_mix::mix_crps_kernel"}


def inputs(c, seed):
    """CPU tensors of a case: h_e (Tn, M * B, De), h_m, truth, the two readouts and the (Tn, obs) weight tables (or None)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    i = collections.OrderedDict()
    i["h_e"], i["h_m"] = r(c.Tn, c.M * c.B, c.De), r(c.Tn, c.M * c.B, c.Dm)
    i["truth"] = r(c.Tn, c.B, c.obs)
    i["w_e"], i["w_m"] = r(c.obs, c.De) / c.De ** 0.5, r(c.obs, c.Dm) / c.Dm ** 0.5
    i["b_e"], i["b_m"] = (0.3 * r(c.obs), 0.3 * r(c.obs)) if c.biases else (None, None)
    i["g_e"], i["g_m"] = (1.2 * torch.rand(c.Tn, c.obs, generator=g), 1.2 * torch.rand(c.Tn, c.obs, generator=g)) \
        if c.weights else (None, None)
    return i


def mixture_values(h_e, h_m, n_members, w_e, b_e, w_m, b_m, g_e, g_m):
    """fp64 mixture values (Tn, M, B, obs) and the sum of the two weighted readout magnitudes (Tn, B, obs)."""
    Tn, MB, _ = h_e.shape
    B = MB // n_members
    vals, mag = 0.0, 0.0
    for h, w, b, g in ((h_e, w_e, b_e, g_e), (h_m, w_m, b_m, g_m)):
        h64, w64 = h.double().reshape(Tn, n_members, B, -1), w.double()
        b64 = b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)
        g64 = g.double()[:, None, :] if g is not None else torch.ones(Tn, 1, w.shape[0], dtype=torch.float64)
        vals = vals + g64[:, None] * (torch.einsum("tmbd,od->tmbo", h64, w64) + b64)
        mag = mag + g64.abs() * (torch.einsum("tmbd,od->tmbo", h64.abs(), w64.abs()).mean(1) + b64.abs())
    return vals, mag


def mix_oracle(h_e, h_m, truth, n_members, w_e, b_e, w_m, b_m, g_e, g_m):
    """fp64 CRPS field (Tn, B, obs) of the mixture and the per-element tolerance scale: reference_checks.crps_oracle's
    recipe (mean member distance to the truth plus the readout magnitude), with both models' weighted magnitudes."""
    vals, mag = mixture_values(h_e, h_m, n_members, w_e, b_e, w_m, b_m, g_e, g_m)
    ens = vals.permute(0, 2, 3, 1)                                          # (Tn, B, obs, M)
    y = truth.double()
    ref = torch.from_numpy(crps_sorted(y.numpy(), ens.numpy()))
    scale = (ens - y[..., None]).abs().mean(-1) + mag
    return ref, scale


def _pair(r):
    return (r[0], r[1]) if isinstance(r, (tuple, list)) else (r.weight, getattr(r, "bias", None))


def oracle_mixture_crps(h_e, h_m, truth, n_members, readout_e, readout_m, weight_e=None, weight_m=None, per_component=False):
    """CPU stand-in with hode.mix.mixture_crps' contract, scored in fp64 by oracle.evalmetrics.crps_field."""
    Tn, obs = truth.shape[0], truth.shape[-1]
    tab = lambda w: None if w is None else (w if torch.is_tensor(w) else torch.full((Tn, obs), float(w)))
    (w_e, b_e), (w_m, b_m) = _pair(readout_e), _pair(readout_m)
    cpu = lambda x: None if x is None else x.detach().cpu()
    vals, _ = mixture_values(cpu(h_e), cpu(h_m), n_members, cpu(w_e), cpu(b_e), cpu(w_m), cpu(b_m), cpu(tab(weight_e)),
                             cpu(tab(weight_m)))
    c = torch.from_numpy(crps_field(cpu(truth).double().numpy(), vals.permute(0, 2, 3, 1).numpy())).float().to(truth.device)
    return c if per_component else c.sum(-1)


def oracle_ensemble_crps(h, truth, n_members, weight=None, bias=None, per_component=False):
    """CPU stand-in with hode.crps.ensemble_crps' contract (member-major batch axis), as tests/test_evaluate.py builds it."""
    Tn, MB, Dv = h.shape
    M, B, obs = n_members, MB // n_members, truth.shape[-1]
    v = h.detach().cpu().reshape(Tn, M, B, Dv).double()
    vals = (v @ weight.detach().cpu().double().t() + (bias.detach().cpu().double() if bias is not None else 0.0)) \
        if weight is not None else v[..., :obs]
    c = torch.from_numpy(crps_field(truth.detach().cpu().double().numpy(), vals.permute(0, 2, 3, 1).numpy())).float().to(truth.device)
    return c if per_component else c.sum(-1)
