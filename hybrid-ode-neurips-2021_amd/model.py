"""Host-side mirror of the reference's ``model.py`` call surface for the hybrid-ODE hot path.

Same class names, constructor signatures, attribute names, parameter creation order and ``state_dict`` keys as the
reference (so ``run_simulation.py`` / ``training_utils.py`` style drivers and reference checkpoints drop in), but the
latent ODE is integrated by the gfx950 kernels of ``libhode.so`` (``hode.odeint``) instead of ``torchdiffeq``:

    reference                                  here
    RocheODE            model.py:446-555       RocheODE            (+ ``hode_solve``: kernel dispatch)
    RocheExpertDecoder  model.py:1030-1121     RocheExpertDecoder  (forward = set_action -> hode.odeint -> readout)
    EncoderLSTM         model.py:383-440       EncoderLSTM
    GaussianReparam / ExponentialPrior / StandardNormalPrior  model.py:18-45
    VariationalInference model.py:1124-1214    VariationalInference

    EncoderLSTMReal / RocheODEReal / DecoderReal / VariationalInferenceReal  model.py:180-242, 570-657, 772-862, 1217-1261
    GRUODECell / DecoderRealBenchmark ("tlstm", "gruode" baselines)         model.py:865-966  (hode.seqdec kernels)
    NeuralODEReal / NeuralODEReal2nd ("neural", "2nd" baselines)           model.py:660-769  (hode.neural_real kernels)
    EncoderPlanarLSTM / VariationalInferenceFlow (planar-flow posterior)   model.py:48-153, 1299-1380 (hode.flow kernels)
    LSTMBaseline (sequence-to-sequence LSTM forecaster)                    model.py:322-380  (hode.lstm.lstm_sequence)

The Sylvester flows of the reference's ``flow.py`` (unused by its ``model.py``) are in ``flow.Sylvester``,
``flow.TriangularSylvester`` and ``flow.sylvester_chain`` (libhode_sylvester.so).  ``EncoderSylvesterLSTM`` is
the posterior they were written for (LHM-SNF; no counterpart in the reference's ``model.py``): ``VariationalInferenceFlow``
and ``training_utils.evaluate_flow`` take it in ``EncoderPlanarLSTM``'s place (libhode_snf.so).
"""

from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

import flow as flows
import hode
import sim_config
from global_config import DTYPE, get_device

_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


class GaussianReparam:
    """Diagonal-Gaussian posterior helpers (reference model.py:18-31)."""

    @staticmethod
    def reparameterize(mu, log_var):
        sigma = torch.exp(0.5 * log_var)
        return torch.randn_like(sigma) * sigma + mu

    @staticmethod
    def log_density(mu, log_var, z):
        sigma = torch.exp(0.5 * log_var)
        lp = -((z - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - _LOG_SQRT_2PI
        return lp.sum(dim=-1)


class _AnalyticKL(torch.autograd.Function):
    """mean_b( -0.5 sum_d(1 + log_var - mu^2 - exp(log_var)) ) (model.py:1188) with a hand-written backward: 8 launches
    instead of the 18 the expression and its autograd graph take -- on a (B, D) operand every one of them is launch latency."""

    @staticmethod
    def forward(ctx, mu, log_var):
        e = torch.exp(log_var)
        ctx.save_for_backward(mu, e)
        B, D = mu.shape
        return (torch.sum(torch.addcmul(log_var, mu, mu, value=-1.0) - e) + float(B * D)) * (-0.5 / B)

    @staticmethod
    def backward(ctx, g):
        mu, e = ctx.saved_tensors
        c = g / mu.shape[0]
        return c * mu, (e - 1.0) * (0.5 * c)


def analytic_kl(mu, log_var):
    if mu.is_cuda and mu.dim() == 2:
        return _AnalyticKL.apply(mu, log_var)
    return torch.mean(-0.5 * torch.sum(1 + log_var - mu ** 2 - log_var.exp(), dim=1), dim=0)


class StandardNormalPrior:
    @staticmethod
    def log_density(z):
        return (-0.5 * z ** 2 - _LOG_SQRT_2PI).sum(dim=-1)


class ExponentialPrior:
    """Exponential(rate 100) prior on the initial latents (reference model.py:41-45)."""

    rate = 100.0

    @staticmethod
    def log_density(z):
        return (math.log(ExponentialPrior.rate) - ExponentialPrior.rate * z).sum(dim=-1)


class EncoderLSTM(nn.Module, GaussianReparam):
    """Masked, reverse-time single-layer LSTM over the observation window -> (mu, log_var) of z0 (model.py:383-440)."""

    def __init__(self, input_dim, hidden_dim, output_dim, normalize=True, device=None):
        super().__init__()
        self.device = get_device() if device is None else device
        self.hidden_dim = hidden_dim
        self.normalize = normalize
        self.model_name = "LSTMEncoder"
        # creation order lstm -> lin -> log_var fixes both the seeded init and the state_dict key order
        self.lstm = nn.LSTM(input_dim, hidden_dim).to(self.device)
        self.lin = nn.Linear(hidden_dim, output_dim).to(self.device)
        self.log_var = nn.Linear(hidden_dim, output_dim).to(self.device)

    def final_hidden(self, x, a, mask):
        """h after walking t = T-1 .. 0 on cat(x,a)*cat(mask,1) (reference model.py:415-422).

        HIP tensors: the fp32-MFMA window kernel (``hode.lstm``: mask/concat fused, h and c stay on chip, BPTT kernel
        for the backward).  CPU tensors (host-logic tests): one ``nn.LSTM`` sequence call on the flipped, pre-masked
        input -- the reference's own operator, same arithmetic as its T single-step calls."""
        if x.dim() == 3 and x.shape[1] == 1:
            raise RuntimeError("EncoderLSTM: batch size 1 is not supported (the reference's x.squeeze() drops the batch axis)")
        p = self.lstm
        if x.is_cuda:
            from hode.lstm import lstm_encode
            return lstm_encode(x, a, mask, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, reverse=True)
        seq = torch.cat([x * mask, a], dim=-1).flip(0)
        _, (h, _) = p(seq)
        return h[0]

    def forward(self, x, a, mask):
        h = self.final_hidden(x, a, mask)
        if h.is_cuda:   # same numbers as nn.Linear; the weight gradient is a split product over the patients (_rows_tn)
            mu = _TallLinear.apply(h, self.lin.weight, self.lin.bias)
            log_var = _TallLinear.apply(h, self.log_var.weight, self.log_var.bias)
        else:
            mu, log_var = self.lin(h), self.log_var(h)
        if self.normalize:
            mu = torch.exp(mu) / 10
            log_var = log_var - 5.0
        return mu, log_var


class EncoderPlanarLSTM(nn.Module):
    """EncoderLSTM's window encoder with amortized planar-flow parameters (reference model.py:48-153): forward returns
    (mu, log_var, u (B, K, D, 1), w (B, K, 1, D), b (B, K, 1, 1)); reparameterize draws z0 ~ N(mu, exp(log_var)), runs the
    K planar flows and the exp(z - 5) output layer.

    HIP tensors: the window goes through the LSTM kernels (``hode.lstm``) and the five heads are one product over the
    concatenated weights.  ``reparameterize`` is the reference's per-draw call surface in eager arithmetic; the training
    and evaluation paths (``VariationalInferenceFlow.loss``, ``training_utils.evaluate_flow``) draw all samples at once
    through the fused kernel pair of ``hode.flow``."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_flows, normalize=True, device=None):
        super().__init__()
        self.device = get_device() if device is None else device
        self.hidden_dim = hidden_dim
        self.normalize = normalize
        self.model_name = "PlanarLSTMEncoder"
        # creation order lstm -> lin -> log_var -> amor_u -> amor_w -> amor_b -> flow_k: seeded init and state_dict keys
        self.lstm = nn.LSTM(input_dim, hidden_dim).to(self.device)
        self.lin = nn.Linear(hidden_dim, output_dim).to(self.device)
        self.log_var = nn.Linear(hidden_dim, output_dim).to(self.device)
        self.q_z_nn_output_dim = hidden_dim
        self.num_flows = num_flows
        self.z_size = output_dim
        self.log_det_j = 0.0
        self.amor_u = nn.Linear(self.q_z_nn_output_dim, self.num_flows * self.z_size).to(self.device)
        self.amor_w = nn.Linear(self.q_z_nn_output_dim, self.num_flows * self.z_size).to(self.device)
        self.amor_b = nn.Linear(self.q_z_nn_output_dim, self.num_flows).to(self.device)
        for k in range(self.num_flows):
            self.add_module("flow_" + str(k), flows.Planar().to(self.device))

    final_hidden = EncoderLSTM.final_hidden

    def _heads(self):
        return (self.lin, self.log_var, self.amor_u, self.amor_w, self.amor_b)

    def forward(self, x, a, mask):
        h = self.final_hidden(x, a, mask)
        B, D, K = h.shape[0], self.z_size, self.num_flows
        if h.is_cuda:   # one product over the concatenated heads; gradients reach every head through the cat
            heads = self._heads()
            out = _TallLinear.apply(h, torch.cat([m.weight for m in heads]), torch.cat([m.bias for m in heads]))
            mu, log_var, u, w, b = torch.split(out, [D, D, K * D, K * D, K], dim=1)
        else:
            mu, log_var, u, w, b = (m(h) for m in self._heads())
        u = u.reshape(B, K, D, 1)
        w = w.reshape(B, K, 1, D)
        b = b.reshape(B, K, 1, 1)
        if self.normalize:
            mu = torch.exp(mu) / 10
            log_var = log_var - 5.0
        return mu, log_var, u, w, b

    def reparameterize(self, mu, log_var, u, w, b):
        log_det_j = 0.0
        z = [GaussianReparam.reparameterize(mu, log_var)]
        for k in range(self.num_flows):
            z_k, log_det_jacobian = getattr(self, "flow_" + str(k))(z[k], u[:, k, :, :], w[:, k, :, :], b[:, k, :, :])
            z.append(z_k)
            log_det_j += log_det_jacobian
        z_exp = torch.exp(z_k - 5.0)
        log_det_j += torch.sum(z_k - 5.0, dim=-1)
        return mu, log_var, z_exp, log_det_j, z[0]

    def log_density(self, mu, log_var, z_1, log_det_j, z0):
        return GaussianReparam.log_density(mu, log_var, z0) - log_det_j

    def flow_draws(self, mu, log_var, u, w, b, eps):
        """Eager (CPU) restatement of S reparameterize calls with given draws eps (S, B, D): returns z_out (S, B, D),
        log_det_j (S, B), z0 (S, B, D) -- the reference's per-draw arithmetic on S * B rows."""
        S, B, D = eps.shape
        z0 = eps * torch.exp(0.5 * log_var) + mu
        z = z0.reshape(S * B, D)
        rep = lambda t: t.unsqueeze(0).expand((S,) + tuple(t.shape)).reshape((S * B,) + tuple(t.shape[1:]))
        log_det_j = 0.0
        for k in range(self.num_flows):
            z, ld = getattr(self, "flow_" + str(k))(z, rep(u[:, k]), rep(w[:, k]), rep(b[:, k]))
            log_det_j = log_det_j + ld
        log_det_j = log_det_j + torch.sum(z - 5.0, dim=-1)
        return torch.exp(z - 5.0).reshape(S, B, D), log_det_j.reshape(S, B), z0

    def posterior_sample(self, encoder_out, eps, s_kl=1):
        """(z_out (S, B, D), kl (B,)) of the draws eps against the Exponential(100) prior: the fused kernel pair of
        ``hode.flow`` on HIP tensors, ``flow_draws`` on CPU tensors."""
        mu, log_var, u, w, b = encoder_out
        if mu.is_cuda:
            from hode.flow import planar_flow_sample
            return planar_flow_sample(mu, log_var, u, w, b, eps, s_kl)
        return _eager_posterior_sample(self, encoder_out, eps, s_kl)


def _eager_posterior_sample(encoder, encoder_out, eps, s_kl):
    """``posterior_sample`` of a flow encoder in eager arithmetic: its ``flow_draws`` and ``log_density`` against the
    Exponential(100) prior, the mean over the draws s_kl .. of log q - log p."""
    z_out, log_det_j, z0 = encoder.flow_draws(*encoder_out, eps)
    log_q = encoder.log_density(encoder_out[0], encoder_out[1], z_out, log_det_j, z0)
    return z_out, torch.mean((log_q - ExponentialPrior.log_density(z_out))[s_kl:], dim=0)


class EncoderSylvesterLSTM(nn.Module):
    """EncoderLSTM's window encoder with amortized Sylvester-flow parameters (LHM-SNF; van den Berg et al. 2018).  The
    reference has the flows (``flow.py:62-219``) but no encoder that uses them; this one follows its ``EncoderPlanarLSTM``
    (model.py:48-153) head for head.  ``flow_type`` is "triangular" (Q the identity / the flip, alternating) or
    "householder" (Q a product of ``num_householder`` reflections, default D); the Bjorck-orthogonalised "orthogonal"
    type is not implemented.

    forward returns the raw heads ``(mu, log_var, full_d (B, K, D, D), diag1, diag2, bias (B, K, D), v (B, K, H, D) or
    None)``; masks, tanh diagonals and the Householder product are ``flow.sylvester_flow_parameters``.  HIP tensors: the
    window goes through the LSTM kernels and the heads are one product over the concatenated weights; the training and
    evaluation paths draw all samples at once through the fused kernel pair of ``hode.snf``
    (``flow.sylvester_posterior_sample``), where r1, r2 and Q never leave the chip.  ``reparameterize``, ``log_density``
    and ``flow_draws`` are the per-draw surface of the planar encoder, with the same return shapes."""

    FLOW_TYPES = ("triangular", "householder")

    def __init__(self, input_dim, hidden_dim, output_dim, num_flows, flow_type="triangular", num_householder=None,
                 normalize=True, device=None):
        super().__init__()
        if flow_type not in self.FLOW_TYPES:
            raise ValueError("EncoderSylvesterLSTM: flow_type %r not in %r (the \"orthogonal\" type is not implemented)"
                             % (flow_type, self.FLOW_TYPES))
        self.device = get_device() if device is None else device
        self.hidden_dim = hidden_dim
        self.normalize = normalize
        self.flow_type = flow_type
        self.model_name = "TriangularSylvesterLSTMEncoder" if flow_type == "triangular" else "HouseholderSylvesterLSTMEncoder"
        # creation order lstm -> lin -> log_var -> amor_d -> amor_diag1 -> amor_diag2 -> amor_b -> [amor_q] -> flow_k
        self.lstm = nn.LSTM(input_dim, hidden_dim).to(self.device)
        self.lin = nn.Linear(hidden_dim, output_dim).to(self.device)
        self.log_var = nn.Linear(hidden_dim, output_dim).to(self.device)
        self.q_z_nn_output_dim = hidden_dim
        self.num_flows = num_flows
        self.z_size = output_dim
        self.num_householder = 0 if flow_type == "triangular" else (output_dim if num_householder is None else int(num_householder))
        if flow_type == "householder" and self.num_householder < 1:
            raise ValueError("EncoderSylvesterLSTM: num_householder %d must be >= 1" % self.num_householder)
        self.log_det_j = 0.0
        K, D = self.num_flows, self.z_size
        self.amor_d = nn.Linear(self.q_z_nn_output_dim, K * D * D).to(self.device)
        self.amor_diag1 = nn.Linear(self.q_z_nn_output_dim, K * D).to(self.device)
        self.amor_diag2 = nn.Linear(self.q_z_nn_output_dim, K * D).to(self.device)
        self.amor_b = nn.Linear(self.q_z_nn_output_dim, K * D).to(self.device)
        if self.num_householder:
            self.amor_q = nn.Linear(self.q_z_nn_output_dim, K * self.num_householder * D).to(self.device)
        for k in range(K):
            mod = flows.TriangularSylvester(D) if flow_type == "triangular" else flows.Sylvester(D)
            self.add_module("flow_" + str(k), mod.to(self.device))

    final_hidden = EncoderLSTM.final_hidden

    def _heads(self):
        heads = (self.lin, self.log_var, self.amor_d, self.amor_diag1, self.amor_diag2, self.amor_b)
        return heads + ((self.amor_q,) if self.num_householder else ())

    def forward(self, x, a, mask):
        h = self.final_hidden(x, a, mask)
        B, D, K, H = h.shape[0], self.z_size, self.num_flows, self.num_householder
        heads = self._heads()
        if h.is_cuda:   # one product over the concatenated heads; gradients reach every head through the cat
            out = _TallLinear.apply(h, torch.cat([m.weight for m in heads]), torch.cat([m.bias for m in heads]))
            outs = torch.split(out, [m.out_features for m in heads], dim=1)
        else:
            outs = tuple(m(h) for m in heads)
        mu, log_var = outs[0], outs[1]
        full_d = outs[2].reshape(B, K, D, D)
        diag1, diag2, bias = (t.reshape(B, K, D) for t in outs[3:6])
        v = outs[6].reshape(B, K, H, D) if H else None
        if self.normalize:
            mu = torch.exp(mu) / 10
            log_var = log_var - 5.0
        return mu, log_var, full_d, diag1, diag2, bias, v

    def reparameterize(self, mu, log_var, full_d, diag1, diag2, bias, v=None):
        r1, r2, q, perm = flows.sylvester_flow_parameters(full_d, diag1, diag2, v)
        log_det_j = 0.0
        z = [GaussianReparam.reparameterize(mu, log_var)]
        for k in range(self.num_flows):
            mod = getattr(self, "flow_" + str(k))
            if q is None:
                z_k, log_det_jacobian = mod._forward(z[k], r1[:, k], r2[:, k], bias[:, k], perm[k], sum_ldj=True)
            else:
                z_k, log_det_jacobian = mod(z[k], r1[:, k], r2[:, k], q[:, k], bias[:, k], sum_ldj=True)
            z.append(z_k)
            log_det_j += log_det_jacobian
        z_exp = torch.exp(z_k - 5.0)
        log_det_j += torch.sum(z_k - 5.0, dim=-1)
        return mu, log_var, z_exp, log_det_j, z[0]

    def log_density(self, mu, log_var, z_1, log_det_j, z0):
        return GaussianReparam.log_density(mu, log_var, z0) - log_det_j

    def flow_draws(self, mu, log_var, full_d, diag1, diag2, bias, v, eps):
        """S reparameterize calls with given draws eps (S, B, D) as one ``flow.sylvester_chain`` call: returns z_out
        (S, B, D), log_det_j (S, B), z0 (S, B, D)."""
        r1, r2, q, perm = flows.sylvester_flow_parameters(full_d, diag1, diag2, v)
        z0 = eps * torch.exp(0.5 * log_var) + mu
        z, log_det_j = flows.sylvester_chain(z0, r1, r2, bias, q, perm)
        return torch.exp(z - 5.0), log_det_j + torch.sum(z - 5.0, dim=-1), z0

    def posterior_sample(self, encoder_out, eps, s_kl=1):
        """(z_out (S, B, D), kl (B,)) of the draws eps against the Exponential(100) prior: the fused kernel pair of
        ``hode.snf`` on HIP tensors, the same arithmetic eagerly on CPU tensors."""
        return flows.sylvester_posterior_sample(*encoder_out, eps, s_kl)


dose_schedule_index = hode.solver.dose_schedule_index


_THETA_FIELDS = sim_config.RochConfig._fields  # == parameter creation order of the reference (model.py:468-482)


STEP_CONTROLS = ("batch", "patient")


def _step_control(module, options):
    """The dopri5 step control of this call: ``options["step_control"]`` if given, else the module's ``step_control``
    attribute, else "batch" (torchdiffeq's: one error norm and one dt for the whole batch).  "patient" gives every patient a
    controller of its own (``hode.patient_dopri5``); anything else is refused."""
    control = options.pop("step_control", getattr(module, "step_control", "batch"))
    if control not in STEP_CONTROLS:
        raise hode.HodeConfigError("hode: step_control %r is not one of %s" % (control, ", ".join(map(repr, STEP_CONTROLS))))
    return control


def _refuse_patient_step_control(module, options):
    """For the rhs families without per-patient kernels: names what serves ``step_control = "patient"``."""
    if _step_control(module, options) == "patient":
        from hode import _dopri5_pp_lib as PL
        raise hode.HodeConfigError("hode: %s has no per-patient step control; step_control='patient' serves %s with "
                                   "method='dopri5'" % (type(module).__name__, PL.sizes_text()))


class _RochePatientDopri5(torch.autograd.Function):
    """h = odeint(RocheODE, y0, t, method="dopri5") with per-patient step control: the two launches of
    ``hode.patient_dopri5``.  Gradients for y0, theta, w, b; none for t, dosage, dose_times (their .grad stays None).  Every
    step size is a constant in the backward, dt_0 included."""

    @staticmethod
    def forward(ctx, y0, theta, w, b, t, dosage, dose_times, rtol, atol, ablate, grad_enabled=True):
        from hode import patient_dopri5 as PP
        f32c = hode.solver._f32c
        y0c, thc, tc, dosc, dtc = f32c(y0), f32c(theta), f32c(t), f32c(dosage), f32c(dose_times)
        wc = f32c(w) if w is not None else None
        bc = f32c(b) if b is not None else None
        # `needs_input_grad` reflects requires_grad, not the grad mode, and inside forward() grad mode is always off: the
        # caller samples it before .apply() (as hode.adaptive.roche_dopri5 does).  Nothing to differentiate: no tape at all.
        no_tape = not (grad_enabled and any(ctx.needs_input_grad[:4]))
        h, ws, stats = PP.patient_dopri5_forward(y0c, thc, wc, bc, tc, dosc, dtc, rtol=rtol, atol=atol, ablate=ablate,
                                                 no_tape=no_tape)
        ctx.save_for_backward(h, thc, wc if wc is not None else thc, bc if bc is not None else thc, tc, dosc, dtc, y0c, ws,
                              stats["n_accepted"])
        ctx.meta = (float(rtol), float(atol), bool(ablate), w is not None, int(stats["max_steps"]))
        return h

    @staticmethod
    def backward(ctx, grad_h):
        from hode import patient_dopri5 as PP
        h, thc, wc, bc, tc, dosc, dtc, y0c, ws, n_accepted = ctx.saved_tensors
        rtol, atol, ablate, has_w, steps = ctx.meta
        need_th = bool(ctx.needs_input_grad[1])
        gy0, gth, gw, gb = PP.patient_dopri5_backward(y0c, thc, wc if has_w else None, bc if has_w else None, tc, dosc, dtc, h, ws,
                                                      n_accepted, steps, hode.solver._f32c(grad_h), rtol=rtol, atol=atol,
                                                      ablate=ablate, need_theta=need_th)
        return gy0, gth, gw, gb, None, None, None, None, None, None, None


class _RocheDoseGrad(torch.autograd.Function):
    """h = odeint(RocheODE, y0, t, method) on a fixed grid with a gradient for the dosage as well (``RocheODE.dose_grad``).
    Forward: the existing lane-per-patient forward, ``hode.roche_solve(..., lanes_per_patient=1)``, so h is bit for bit what
    that call returns.  Backward: ``hode.dose.dose_backward`` (libhode_dose.so).  Gradients for y0, theta, w, b and dosage;
    none for t and dose_times (their .grad stays None)."""

    @staticmethod
    def forward(ctx, y0, theta, w, b, t, dosage, dose_times, method, ablate, perturb, check_finite, library):
        f32c = hode.solver._f32c
        thc, tc, dosc, dtc = f32c(theta), f32c(t), f32c(dosage), f32c(dose_times)
        wc = f32c(w) if w is not None else None
        bc = f32c(b) if b is not None else None
        with torch.no_grad():  # detached inputs: the forward keeps nothing for a backward of its own
            h = hode.roche_solve(f32c(y0), thc, wc, bc, tc, dosc, dtc, method=method, ablate=ablate, perturb=perturb,
                                 lanes_per_patient=1, check_finite=check_finite, library=library)
        ctx.save_for_backward(h, thc, wc if wc is not None else thc, bc if bc is not None else thc, tc, dosc, dtc)
        ctx.meta = (method, bool(ablate), bool(perturb), w is not None)
        return h

    @staticmethod
    def backward(ctx, grad_h):
        from hode import dose
        h, thc, wc, bc, tc, dosc, dtc = ctx.saved_tensors
        method, ablate, perturb, has_w = ctx.meta
        need_th = bool(ctx.needs_input_grad[1])
        gy0, gth, gw, gb, gdos = dose.dose_backward(h, thc, wc if has_w else None, bc if has_w else None, tc, dosc, dtc,
                                                    hode.solver._f32c(grad_h), method=method, ablate=ablate, perturb=perturb,
                                                    need_theta=need_th)
        return gy0, gth, gw, gb, None, gdos, None, None, None, None, None, None


class RocheODE(nn.Module):
    """Expert PK/PD block + ``tanh(W y + b)`` learned block; ``forward(t, y)`` is the rhs (model.py:446-555)."""

    def __init__(self, latent_dim, action_dim, t_max, step_size, ablate=False, device=None, dtype=DTYPE):
        super().__init__()
        assert action_dim == 1
        self.action_dim = action_dim
        self.latent_dim = int(latent_dim)
        self.expert_dim = 4
        self.ml_dim = self.latent_dim - self.expert_dim
        self.expanded = self.ml_dim > 0
        self.ablate = ablate
        self.device = get_device() if device is None else device
        self.t_max = t_max
        self.step_size = step_size
        cfg = sim_config.RochConfig()
        for name in _THETA_FIELDS:
            setattr(self, name, nn.Parameter(torch.tensor(getattr(cfg, name), device=self.device, dtype=dtype)))
        if self.ablate:
            self.theta_1 = nn.Parameter(torch.tensor(1, device=self.device, dtype=dtype))
            self.theta_2 = nn.Parameter(torch.tensor(2, device=self.device, dtype=dtype))
        if self.expanded:
            self.ml_net = nn.Sequential(nn.Linear(self.latent_dim, self.ml_dim), nn.Tanh()).to(self.device)
        else:
            self.ml_net = nn.Identity().to(self.device)
        self.times = None
        self.dosage = None
        # tuning knobs of the kernel dispatch (not part of the reference surface)
        self.lanes_per_patient = 0
        self.check_finite = False
        # dopri5 only: "batch" = torchdiffeq's controller (one error norm, one dt for the whole batch); "patient" = a
        # controller per patient (hode.patient_dopri5); options["step_control"] of hode.odeint overrides it for one call
        self.step_control = "batch"
        # fixed-grid methods only: True lets a gradient reach the treatment -- set_action takes the dosage from an action
        # that requires grad differentiably, and the solve's backward fills dosage.grad (hode.dose, libhode_dose.so)
        self.dose_grad = False

    # -- dose schedule -------------------------------------------------------------------------------------
    def set_action(self, action):
        """dosage (B,) = max over time; times (B, K) = non-zero grid indices * step_size.  Vectorised: the
        reference's per-patient Python loop (model.py:500-507) costs 0.19 s at 10k patients.

        Finding the dose indices needs the dose count K on the host (one device read-back + ``nonzero``): three host
        synchronisations in the middle of a training step, behind which the host has to enqueue the rest of the step while
        the GPU waits (bench.py ``full_training_step.host_enqueue_ms``).  Two sync-free routes: a batch source that knows
        its data (``hode.batches.DeviceFolds``) attaches the precomputed schedule to the action tensor
        (``action.hode_schedule = (dosage, dose_index)``), and a tensor OBJECT that was analysed before and has not been written to
        since (same object, same version counter) reuses its result.

        With ``dose_grad`` on and an action that requires grad, the dosage is always taken from the action by ``torch.max``
        (as the reference does: the gradient goes to ONE entry of the action per patient, also among equal doses); the two
        routes may still supply the dose indices."""
        track = bool(getattr(self, "dose_grad", False)) and action.requires_grad
        sched = getattr(action, "hode_schedule", None)
        if sched is not None:
            self.dosage, idx = sched
            if track:
                self.dosage = torch.max(action[..., 0], dim=0)[0]
            self.times = idx * self.step_size
            return
        # identity, not address: the cache keeps the tensor alive, so its storage cannot be recycled for another batch
        cached = getattr(self, "_schedule_cache", None)
        if cached is not None and cached[0] is action and cached[1] == action._version:
            self.dosage, self.times = cached[2], cached[3] * self.step_size
            if track:
                self.dosage = torch.max(action[..., 0], dim=0)[0]
            return
        dosage, idx = dose_schedule_index(action)
        self.dosage, self.times = dosage, idx * self.step_size
        self._schedule_cache = (action, action._version, dosage.detach() if track else dosage, idx)

    def dose_at_time(self, t):
        on = t >= self.times
        return self.dosage * torch.sum(torch.exp(self.kel * (self.times - t) * on) * on, dim=-1)

    # -- rhs as a torch function (API parity; the solver never calls this) ----------------------------------
    def forward(self, t, y):
        dis, ir, imm, dose2 = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
        if self.ablate:
            cols = [ir, -1.0 * dis * self.theta_1, dose2, -1.0 * imm * self.theta_2]
        else:
            dose = self.dose_at_time(t)
            irp = ir ** self.HillPatho
            cols = [
                dis * self.k_disprog - dis * imm ** self.HillCure * self.k_discure_immunity - dis * ir * self.k_discure_immunereact,
                dis * self.k_immune_disease - ir * self.k_immune_off + dis * ir * self.k_immune_feedback
                + (irp * self.emax_patho) / (self.ec50_patho ** self.HillPatho + irp) - dose2 * ir * self.k_dexa,
                ir * self.k_immunity,
                self.kel * dose - self.kel * dose2,
            ]
        out = torch.stack(cols, dim=-1)
        return torch.cat([out, self.ml_net(y)], dim=-1) if self.expanded else out

    # -- kernel dispatch (what hode.odeint calls) -----------------------------------------------------------
    def theta_vector(self):
        names = list(_THETA_FIELDS) + (["theta_1", "theta_2"] if self.ablate else [])
        return hode.solver.pack_theta([getattr(self, n) for n in names], self.device)

    def hode_solve(self, y0, t, rtol, atol, method, options):
        if self.times is None:
            raise RuntimeError("RocheODE: call set_action(a) before integrating")
        w = self.ml_net[0].weight if self.expanded else None
        b = self.ml_net[0].bias if self.expanded else None
        control = _step_control(self, options)  # the fixed-grid methods ignore it
        if self.dose_grad:
            from hode import dose
            if method == "dopri5":
                raise hode.HodeConfigError("hode: RocheODE.dose_grad serves the fixed-grid methods euler / midpoint / rk4; "
                                           "method='dopri5' (step_control=%r) has no dose gradient" % (control,))
            dose.check_domain(self.latent_dim)  # names the sizes held and libhode_dose.so; nothing is loaded or launched before
            if self.dosage.requires_grad:
                from hode import substep
                perturb = bool(options.pop("perturb", False))
                theta = self.theta_vector()
                times = self.times.reshape(y0.shape[0], -1).to(torch.float32)
                return substep.solve_with_step_size(
                    lambda grid: _RocheDoseGrad.apply(y0, theta, w, b, grid, self.dosage, times, method, bool(self.ablate), perturb,
                                                      bool(self.check_finite), None),
                    t, options.pop("step_size", None))
        if method == "dopri5" and control == "patient":
            from hode import patient_dopri5
            patient_dopri5.check_domain(self.latent_dim)  # names the sizes held; nothing is loaded or launched before
            return _RochePatientDopri5.apply(y0, self.theta_vector(), w, b, t, self.dosage,
                                             self.times.reshape(y0.shape[0], -1).to(torch.float32), rtol, atol, bool(self.ablate),
                                             torch.is_grad_enabled())
        from hode import _roche_dims_lib as RL
        held = RL.DIMS + (RL.LIBHODE_DP_DIMS if method == "dopri5" else RL.LIBHODE_RK_DIMS)
        if self.latent_dim not in held:
            raise hode.HodeConfigError("hode: RocheODE with method=%r is compiled for latent dimensions %s (got %d); "
                                       "there is no torch-eager path in the product"
                                       % (method, RL.sizes_text(method == "dopri5"), self.latent_dim))
        library = RL.roche_solver_library(self.latent_dim)
        if method == "dopri5":
            from hode import adaptive
            return adaptive.roche_dopri5(y0, self.theta_vector(), w, b, t, self.dosage, self.times, rtol=rtol, atol=atol,
                                         ablate=self.ablate, library=library)
        from hode import substep
        perturb = bool(options.pop("perturb", False))
        theta = self.theta_vector()
        return substep.solve_with_step_size(
            lambda grid: hode.roche_solve(y0, theta, w, b, grid, self.dosage, self.times, method=method, ablate=self.ablate,
                                          perturb=perturb, lanes_per_patient=self.lanes_per_patient,
                                          check_finite=self.check_finite, library=library),
            t, options.pop("step_size", None))


class NeuralODE(nn.Module):
    """Pure neural rhs ``tanh(W2 tanh(W1 [y, Dose(t)] + b1) + b2)`` with an impulse dose (model.py:969-1026)."""

    def __init__(self, latent_dim, action_dim, t_max, step_size, device=None, dtype=DTYPE):
        super().__init__()
        assert action_dim == 1
        self.action_dim = action_dim
        self.latent_dim = int(latent_dim)
        self.expert_dim = 4
        self.ml_dim = self.latent_dim
        self.device = get_device() if device is None else device
        self.t_max, self.step_size = t_max, step_size
        self.kel = nn.Parameter(torch.tensor(sim_config.RochConfig().kel, device=self.device, dtype=dtype))  # unused by forward
        d = self.latent_dim
        self.ml_net = nn.Sequential(nn.Linear(d + 1, d * 10), nn.Tanh(), nn.Linear(d * 10, d), nn.Tanh()).to(self.device)
        self.times = None
        self.dosage = None

    set_action = RocheODE.set_action

    def dose_at_time(self, t):
        return self.dosage * torch.sum(self.times == t, dim=-1)

    def forward(self, t, y):
        return self.ml_net(torch.cat([y, self.dose_at_time(t)[:, None]], dim=-1))

    def hode_solve(self, y0, t, rtol, atol, method, options):
        if self.times is None:
            raise RuntimeError("NeuralODE: call set_action(a) before integrating")
        _refuse_patient_step_control(self, options)
        from hode import neural
        if method == "dopri5":
            from hode import adaptive
            if self.latent_dim not in adaptive.NEURAL_DIMS and self.latent_dim not in adaptive.NEURAL_ODD_DIMS:
                raise hode.HodeConfigError("hode: NeuralODE with method='dopri5' is compiled for latent dimensions %s "
                                           "(libhode.so) and %s (libhode_neural_odd.so) (got %d); "
                                           "there is no torch-eager path in the product"
                                           % (", ".join(str(d) for d in adaptive.NEURAL_DIMS),
                                              ", ".join(str(d) for d in adaptive.NEURAL_ODD_DIMS), self.latent_dim))
            # the reference's default for --method=neural (sim_config.py:50): fused MFMA attempt kernels
            return adaptive.neural_dopri5(y0, self.ml_net[0].weight, self.ml_net[0].bias, self.ml_net[2].weight,
                                          self.ml_net[2].bias, t, self.dosage, self.times, rtol=rtol, atol=atol)
        from hode import substep
        perturb = bool(options.pop("perturb", False))
        return substep.solve_with_step_size(
            lambda grid: neural.neural_solve(y0, self.ml_net[0].weight, self.ml_net[0].bias, self.ml_net[2].weight,
                                             self.ml_net[2].bias, grid, self.dosage, self.times, method=method, perturb=perturb),
            t, options.pop("step_size", None))


class RocheExpertDecoder(nn.Module):
    """z0 -> latent trajectory h (T,B,D) on the observation grid -> linear readout x_hat (model.py:1030-1121)."""

    def __init__(self, obs_dim, latent_dim, action_dim, t_max, step_size, roche=True, ablate=False, method="dopri5",
                 ode_step_size=None, device=None, dtype=DTYPE):
        super().__init__()
        self.time_dim = int(t_max / step_size)
        self.obs_dim, self.latent_dim, self.action_dim = obs_dim, latent_dim, action_dim
        self.t_max, self.step_size = t_max, step_size
        self.roche, self.ablate = roche, ablate
        self.model_name = ("ExpertDecoder" if latent_dim == 4 else "HybridDecoder") if roche else "NeuralODEDecoder"
        if ablate:
            self.model_name += "Ablate"
            print("Running ablation study")
        self.device = get_device() if device is None else device
        self.t = torch.arange(0, t_max + step_size, step_size, device=self.device, dtype=dtype)
        self.options = {"method": method, "rtol": 1e-7, "atol": 1e-8}
        # readout first, then the ode: same parameter creation order as the reference (seeded-init parity)
        self.output_function = nn.Sequential(nn.Linear(latent_dim, obs_dim, bias=True)).to(self.device)
        if roche:
            self.ode = RocheODE(latent_dim, action_dim, t_max, step_size, ablate=ablate, device=self.device)
        else:
            self.ode = NeuralODE(latent_dim, action_dim, t_max, step_size, self.device)
        self._odeint = hode.odeint  # tests swap in the CPU oracle here; the product path never does

    def latent(self, init, a):
        """Latent trajectory h (T, B, D) only."""
        self.ode.set_action(a)
        return self._odeint(self.ode, init, self.t, rtol=self.options["rtol"], atol=self.options["atol"],
                            method=self.options["method"])

    def forward(self, init, a):
        h = self.latent(init, a)
        return self.output_function(h), h

    def fused_likelihood_ok(self, x):
        from hode import readout
        return x.is_cuda and self._odeint is hode.odeint and readout.supported(self.latent_dim, self.obs_dim)

    def masked_sse(self, h, x, mask):
        """sum((x - output_function(h))^2 * mask) / B in one fused pass (x_hat never hits HBM)."""
        from hode import readout
        lin = self.output_function[0]
        return readout.masked_sse_readout(h, x, mask, lin.weight, lin.bias)


class EncoderLSTMReal(nn.Module, GaussianReparam):
    """Real-data encoder (model.py:180-242): LSTM over cat(x, a_in, t/max(mask)) with NO input masking, two-layer tanh
    heads; ``reverse`` flips the window first.  ``output_all`` returns the two heads at every step of the window,
    (T, B, output_dim) each, rows in processing order (after the flip when ``reverse``; as in the reference they are not
    flipped back) -- ``hode.lstm.lstm_sequence``; run_real.py passes False (the final step: ``hode.lstm.lstm_encode``)."""

    def __init__(self, input_dim, hidden_dim, output_dim, output_all=False, reverse=True, normalize=True, device=None):
        super().__init__()
        self.device = get_device() if device is None else device
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.normalize = normalize
        self.model_name = "LSTMReal"
        self.lstm = nn.LSTM(input_dim, hidden_dim).to(self.device)
        self.lin = nn.Sequential(nn.Linear(hidden_dim, hidden_dim + 1), nn.Tanh(), nn.Linear(hidden_dim + 1, output_dim), nn.Tanh()).to(self.device)
        self.log_var = nn.Sequential(nn.Linear(hidden_dim, hidden_dim + 1), nn.Tanh(), nn.Linear(hidden_dim + 1, output_dim), nn.Tanh()).to(self.device)
        self.reverse = reverse
        self.output_all = output_all

    def forward(self, x, a, m):
        if self.reverse:
            x, a, m = torch.flip(x, [0]), torch.flip(a, [0]), torch.flip(m, [0])
        T, B = m.shape[0], m.shape[1]
        tt = (torch.arange(T, device=x.device, dtype=x.dtype) / m.max()).view(T, 1, 1).expand(T, B, 1)
        x_in = torch.cat([x, a, tt], dim=-1)
        p = self.lstm
        if self.output_all:
            if x_in.is_cuda:
                from hode.lstm import lstm_sequence
                out = lstm_sequence(x_in, None, None, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, reverse=False)
            else:
                out = p(x_in)[0]
        elif x_in.is_cuda:
            from hode.lstm import lstm_encode
            out = lstm_encode(x_in, None, None, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, reverse=False)
        else:
            out = p(x_in)[1][0][0]
        if out.is_cuda:
            return _tall_mlp(self.lin, out), _tall_mlp(self.log_var, out)
        return self.lin(out), self.log_var(out)


class LSTMBaseline(nn.Module):
    """Sequence-to-sequence LSTM forecaster for the real-data set (model.py:322-380): an LSTM over cat(x, a) in forward time
    (the mask is not applied to the inputs, as in the reference), then Linear(H, H+1) / ELU / Linear(H+1, output_dim) on the
    hidden state of every step; ``loss`` is the masked one-step-ahead SSE.

    HIP tensors: ``hode.lstm.lstm_sequence`` (the window kernel with every step's h as output, the BPTT kernel with a
    cotangent per step) and ``_tall_mlp`` for the readout; a hidden size above 160 raises ``HodeConfigError``.  CPU tensors
    (host-logic tests): ``nn.LSTM``."""

    def __init__(self, input_dim, hidden_dim, output_dim, normalize=True, device=None):
        super().__init__()
        self.device = get_device() if device is None else device
        self.hidden_dim = hidden_dim
        self.normalize = normalize
        self.output_dim = output_dim
        self.model_name = "LSTMBaseline"
        # creation order lstm -> out fixes both the seeded init and the state_dict key order
        self.lstm = nn.LSTM(input_dim, hidden_dim).to(self.device)
        self.out = nn.Sequential(nn.Linear(self.hidden_dim, self.hidden_dim + 1, bias=True), nn.ELU(),
                                 nn.Linear(self.hidden_dim + 1, self.output_dim, bias=True)).to(self.device)

    def forward(self, x, a, mask):
        if x.dim() == 3 and x.shape[1] == 1:
            raise RuntimeError("LSTMBaseline: batch size 1 is not supported (the reference's x.squeeze() drops the batch axis)")
        p = self.lstm
        if x.is_cuda:
            from hode.lstm import lstm_sequence
            out = lstm_sequence(x, a, None, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, reverse=False)
            return _tall_mlp(self.out, out)
        out, _ = p(torch.cat([x, a], dim=-1))
        return self.out(out)

    def loss(self, data):
        x, a, mask, s = data["measurements"], data["actions"], data["masks"], data["statics"]
        a_in = torch.cat([a, s], dim=-1)
        x_hat = self.forward(x, a_in, mask)[:-1]
        # row t of x_hat predicts x[t + 1]; masked SSE per patient of the batch
        return torch.sum((x[1:] - x_hat) ** 2 * mask[1:]) / x.shape[1]

    def save(self, path, itr, best_loss):
        path = path + self.model_name
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"itr": itr, "state_dict": self.state_dict(), "best_loss": best_loss}, path)


class _RocheRealDoseGrad(torch.autograd.Function):
    """h = odeint(RocheODEReal, y0, t, method) on a fixed grid with a gradient for the dose table act (Ta, B) as well
    (``RocheODEReal.dose_grad``).  Forward: ``hode.real.real_solve`` under no_grad on detached inputs, so h is bit for bit what
    the plain call returns at every latent size.  Backward: ``hode.real_dose.real_dose_backward`` (libhode_real_dose.so).
    Gradients for y0, theta, wflat and act; none for t (its .grad stays None)."""

    @staticmethod
    def forward(ctx, y0, theta, wflat, t, act, hidden, method, perturb):
        from hode import real
        f32c = hode.solver._f32c
        thc, wc, tc, ac = f32c(theta), f32c(wflat), f32c(t), f32c(act)
        with torch.no_grad():  # detached inputs: the forward keeps nothing for a backward of its own
            h = real.real_solve(f32c(y0), thc, wc, tc, ac, hidden, method=method, perturb=perturb, library=None)
        ctx.save_for_backward(h, thc, wc, tc, ac)
        ctx.meta = (int(hidden), method, bool(perturb))
        return h

    @staticmethod
    def backward(ctx, grad_h):
        from hode import real_dose
        h, thc, wc, tc, ac = ctx.saved_tensors
        hidden, method, perturb = ctx.meta
        gy0, gth, gw, gact = real_dose.real_dose_backward(h, thc, wc, tc, ac, hode.solver._f32c(grad_h), hidden, method=method,
                                                          perturb=perturb)
        return gy0, gth, gw, None, gact, None, None, None


class _RocheRealPatientDopri5(torch.autograd.Function):
    """h = odeint(RocheODEReal, y0, t, method="dopri5", options={"step_t": t}) with per-patient step control: the two
    launches of ``hode.real_pp`` (libhode_real_pp.so).  Gradients for y0, theta and wflat; none for t and the dose table
    (their .grad stays None).  Every step size is a constant in the backward, dt_0 included."""

    @staticmethod
    def forward(ctx, y0, theta, wflat, t, act, hidden, rtol, atol, grad_enabled=True):
        from hode import real_pp
        f32c = hode.solver._f32c
        y0c, thc, wc, tc, ac = f32c(y0), f32c(theta), f32c(wflat), f32c(t), f32c(act)
        # `needs_input_grad` reflects requires_grad, not the grad mode, and inside forward() grad mode is always off: the
        # caller samples it before .apply().  Nothing to differentiate: no tape at all.
        no_tape = not (grad_enabled and any(ctx.needs_input_grad[:3]))
        h, ws, stats = real_pp.real_patient_dopri5_forward(y0c, thc, wc, tc, ac, hidden, rtol=rtol, atol=atol, no_tape=no_tape)
        ctx.save_for_backward(h, thc, wc, tc, ac, y0c, ws, stats["n_accepted"])
        ctx.meta = (int(hidden), float(rtol), float(atol), int(stats["max_steps"]))
        return h

    @staticmethod
    def backward(ctx, grad_h):
        from hode import real_pp
        h, thc, wc, tc, ac, y0c, ws, n_accepted = ctx.saved_tensors
        hidden, rtol, atol, steps = ctx.meta
        gy0, gth, gw = real_pp.real_patient_dopri5_backward(y0c, thc, wc, tc, ac, hidden, h, ws, n_accepted, steps,
                                                            hode.solver._f32c(grad_h), rtol=rtol, atol=atol)
        return gy0, gth, gw, None, None, None, None, None, None


class RocheODEReal(nn.Module):
    """Real-data hybrid rhs: two small MLPs for x1, x2, expert x3 / Dose2, GRU-ODE block on the rest (model.py:570-657).

    A reproduced quirk: the reference's ``dose_at_time`` sums over dims (0, 2) (model.py:653-657), so EVERY column of the
    action handed to ``set_action_static`` is added into the dose.  ``run_real_ensemble.py`` and ``run_real_residual.py``
    call the expert decoder with ``cat([a, s], -1)`` as its action: the published expert forecasts of the ensemble and
    residual rows had the static covariates added to the dose.  The decay is linear in the dose, so the kernels are handed
    the column sum; with one column (every other script) the call is what it always was."""

    def __init__(self, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, device=None, dtype=DTYPE):
        super().__init__()
        self.action_dim, self.latent_dim = int(action_dim), int(latent_dim)
        self.static_dim, self.hidden_dim = int(static_dim), int(hidden_dim)
        self.dosage = None
        self._times = None
        self.device = get_device() if device is None else device
        self.t_max, self.step_size = t_max, step_size
        h = self.hidden_dim
        self.dx1_net = nn.Sequential(nn.Linear(3, h), nn.Tanh(), nn.Linear(h, 1), nn.Tanh())
        self.dx2_net = nn.Sequential(nn.Linear(2, h), nn.Tanh(), nn.Linear(h, 1), nn.Tanh())
        self.expert_dim = 4
        self.expert_only = self.latent_dim == self.expert_dim
        if not self.expert_only:
            m = self.latent_dim - self.expert_dim
            self.lin_hh = nn.Linear(m, m, bias=False)
            self.lin_hz = nn.Linear(m, m, bias=False)
            self.lin_hr = nn.Linear(m, m, bias=False)
        self.k_immunity = nn.Parameter(torch.tensor(1, device=self.device, dtype=dtype))
        self.kel = nn.Parameter(torch.tensor(0.2, device=self.device, dtype=dtype))
        self.kel2 = nn.Parameter(torch.tensor(0.2, device=self.device, dtype=dtype))
        # fixed-grid methods only: True lets a gradient reach the treatment -- with an action that requires grad the solve's
        # backward fills the gradient of the dose table (hode.real_dose, libhode_real_dose.so)
        self.dose_grad = False
        # dopri5 only: "batch" has no kernel for this rhs (refused); "patient" gives every patient a controller of its own
        # and cuts the steps at the output times (hode.real_pp); options["step_control"] of hode.odeint overrides it for one call
        self.step_control = "batch"
        self.to(self.device)  # the reference leaves the sub-networks on the default device; everything lives on one here

    def set_action_static(self, action, static):
        self.dosage = action
        self._times = None

    @property
    def times(self):
        """1, 2, .., T along the time axis, shaped like the action (model.py:650-651).  Only the eager rhs (`forward`,
        `dose_at_time`) reads it -- the kernels index time themselves -- so it is formed on first use, not per step."""
        if self._times is None and self.dosage is not None:
            self._times = torch.cumsum(torch.ones_like(self.dosage), dim=0)
        return self._times

    @times.setter
    def times(self, value):
        self._times = value

    def dose_at_time(self, t):
        on = t >= self.times
        return torch.sum(self.dosage * torch.exp(self.kel * (self.times - t) * on) * on, dim=(0, 2))

    def forward(self, t, y):
        dose = self.dose_at_time(t)
        cols = [self.dx1_net(y[:, :3]), self.dx2_net(y[:, :2]), (y[:, 1] * self.k_immunity)[..., None],
                (self.kel * dose - self.kel2 * y[:, 3])[..., None]]
        if not self.expert_only:
            hv = y[..., 4:]
            r = torch.sigmoid(self.lin_hr(hv))
            z = torch.sigmoid(self.lin_hz(hv))
            u = torch.tanh(self.lin_hh(r * hv))
            cols.append((1 - z) * (u - hv))
        return torch.cat(cols, dim=-1)

    def flat_weights(self):
        ps = [self.dx1_net[0].weight, self.dx1_net[0].bias, self.dx1_net[2].weight, self.dx1_net[2].bias,
              self.dx2_net[0].weight, self.dx2_net[0].bias, self.dx2_net[2].weight, self.dx2_net[2].bias]
        if not self.expert_only:
            ps += [self.lin_hh.weight, self.lin_hz.weight, self.lin_hr.weight]
        return torch.cat([p.reshape(-1) for p in ps])

    def hode_solve(self, y0, t, rtol, atol, method, options):
        if self.dosage is None:
            raise RuntimeError("RocheODEReal: call set_action_static(a, s) before integrating")
        if _step_control(self, options) == "patient":
            if method == "dopri5":
                return self._solve_patient_dopri5(y0, t, rtol, atol, options)
            _refuse_patient_step_control(self, {"step_control": "patient"})
        from hode import real
        if method == "dopri5":
            # DecoderReal hands dopri5 a `step_t` grid (model.py:826: steps are cut at the hourly dose switches); that
            # option's semantics are not restated by the oracle.  real.sh:15 uses midpoint.
            raise hode.HodeConfigError("hode: RocheODEReal is built for the fixed-grid methods (euler, midpoint, rk4); "
                                 "dopri5 with options['step_t'] is not supported")
        from hode import substep
        step_size = options.pop("step_size", None)
        if step_size is not None and t.numel() > 1:
            # torchdiffeq builds its own grid t0 + k*step_size; when that IS the output grid (run_real.py's default,
            # ode_step_div = 1) nothing has to be interpolated
            # (a host read-back: cached per grid tensor, the decoder hands over the same `t` at every call)
            cache = getattr(self, "_uniform_grid_cache", None)
            if cache is None or cache[0] is not t or cache[1] != (t._version, float(step_size)):
                cache = (t, (t._version, float(step_size)), bool(torch.allclose(t[1:] - t[:-1], torch.full_like(t[1:], float(step_size)))))
                self._uniform_grid_cache = cache
            if cache[2]:
                step_size = None
        options.pop("step_t", None)  # ignored by fixed-grid solvers (torchdiffeq only warns)
        theta = torch.stack([self.k_immunity, self.kel, self.kel2])
        wflat, perturb = self.flat_weights(), bool(options.pop("perturb", False))
        # more than one action column: the reference's sum over dims (0, 2) adds them all into the dose (see the class docstring)
        dose = self.dosage[..., 0] if self.dosage.shape[-1] == 1 else self.dosage.sum(-1)
        if self.dose_grad and dose.requires_grad and torch.is_grad_enabled():
            from hode import real_dose
            real_dose.check_domain(self.latent_dim, self.hidden_dim)  # names the sizes held and libhode_real_dose.so; nothing is loaded or launched before
            # the column sum above stays a torch op: every column of the action receives the same gradient
            return substep.solve_with_step_size(
                lambda grid: _RocheRealDoseGrad.apply(y0, theta, wflat, grid, dose, self.hidden_dim, method, perturb),
                t, step_size)
        # which library serves this latent size (libhode.so at 4 and 20, libhode_real_dims.so at 5 .. 19) is real_solve's choice
        return substep.solve_with_step_size(
            lambda grid: real.real_solve(y0, theta, wflat, grid, dose, self.hidden_dim, method=method, perturb=perturb, library=None),
            t, step_size)

    def _solve_patient_dopri5(self, y0, t, rtol, atol, options):
        """dopri5 with per-patient step control and the steps cut at the output times (``hode.real_pp``): what
        ``options["step_t"] = t`` means for a batch of one.  ``step_size`` and ``perturb`` are ignored, as torchdiffeq ignores
        them for dopri5.  Every refusal comes before a library is loaded."""
        from hode import real_pp
        real_pp.check_domain(self.latent_dim, self.hidden_dim)
        step_t = options.pop("step_t", None)
        if step_t is not None and step_t is not t:
            step_t = torch.as_tensor(step_t)
            if step_t.shape != t.shape or not bool(torch.equal(step_t.to(t.device, t.dtype), t)):
                raise hode.HodeConfigError("hode: RocheODEReal with step_control='patient' cuts the steps at the output times; "
                                           "options['step_t'] must be the output grid t itself (or absent)")
        options.pop("step_size", None)
        options.pop("perturb", None)
        dose = self.dosage[..., 0] if self.dosage.shape[-1] == 1 else self.dosage.sum(-1)
        grad_enabled = torch.is_grad_enabled()
        if self.dose_grad and dose.requires_grad and grad_enabled:
            raise hode.HodeConfigError("hode: RocheODEReal.dose_grad serves the fixed-grid methods euler / midpoint / rk4; "
                                       "method='dopri5' (step_control='patient') has no dose-table gradient -- detach the "
                                       "action or switch dose_grad off")
        hode.solver._require_gpu(y0, t, dose, self.kel)
        theta = torch.stack([self.k_immunity, self.kel, self.kel2])
        return _RocheRealPatientDopri5.apply(y0, theta, self.flat_weights(), t, dose.detach(), self.hidden_dim, float(rtol),
                                             float(atol), grad_enabled)

    def hode_solve_steps(self, init, t, method, options):
        """One-step-ahead solve (reference DecoderReal.forward with a 3-D ``init``): interval i of ``t`` integrated on its
        own from ``init[i]``; h (len(t), B, D) with the zero row first (``hode.real_step.real_step_solve``)."""
        if self.dosage is None:
            raise RuntimeError("RocheODEReal: call set_action_static(a, s) before integrating")
        from hode import real_step
        if method == "dopri5":
            raise hode.HodeConfigError("hode: RocheODEReal is built for the fixed-grid methods (euler, midpoint, rk4); "
                                       "dopri5 with options['step_t'] is not supported")
        options = dict(options)
        theta = torch.stack([self.k_immunity, self.kel, self.kel2])
        dose = self.dosage[..., 0] if self.dosage.shape[-1] == 1 else self.dosage.sum(-1)
        if self.dose_grad and dose.requires_grad and torch.is_grad_enabled():
            raise hode.HodeConfigError("hode: RocheODEReal.dose_grad serves the chained solve (a 2-D init); the one-step-ahead "
                                       "solve (a 3-D init) has no dose-table gradient -- detach the action or switch dose_grad off")
        return real_step.real_step_solve(init, theta, self.flat_weights(), t, dose, self.hidden_dim, method=method,
                                         perturb=bool(options.pop("perturb", False)), step_size=options.pop("step_size", None))


class _NeuralODERealBase(nn.Module):
    """Shared body of the neural ODE baselines of the real-data experiment (reference model.py:660-769): an MLP on
    [y, dose(t)] with dose(t) = cumsum(action, 0)[int(t)] (zeros once int(t) >= Ta).  ``forward`` is the reference's eager
    rhs; ``hode_solve`` integrates on the gfx950 kernels (``hode.neural_real``), which run on a HIP device only."""

    kind = None

    def __init__(self, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, out_dim, device=None, dtype=DTYPE):
        super().__init__()
        self.action_dim, self.latent_dim = int(action_dim), int(latent_dim)
        self.static_dim, self.hidden_dim = int(static_dim), int(hidden_dim)
        self.device = get_device() if device is None else device
        self.t_max, self.step_size = t_max, step_size
        self.ml_net = nn.Sequential(nn.Linear(self.latent_dim + self.action_dim, self.hidden_dim), nn.Tanh(),
                                    nn.Linear(self.hidden_dim, out_dim), nn.Tanh()).to(self.device)
        self.action = None
        self.static = None
        self._rows = None

    def set_action_static(self, action, static):
        self.action = action
        self.static = static[0, :, :] if static is not None and static.dim() == 3 else static  # stored, unused

    def dose_at_time(self, t):
        t_int = int(t)
        if t_int >= self.action.shape[0]:
            return torch.zeros_like(self.action[0, :, :])
        return torch.cumsum(self.action, dim=0)[t_int, :, :]

    def _table_index(self, grid, method, perturb, device):
        """Flat dose-table rows of every (interval, stage) of the solve over ``grid``: one host read-back per grid tensor
        (cached on its identity and version, like DecoderRealBenchmark's step tables), so a training step has no sync."""
        from hode import neural_real
        Ta = int(self.action.shape[0])
        key = (grid, grid._version, method, bool(perturb), Ta, device)
        if self._rows is None or self._rows[0] is not grid or self._rows[1:6] != key[1:]:
            rows = neural_real.stage_rows(grid, method, perturb, Ta)
            self._rows = key + (neural_real.table_index(rows, Ta).reshape(-1).to(device),)
        return self._rows[6]

    def hode_solve(self, y0, t, rtol, atol, method, options):
        from hode import neural_real, substep
        _refuse_patient_step_control(self, options)
        neural_real.check_config(self.kind, self.latent_dim, self.hidden_dim, self.action_dim, method)
        if self.action is None:
            raise RuntimeError("%s: call set_action_static(a, s) before integrating" % type(self).__name__)
        step_size = options.pop("step_size", None)
        if step_size is not None and t.numel() > 1:
            # the solver grid t0 + k*step_size IS the output grid at run_real.py's default (ode_step_div = 1): nothing to
            # interpolate (the check is a host read-back, cached per grid tensor as in RocheODEReal)
            cache = getattr(self, "_uniform_grid_cache", None)
            if cache is None or cache[0] is not t or cache[1] != (t._version, float(step_size)):
                cache = (t, (t._version, float(step_size)), bool(torch.allclose(t[1:] - t[:-1], torch.full_like(t[1:], float(step_size)))))
                self._uniform_grid_cache = cache
            if cache[2]:
                step_size = None
        options.pop("step_t", None)  # ignored by fixed-grid solvers (torchdiffeq only warns)
        perturb = bool(options.pop("perturb", False))
        l0, l2 = self.ml_net[0], self.ml_net[2]

        def solve_on(grid):
            index = self._table_index(grid, method, perturb, y0.device)
            return neural_real.neural_real_solve(self.kind, y0, l0.weight, l0.bias, l2.weight, l2.bias, grid, self.action,
                                                 index, method)

        return substep.solve_with_step_size(solve_on, t, step_size)


class NeuralODEReal(_NeuralODERealBase):
    """``neural`` baseline (reference model.py:710-769): dy/dt = ml_net([y, dose(t)]), ml_net = Linear(D+1, H), Tanh,
    Linear(H, D), Tanh."""

    kind = "neural"

    def __init__(self, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, device=None, dtype=DTYPE):
        super().__init__(latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, int(latent_dim), device, dtype)

    def forward(self, t, y):
        dose = self.dose_at_time(t)
        return self.ml_net(torch.cat([y, dose], dim=-1))


class NeuralODEReal2nd(_NeuralODERealBase):
    """``2nd`` baseline (reference model.py:660-707): dy/dt = [ml_net([y, dose(t)]), y[:, :D//2]], ml_net = Linear(D+1, H),
    Tanh, Linear(H, D//2), Tanh.  Odd D cannot be integrated (the derivative has D - 1 columns); ``hode_solve`` refuses it."""

    kind = "2nd"

    def __init__(self, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, device=None, dtype=DTYPE):
        super().__init__(latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, int(latent_dim) // 2, device, dtype)

    def forward(self, t, y):
        dose = self.dose_at_time(t)
        return torch.cat([self.ml_net(torch.cat([y, dose], dim=-1)), y[..., : (self.latent_dim // 2)]], dim=-1)


class _TallLinear(torch.autograd.Function):
    """``x @ W.T + b`` for x with ~1e6 rows and ~20 columns.  Same numbers as ``nn.Linear``; the backward forms the bias
    gradient as a (1 x rows) GEMM -- torch's column sum over such a shape takes 2 ms at 0.8 M x 21 (config 5), two orders
    of magnitude off the HBM rate."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.addmm(bias, x, weight.t())

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        return g @ weight, _rows_tn(g, x), _rows_sum(g)


_ONES = {}


def _ones(*shape, like):
    """Constant all-ones GEMM operand, kept per (shape, device, dtype): a fill kernel per use is 5 us of launch latency."""
    key = (shape, like.device, like.dtype)
    if key not in _ONES:
        _ONES[key] = torch.ones(shape, device=like.device, dtype=like.dtype)
    return _ONES[key]


def _row_slices(t):
    rows = t.shape[0]
    if t.is_cuda:
        for cand in range(64, 1, -1):
            if rows % cand == 0 and rows // cand >= 128:
                return cand
    return 1


def _rows_sum(g):
    """Column sums of a (rows x n) matrix as GEMMs with a ones vector, over row slices like `_rows_tn`."""
    rows, P = g.shape[0], _row_slices(g)
    if P == 1:
        return (_ones(1, rows, like=g) @ g).reshape(-1)
    part = torch.bmm(_ones(P, 1, rows // P, like=g), g.reshape(P, rows // P, -1))
    return (_ones(1, P, like=g) @ part.view(P, -1)).reshape(-1)


def _rows_tn(g, x):
    """``g.T @ x`` for (rows x n), (rows x k) with rows in the thousands and n, k in the tens: the result is a handful of
    tiles, so the library runs the whole contraction on as many workgroups (57 us for 45 x 44 over 8 192 rows, config 5's
    encoder heads).  The rows are cut into P slices, one batched product forms P partial results on P times as many
    workgroups and a (1 x P) product folds them."""
    rows, P = g.shape[0], _row_slices(g)
    if P == 1:
        return g.t() @ x
    part = torch.bmm(g.reshape(P, rows // P, -1).transpose(1, 2), x.reshape(P, rows // P, -1))   # reshape: x may be a strided view
    return (_ones(1, P, like=g) @ part.view(P, -1)).view(part.shape[1], part.shape[2])


def _tall_mlp(seq, x):
    """Apply an ``nn.Sequential`` of Linear / activation layers to (..., k) rows with ``_TallLinear`` for the Linear ones."""
    shape = x.shape[:-1]
    y = x.reshape(-1, x.shape[-1])
    for layer in seq:
        y = _TallLinear.apply(y, layer.weight, layer.bias) if isinstance(layer, nn.Linear) else layer(y)
    return y.reshape(*shape, y.shape[-1])


class DecoderReal(nn.Module):
    """z0 -> h over t = t0-1 .. t_max-1 -> MLP readout, first output row dropped (model.py:772-862).  ``ode_type``
    "neural" / "2nd" build the neural ODE baselines (``NeuralODEReal`` / ``NeuralODEReal2nd``), which run on the GPU
    kernels only: constructing them on a non-HIP device raises ``HodeConfigError``; anything else is the hybrid rhs.

    A 3-D ``init`` (>= t_max - 1, B, D) is the reference's one-step-ahead mode (model.py:838-861; the hybrid rhs only):
    interval i = t[i] -> t[i + 1], i < t_max - 1, is integrated on its own from ``init[i]``; ``h`` is the end states behind a
    zero row, (t_max, B, D), and row 0 of ``x_hat`` is zero.  With ``hode.odeint`` all intervals run in one kernel launch
    per direction (``hode.real_step``); with any other ``_odeint`` they are the reference's loop of solver calls."""

    def __init__(self, obs_dim, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, t0=0, method="dopri5",
                 ode_step_size=None, ode_type="neural", device=None, dtype=DTYPE):
        super().__init__()
        self.time_dim = int(t_max / step_size)
        self.obs_dim, self.latent_dim, self.action_dim = obs_dim, latent_dim, action_dim
        self.t_max, self.t0 = t_max, t0
        self.static_dim, self.hidden_dim = int(static_dim), int(hidden_dim)
        self.model_name = "DecoderReal_" + ode_type
        self.device = get_device() if device is None else device
        self.output_function = nn.Sequential(nn.Linear(latent_dim, latent_dim + 1, bias=True), nn.ELU(),
                                             nn.Linear(latent_dim + 1, obs_dim, bias=True)).to(self.device)
        if ode_type in ("neural", "2nd"):
            from hode import neural_real
            neural_real.check_config(ode_type, latent_dim, hidden_dim, action_dim)
            if torch.device(self.device).type != "cuda":
                raise hode.HodeConfigError("DecoderReal(ode_type=%r): the NeuralODEReal baselines run on the GPU kernels only "
                                           "(device %s)" % (ode_type, self.device))
            cls = NeuralODEReal if ode_type == "neural" else NeuralODEReal2nd
            self.ode = cls(latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, self.device)
        else:
            self.ode = RocheODEReal(latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, self.device)
        self.t = torch.arange(t0 - 1, t_max, step_size, device=self.device, dtype=dtype)
        self.options = {"step_t": self.t, "step_size": ode_step_size, "perturb": True}
        self.rtol, self.atol = 1e-7, 1e-8
        self.method = method
        self.step_size = ode_step_size
        self._odeint = hode.odeint

    def forward(self, init, a, s):
        self.ode.set_action_static(a, s)
        h = self.latent(init, a, s)
        if h.is_cuda and h.shape[0] * h.shape[1] >= 65536:
            x_hat = _tall_mlp(self.output_function, h)[1:]
        else:
            x_hat = self.output_function(h)[1:]
        if init.dim() != 2:  # the reference's `x_hat[0] = 0.0`, without a write into a view autograd needs
            x_hat = torch.cat([torch.zeros_like(x_hat[:1]), x_hat[1:]], dim=0)
        return x_hat, h

    def latent(self, init, a, s):
        """Latent trajectory h (T - t0 + 1, B, D) only (row 0 = the state at t0 - 1, which the readout drops); for a 3-D
        ``init`` the one-step-ahead states (t_max, B, D) behind their zero row."""
        self.ode.set_action_static(a, s)
        if init.dim() != 2:
            return self._latent_steps(init)
        return self._odeint(self.ode, init, self.t, method=self.method, options=dict(self.options), rtol=self.rtol, atol=self.atol)

    def _latent_steps(self, init):
        if not isinstance(self.ode, RocheODEReal):
            raise hode.HodeConfigError("DecoderReal(%s): per-step initial states (3-D init) are served by the hybrid decoder "
                                       "(ode_type='hybrid') only" % self.model_name)
        n = int(self.t_max) - 1
        if self.t.numel() < self.t_max:
            raise hode.HodeConfigError("DecoderReal: per-step initial states (3-D init) need a grid of at least t_max = %d points, this "
                                       "decoder's has %d (t0 = %s): the reference hands the solver fewer than two time points for "
                                       "the last intervals there, and nothing defines the result" % (self.t_max, self.t.numel(), self.t0))
        if init.dim() != 3 or init.shape[0] < n:
            raise hode.HodeConfigError("DecoderReal: per-step initial states are (>= t_max - 1 = %d, B, D), one row per interval; "
                                       "got %s" % (n, tuple(init.shape)))
        if self._odeint is hode.odeint:
            cache = getattr(self, "_step_grid", None)   # the same grid tensor at every call: its table is cached on identity
            if cache is None or cache[0] is not self.t or cache[1] != self.t._version:
                cache = (self.t, self.t._version, self.t[: n + 1])
                self._step_grid = cache
            return self.ode.hode_solve_steps(init, cache[2], self.method, self.options)
        ends = [self._odeint(self.ode, init[i], self.t[i:i + 2], method=self.method, options=dict(self.options), rtol=self.rtol,
                             atol=self.atol)[-1] for i in range(n)]
        return torch.stack([torch.zeros_like(ends[0])] + ends, dim=0)

    def fused_likelihood_ok(self, x):
        from hode import readout
        return (x.is_cuda and self._odeint is hode.odeint
                and readout.mlp_supported(self.latent_dim, self.output_function[0].out_features, self.obs_dim))

    def masked_sse(self, h, x, mask, time_weight=None):
        """sum((x - output_function(h[1:]))^2 * mask * time_weight) / B in one fused pass over the rows (x_hat never hits
        HBM; the two Linear layers, the ELU, the loss and all their gradients are one kernel)."""
        from hode import readout
        l0, l2 = self.output_function[0], self.output_function[2]
        return readout.masked_sse_readout_mlp(h, x, mask, l0.weight, l0.bias, l2.weight, l2.bias, time_weight, skip_rows=1)


class GRUODECell(nn.Module):
    """GRU-ODE cell of the ``gruode`` baseline (reference model.py:865-886).  ``forward(a, h_all)`` is the eager arithmetic:
    with x = [h_all[0], a], z = sigmoid(lin_hz x) and n = tanh(lin_hn(z * x)) it returns (1 - z[..., :D]) * (n - h_all[0])
    together with the state it was handed, (h_all[0], 0).  ``DecoderRealBenchmark`` runs the same cell in one kernel."""

    def __init__(self, hidden_size, bias=True):
        super().__init__()
        self.hidden_size = hidden_size
        self.lin_hz = nn.Linear(hidden_size + 2, hidden_size + 2, bias=False)
        self.lin_hn = nn.Linear(hidden_size + 2, hidden_size, bias=False)

    def forward(self, a, h_all):
        state = h_all[0]
        x = torch.cat([state, a], dim=-1)
        z = torch.sigmoid(self.lin_hz(x))
        n = torch.tanh(self.lin_hn(z * x))
        return (1 - z[:, :, : self.hidden_size]) * (n - state), (state, 0)


class DecoderRealBenchmark(nn.Module):
    """Recurrent baselines of the real-data experiment (reference model.py:889-966): z0 -> h over t = t0 .. t_max - 1 ->
    MLP readout; unlike ``DecoderReal`` no output row is dropped.

    ``tlstm``: nn.LSTM(2 action_dim, D) stepped over the grid with h0 = c0 = init, input [a[t], t / t_max].
    ``gruode``: the reference hands ``GRUODECell`` the pair (hidden, c) and takes back (out, (hidden, c)); the cell returns
    the state it was given, so the hidden state stays ``init`` at every step and h[k] is the cell's output for
    x_k = [init, a[t_k], t_k / t_max].  That is what the published numbers ran; it is reproduced, not fixed.

    Both run as one gfx950 kernel per direction (``hode.seqdec``); CPU tensors raise ``HodeConfigError``.  ``method``,
    ``ode_step_size`` and ``hidden_dim`` are stored and unused, as in the reference.  The cell is moved to ``device`` with
    the rest of the module (the reference leaves it on the default device)."""

    def __init__(self, obs_dim, latent_dim, action_dim, static_dim, hidden_dim, t_max, step_size, t0=0, method="dopri5",
                 ode_step_size=None, ode_type="tlstm", device=None, dtype=DTYPE):
        super().__init__()
        self.time_dim = int(t_max / step_size)
        self.obs_dim, self.latent_dim, self.action_dim = obs_dim, latent_dim, action_dim
        self.t_max, self.t0, self.step_size = t_max, t0, step_size
        self.static_dim, self.hidden_dim = int(static_dim), int(hidden_dim)
        self.model_name = "DecoderReal_" + ode_type
        self.device = get_device() if device is None else device
        # readout first, then the cell: the reference's parameter creation order (seeded-init parity)
        self.output_function = nn.Sequential(nn.Linear(latent_dim, latent_dim + 1, bias=True), nn.ELU(),
                                             nn.Linear(latent_dim + 1, obs_dim, bias=True)).to(self.device)
        self.ode_type = ode_type
        if ode_type == "tlstm":
            self.rnn = nn.LSTM(action_dim * 2, latent_dim).to(self.device)
        elif ode_type == "gruode":
            self.rnn = GRUODECell(latent_dim).to(self.device)
        else:
            raise hode.HodeConfigError("DecoderRealBenchmark(ode_type=%r): the baselines are 'tlstm' and 'gruode'" % (ode_type,))
        self.t = torch.arange(t0, t_max, step_size, device=self.device, dtype=dtype)
        self.method = method
        self.step_size = ode_step_size
        self._tables = None

    def _step_tables(self, device):
        """Action row and time feature of every step, built once per grid tensor and device (one host read-back)."""
        key = (self.t, self.t._version, self.t_max, device)
        if self._tables is None or self._tables[0] is not key[0] or self._tables[1:4] != key[1:]:
            from hode import seqdec
            self._tables = key + seqdec.step_tables(self.t, self.t_max, device)
        return self._tables[4:]

    def latent(self, init, a, s):
        """Decoder outputs h (len(t), B, D) before the readout."""
        from hode import seqdec
        from hode.solver import _require_gpu
        _require_gpu(init, a)
        if init.dim() != 2:
            raise hode.HodeConfigError("DecoderRealBenchmark: per-step initial states (3-D init) are outside the accelerated path; "
                                       "DecoderReal(ode_type='hybrid') serves them")
        idx, tau, max_row = self._step_tables(init.device)
        if self.ode_type == "tlstm":
            r = self.rnn
            return seqdec.tlstm(init, a, idx, tau, max_row, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)
        return seqdec.gruode(init, a, idx, tau, max_row, self.rnn.lin_hz.weight, self.rnn.lin_hn.weight)

    def forward(self, init, a, s):
        h = self.latent(init, a, s)
        if h.shape[0] * h.shape[1] >= 65536:
            return _tall_mlp(self.output_function, h), h
        return self.output_function(h), h

    def fused_likelihood_ok(self, x):
        from hode import readout
        return x.is_cuda and readout.mlp_supported(self.latent_dim, self.output_function[0].out_features, self.obs_dim)

    def masked_sse(self, h, x, mask, time_weight=None):
        """sum((x - output_function(h))^2 * mask * time_weight) / B in one fused pass over the rows (every row of h)."""
        from hode import readout
        if h.shape[0] != x.shape[0] or h.shape[1] != x.shape[1]:
            raise hode.HodeConfigError("DecoderRealBenchmark.masked_sse: h has %d x %d rows, x %d x %d" % (h.shape[0], h.shape[1],
                                                                                                        x.shape[0], x.shape[1]))
        l0, l2 = self.output_function[0], self.output_function[2]
        return readout.masked_sse_readout_mlp(h, x, mask, l0.weight, l0.bias, l2.weight, l2.bias, time_weight, skip_rows=0)


class VariationalInference:
    """Negative ELBO: masked SSE likelihood + KL (analytic vs N(0,1), or Monte-Carlo vs a given prior) (model.py:1124-1214)."""

    epsilon = torch.finfo(DTYPE).eps

    def __init__(self, encoder, decoder, elbo=True, prior_log_pdf=None, mc_size=100):
        self.encoder, self.decoder = encoder, decoder
        self.prior_log_pdf = prior_log_pdf
        self.mc_size = mc_size
        self.elbo = elbo
        self.fuse_likelihood = True  # fused readout + masked-SSE kernel when the decoder supports the shape
        self.fuse_mc_kl = True       # fused Monte-Carlo KL kernel for the Exponential prior
        self.model_name = "VI_{}_{}.pkl".format(encoder.model_name, decoder.model_name)

    def save(self, path, itr, best_loss):
        path = path + self.model_name
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"itr": itr, "encoder_state_dict": self.encoder.state_dict(),
                    "decoder_state_dict": self.decoder.state_dict(), "best_loss": best_loss}, path)

    def parameters(self):
        return list(self.encoder.parameters()) + list(self.decoder.parameters())

    def loss(self, data):
        x, a, mask = data["measurements"], data["actions"], data["masks"]
        self.x, self.a, self.mask = x, a, mask
        mu, log_var = self.encoder(x, a, mask)
        self.mu, self.log_var = mu, log_var
        z = self.encoder.reparameterize(mu, log_var) if self.elbo else mu
        self.z = z
        fused = getattr(self.decoder, "fused_likelihood_ok", None)
        if self.fuse_likelihood and fused is not None and fused(x):
            # readout + masked SSE (+ gradients) in one HBM pass; x_hat is produced only if somebody reads vi.x_hat
            h_hat = self.decoder.latent(z, a)
            self.h_hat, self._x_hat = h_hat, None
            lik = self.decoder.masked_sse(h_hat, x, mask)
        else:
            x_hat, h_hat = self.decoder(z, a)
            self._x_hat, self.h_hat = x_hat, h_hat
            lik = torch.sum((x - x_hat) ** 2 * mask) / x.shape[1]
        if not self.elbo:
            return lik
        if self.prior_log_pdf is None:
            kld = analytic_kl(mu, log_var)
        else:
            kld = torch.mean(self.mc_kl(mu, log_var, self.mc_size), dim=0)
        return lik + kld

    @property
    def x_hat(self):
        if getattr(self, "_x_hat", None) is None and getattr(self, "h_hat", None) is not None:
            with torch.no_grad():
                self._x_hat = self.decoder.output_function(self.h_hat)
                if isinstance(self.decoder, DecoderReal):
                    self._x_hat = self._x_hat[1:]  # output_function(h)[1:], model.py:859
        return self._x_hat

    @x_hat.setter
    def x_hat(self, value):
        self._x_hat = value

    def mc_kl(self, mu, log_var, sample_size):
        """E_q[log q - log p] from `sample_size` draws, non-positive draws clamped to eps.  All draws in one batched
        tensor (sample axis first) instead of the reference's Python loop; same RNG stream order."""
        sigma = torch.exp(0.5 * log_var)
        eps = torch.randn((sample_size,) + tuple(sigma.shape), device=sigma.device, dtype=sigma.dtype)
        if (mu.is_cuda and self.prior_log_pdf is ExponentialPrior.log_density
                and type(self.encoder).log_density is GaussianReparam.log_density and self.fuse_mc_kl):
            from hode import mckl  # one kernel, analytic gradients (hode_mc_kl_exponential)
            return mckl.mc_kl_exponential(mu, log_var, eps, ExponentialPrior.rate, self.epsilon).sum(dim=-1)
        z = eps * sigma + mu
        z = torch.where(z <= 0.0, torch.full_like(z, self.epsilon), z)
        log_q = self.encoder.log_density(mu, log_var, z)
        return torch.mean(log_q - self.prior_log_pdf(z), dim=0)


class VariationalInferenceReal(VariationalInference):
    """Real-data objective (model.py:1217-1261): encode the first t0 steps, decode the rest, masked SSE on x[t0:]."""

    def __init__(self, encoder, decoder, elbo=True, prior_log_pdf=None, mc_size=100, t0=24, weight=False):
        super().__init__(encoder, decoder, elbo, prior_log_pdf, mc_size)
        self.t0 = t0
        self.weight = weight

    def loss(self, data):
        x, a, mask, s = data["measurements"], data["actions"], data["masks"], data["statics"]
        t0 = self.t0
        mu, log_var = self.encoder(x[:t0], torch.cat([a[:t0], s[:t0]], dim=-1), mask[:t0])   # only the window is assembled
        z = self.encoder.reparameterize(mu, log_var) if self.elbo else mu
        self.z = z
        fused = getattr(self.decoder, "fused_likelihood_ok", None)
        if self.fuse_likelihood and fused is not None and fused(x):
            # readout MLP + masked, time-weighted SSE (+ every gradient) in one pass; x_hat only if somebody reads vi.x_hat
            h_hat = self.decoder.latent(z, a, s)
            self.h_hat, self._x_hat = h_hat, None
            tw = 1 / torch.arange(1, self.decoder.t_max - t0 + 1, device=x.device, dtype=torch.float32) if self.weight else None
            lik = self.decoder.masked_sse(h_hat, x[t0:], mask[t0:], tw)
        else:
            x_hat, h_hat = self.decoder(z, a, s)
            self.x_hat, self.h_hat = x_hat, h_hat
            if self.weight:
                weight = 1 / torch.arange(1, self.decoder.t_max - t0 + 1, device=x.device)[:, None, None]
            else:
                weight = 1.0
            lik = torch.sum((x[t0:] - x_hat) ** 2 * mask[t0:] * weight) / x[t0:].shape[1]
        if not self.elbo:
            return lik
        if self.prior_log_pdf is None:
            kld = analytic_kl(mu, log_var)
        else:
            kld = torch.mean(self.mc_kl(mu, log_var, self.mc_size), dim=0)
        return lik + kld


class VariationalInferenceFlow:
    """Negative ELBO with a flow posterior (reference model.py:1299-1380): masked SSE of one flow draw's
    decode + Monte-Carlo KL of ``mc_size`` further draws against the prior.  With ``mc_size == 1`` the decoder's draw
    is reused and the KL term is ``mean(log_p - log_q)`` -- the reference's sign, kept as is.  The encoder is an
    ``EncoderPlanarLSTM`` (LHM-NF) or an ``EncoderSylvesterLSTM`` (LHM-SNF); it supplies the draws.

    HIP tensors: all 1 + mc_size draws come from one (S, B, D) ``randn`` block and go through one fused forward and one
    fused backward launch (the encoder's ``posterior_sample``: ``hode.flow.planar_flow_sample`` or
    ``flow.sylvester_posterior_sample``); the likelihood takes the fused readout + masked-SSE path.
    RNG stream: the reference draws (B, D) per ``reparameterize`` call (decoder draw first, then the KL draws); here the
    same draws come from one (1 + mc_size, B, D) tensor in the same order, so the numbers differ from a seeded reference
    run although the distribution is the same.  The prior must be ``ExponentialPrior.log_density`` on the device (the
    kernel's prior); ``prior_log_pdf=None`` fails as in the reference (TypeError)."""

    def __init__(self, encoder, decoder, elbo=True, prior_log_pdf=None, mc_size=100):
        self.encoder = encoder
        self.decoder = decoder
        self.prior_log_pdf = prior_log_pdf
        self.mc_size = mc_size
        self.elbo = elbo
        self.fuse_likelihood = True
        self.model_name = "VI_FLOW_{}_{}.pkl".format(encoder.model_name, decoder.model_name)

    def save(self, path, itr, best_loss):
        path = path + self.model_name
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"itr": itr, "encoder_state_dict": self.encoder.state_dict(),
                    "decoder_state_dict": self.decoder.state_dict(), "best_loss": best_loss}, path)

    def parameters(self):
        return list(self.encoder.parameters()) + list(self.decoder.parameters())

    def noise(self, n_samples, like):
        """The standard-normal draws of one loss call: (n_samples, B, D), sample axis first."""
        return torch.randn((n_samples,) + tuple(like.shape), device=like.device, dtype=like.dtype)

    def flow_kl(self, encoder_out, eps, s_kl):
        """(z_out (S, B, D), kl (B,)): the flow draws of eps and the mean over draws s_kl.. of log q - log p."""
        mu, log_var = encoder_out[0], encoder_out[1]
        if self.prior_log_pdf is None:
            raise TypeError("'NoneType' object is not callable")  # the reference calls prior_log_pdf(z)
        if mu.is_cuda:
            if self.prior_log_pdf is not ExponentialPrior.log_density:
                raise hode.HodeConfigError("VariationalInferenceFlow: the device path implements the Exponential(100) "
                                           "prior only (ExponentialPrior.log_density)")
            return self.encoder.posterior_sample(encoder_out, eps, s_kl)  # the encoder's fused kernel pair
        z_out, log_det_j, z0 = self.encoder.flow_draws(*encoder_out, eps)
        log_q = self.encoder.log_density(mu, log_var, z_out, log_det_j, z0)
        return z_out, torch.mean((log_q - self.prior_log_pdf(z_out))[s_kl:], dim=0)

    def loss(self, data):
        x, a, mask = data["measurements"], data["actions"], data["masks"]
        self.x, self.a, self.mask = x, a, mask
        encoder_out = self.encoder(x, a, mask)
        mu = encoder_out[0]
        single = self.mc_size == 1
        eps = self.noise(1 if single else 1 + self.mc_size, mu)
        z_all, kl = self.flow_kl(encoder_out, eps, 0 if single else 1)
        z = z_all[0]
        self.z = z
        fused = getattr(self.decoder, "fused_likelihood_ok", None)
        if self.fuse_likelihood and fused is not None and fused(x):
            h_hat = self.decoder.latent(z, a)
            self.h_hat, self._x_hat = h_hat, None
            lik = self.decoder.masked_sse(h_hat, x, mask)
        else:
            x_hat, h_hat = self.decoder(z, a)
            self._x_hat, self.h_hat = x_hat, h_hat
            lik = torch.sum((x - x_hat) ** 2 * mask) / x.shape[1]
        kld = torch.mean(-kl if single else kl, dim=0)
        return lik + kld if self.elbo else lik

    x_hat = VariationalInference.x_hat
