"""The synthetic data generator on the GPU (libhode_datagen.so): what the reference's ``DataGeneratorRoche.solve`` does
with one ``scipy.integrate.ode("lsoda")`` loop per patient (``dataloader.py:96-198``) and ``generate_data`` does with the
stacked results (``:255-266``), as one call: a per-patient adaptive float64 Dormand-Prince solve of the TRUE hybrid ODE, the
noisy linear readout, the z-score over all patients and times, and the observation masks.  Evaluation-side code: no
autograd."""

from __future__ import annotations

import torch

from . import _datagen_lib as GL
from .solver import _f32c, _require_gpu, _stream

DEFAULT_MAX_STEPS = 10000


def _refuse(msg):
    raise GL.HodeConfigError("hode.datagen: " + msg)


def _tensor(x, like=None):
    """Tensors stay where they are; anything else (numpy arrays, lists) becomes a tensor next to `like`."""
    if torch.is_tensor(x):
        return x.detach()
    return torch.as_tensor(x, device=None if like is None else like.device)


def n_times(t_max, step_size):
    """The reference's ``time_dim`` (dataloader.py:45)."""
    return int(t_max / step_size + 1)


def simulate(init, dose_time, dose_amount, roche_config, ml_coef, output_coef, output_sigma, t_max, step_size, p_remove,
             seed, rtol=1e-8, atol=1e-10, max_steps=DEFAULT_MAX_STEPS, noise=None, return_noise=False, return_steps=False):
    """Integrate every patient of ``init`` (N, D) over the grid ``0, step_size, .., t_max`` and form the data set.

    ``dose_time`` (N, K) and ``dose_amount`` (N,) are the dose schedule, ``roche_config`` the 13 rate constants in the
    order of ``sim_config.RochConfig``, ``ml_coef`` (D, D - 4) and ``output_coef`` (obs, D + 1) the generator's
    coefficients.  ``noise`` (T, N, obs), when given, replaces the kernel's own draw of the output noise.  Returns a dict of
    device tensors in the time-major layout: ``latents`` (T, N, D), ``actions`` (T, N, 1), ``measurements`` and ``masks``
    (T, N, obs), all float32; ``status`` (N,) int32; ``mean`` and ``std`` (obs,) float64 of the raw outputs; ``noise``
    (T, N, obs) float64 with ``return_noise`` and ``steps`` (N,) int32 with ``return_steps``.

    A patient whose state turns non-finite, or who needs more than ``max_steps`` attempted steps in one grid interval, has
    ``status`` = the first grid index it has no state for (-1 for index 0; 0 means fine); its latents, actions and
    measurements are zero from there on and its masks 0.  The reference pads a failed patient with zeros in the same way;
    its ``mask[latents.shape[1]:] = 0`` is evidently meant to mask the padding but runs after it, so it is a no-op there."""
    init = _tensor(init)
    if init.dim() != 2:
        _refuse("init must be (N, D), got %s" % (tuple(init.shape),))
    dose_time, dose_amount = _tensor(dose_time, init), _tensor(dose_amount, init)
    ml_coef, output_coef = _tensor(ml_coef, init), _tensor(output_coef, init)
    N, D = init.shape
    if dose_time.dim() == 1:
        dose_time = dose_time[:, None]
    K, obs, T = dose_time.shape[-1], output_coef.shape[0], n_times(t_max, step_size)
    if D not in GL.DIMS:
        _refuse("latent_dim %d has no compiled kernel %s" % (D, GL.DIMS))
    if N < 1 or T < 2:
        _refuse("needs at least one patient and two grid points (N %d, T %d)" % (N, T))
    if not 1 <= obs <= GL.MAX_OBS:
        _refuse("obs %d outside 1..%d" % (obs, GL.MAX_OBS))
    if not 1 <= K <= GL.MAX_DOSES:
        _refuse("%d doses per patient, outside 1..%d" % (K, GL.MAX_DOSES))
    if T * N > 2 ** 31 - 1:
        _refuse("T * N = %d exceeds 2^31 - 1" % (T * N))
    for name, x, shape in (("dose_time", dose_time, (N, K)), ("dose_amount", dose_amount, (N,)),
                           ("ml_coef", ml_coef, (D, D - 4)), ("output_coef", output_coef, (obs, D + 1))):
        if tuple(x.shape) != shape:
            _refuse("%s shape %s != %s" % (name, tuple(x.shape), shape))
    if noise is not None and tuple(noise.shape) != (T, N, obs):
        _refuse("noise shape %s != %s" % (tuple(noise.shape), (T, N, obs)))
    theta = [float(v) for v in roche_config]
    if len(theta) != GL.N_THETA:
        _refuse("roche_config has %d entries, not %d" % (len(theta), GL.N_THETA))
    _require_gpu(init, dose_time, dose_amount, ml_coef, output_coef, noise)
    lib = GL.lib()
    dev = init.device
    # float64 inputs are staged into buffers of this call's own (whatever dtype, stride or offset they came with)
    init64 = torch.empty((N, D), device=dev, dtype=torch.float64)
    init64.copy_(init)
    times64 = torch.empty((N, K), device=dev, dtype=torch.float64)
    times64.copy_(dose_time)
    amount64 = torch.empty((N,), device=dev, dtype=torch.float64)
    amount64.copy_(dose_amount)
    ml64 = torch.empty((D, max(D - 4, 1)), device=dev, dtype=torch.float64)
    if D > 4:
        ml64.copy_(ml_coef)
    oc64 = torch.empty((obs, D + 1), device=dev, dtype=torch.float64)
    oc64.copy_(output_coef)
    noisec = _f32c(noise) if noise is not None else None
    latents = torch.empty((T, N, D), device=dev, dtype=torch.float32)
    actions = torch.empty((T, N, 1), device=dev, dtype=torch.float32)
    measurements = torch.empty((T, N, obs), device=dev, dtype=torch.float32)
    masks = torch.empty((T, N, obs), device=dev, dtype=torch.float32)
    status = torch.empty((N,), device=dev, dtype=torch.int32)
    steps = torch.empty((N,), device=dev, dtype=torch.int32) if return_steps else None
    noise_out = torch.empty((T, N, obs), device=dev, dtype=torch.float64) if return_noise else None
    ws_bytes = int(lib.hode_datagen_workspace_bytes(N, obs))
    ws = torch.empty((ws_bytes // 8,), device=dev, dtype=torch.float64)
    d = GL.new_desc()
    d.n_patients, d.n_times, d.latent_dim, d.obs_dim, d.n_dose, d.max_steps = N, T, D, obs, K, int(max_steps)
    d.seed = int(seed) & (2 ** 64 - 1)
    d.step, d.rtol, d.atol, d.sigma, d.p_remove = float(step_size), float(rtol), float(atol), float(output_sigma), float(p_remove)
    for i, v in enumerate(theta):
        d.theta[i] = v
    d.init, d.dose_times, d.dose_amount = init64.data_ptr(), times64.data_ptr(), amount64.data_ptr()
    d.ml_coef, d.output_coef = ml64.data_ptr(), oc64.data_ptr()
    d.noise = noisec.data_ptr() if noisec is not None else 0
    d.latents, d.actions, d.measurements, d.masks = latents.data_ptr(), actions.data_ptr(), measurements.data_ptr(), masks.data_ptr()
    d.noise_out = noise_out.data_ptr() if noise_out is not None else 0
    d.status = status.data_ptr()
    d.steps = steps.data_ptr() if steps is not None else 0
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
    with torch.cuda.device(dev):
        GL.check(lib.hode_datagen_generate(d, _stream()), "hode_datagen_generate")
    out = {"latents": latents, "actions": actions, "measurements": measurements, "masks": masks, "status": status,
           "mean": ws[:obs], "std": ws[obs:2 * obs]}
    if return_noise:
        out["noise"] = noise_out
    if return_steps:
        out["steps"] = steps
    return out
