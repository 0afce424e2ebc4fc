#!/usr/bin/env python
"""Sylvester-flow timing on the device: the fused pair (hode_sylvester_fwd + hode_sylvester_bwd through
flow.sylvester_chain and autograd) against the reference-style eager loop (flow.Sylvester's arithmetic, one module call
per draw and flow, autograd backward) on the same device in the same call, and each kernel on its own
through the plain launch functions of hode.sylvester.  HIP events, median of `--reps` timed repeats; every shape is warmed
up first and the clock is ramped by a quarter of a second of the fused pair before anything is timed.  Prints one line per
measurement and a JSON summary line.

    python tools/sylvester_probe.py [--reps 50] [--no-eager]

Per-kernel times: the same probe with --no-eager under `rocprofv3 --kernel-trace --stats` (the two shapes run different
tiles, so the statistics keep them apart by kernel name)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-ode-neurips-2021_amd")]

import flow  # noqa: E402
from hode.sylvester import sylvester_backward, sylvester_forward  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
SHAPES = ((10, 6, 6, 4, 51), (10000, 12, 12, 4, 51))  # (B, D, M, K, S)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def ramp(fn, seconds=0.25):
    t0 = time.time()
    while time.time() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def inputs(B, D, M, K, S):
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731

    def tri():
        r = torch.triu(rn(B, K, M, M), diagonal=1) / M ** 0.5 + 0.02 * rn(B, K, M, M)
        diag = (torch.rand(B, K, M, device=DEV, generator=g) * 2 - 1) * 0.94
        return (r - torch.diag_embed(torch.diagonal(r, dim1=-2, dim2=-1)) + torch.diag_embed(diag)).requires_grad_(True)

    q = torch.linalg.qr(rn(B, K, D, M))[0].contiguous().requires_grad_(True)
    return rn(S, B, D).requires_grad_(True), tri(), tri(), (0.3 * rn(B, K, M)).requires_grad_(True), q


def fused_step(z0, r1, r2, b, q):
    z, logdet = flow.sylvester_chain(z0, r1, r2, b, q)
    (z.sum() + logdet.mean()).backward()


def eager_step(mods, z0, r1, r2, b, q):
    """The reference's arithmetic: one Sylvester module call per draw and flow on (B, D) tensors, autograd backward."""
    zs, lds = [], []
    for s in range(z0.shape[0]):
        z, logdet = z0[s], 0.0
        for k, mod in enumerate(mods):
            z, ld = mod._eager(z, r1[:, k], r2[:, k], q[:, k], b[:, k].unsqueeze(1))
            logdet = logdet + ld
        zs.append(z)
        lds.append(logdet)
    (torch.stack(zs).sum() + torch.stack(lds).mean()).backward()


class _EagerSylvester(flow.Sylvester):
    """flow.Sylvester held to its eager arithmetic on the device (the module itself would take the kernel there)."""

    def _eager(self, zk, r1, r2, q, b):
        z, log_diag = flow._sylvester_step_eager(zk, r1, r2, b.reshape(b.shape[0], -1), q)
        return z, log_diag.sum(-1)


def algorithmic_bytes(B, D, M, K, S):
    """Per direction: the draws' state once per flow in and out (the flows are streamed, the state lives in memory
    between them), logdet once per flow, the parameters (and, backward, their gradients) once."""
    params = 4 * B * K * (2 * M * M + M + D * M)
    state = 4 * S * B * D
    fwd = K * 2 * state + K * 2 * 4 * S * B + params
    bwd = K * 3 * state + state + 4 * S * B + 2 * params   # z_k and zbar in, zbar out per flow; grad_z once
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-eager", action="store_true", help="skip the eager loop (for a run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    res = {}
    for B, D, M, K, S in SHAPES:
        z0, r1, r2, b, q = inputs(B, D, M, K, S)
        mods = [_EagerSylvester(M).to(DEV) for _ in range(K)]
        plain = [t.detach() for t in (z0, r1, r2, b, q)]
        gz, gl = torch.ones(S, B, D, device=DEV), torch.full((S, B), 1.0 / (S * B), device=DEV)
        tape = sylvester_forward(*plain)[3]
        ramp(lambda: fused_step(z0, r1, r2, b, q), 0.02 if a.no_eager else 0.25)   # a short one keeps a kernel trace small
        t_fwd = timed(lambda: sylvester_forward(*plain), a.reps)
        t_bwd = timed(lambda: sylvester_backward(*plain, None, tape, gz, gl), a.reps)
        t_pair = timed(lambda: fused_step(z0, r1, r2, b, q), a.reps)
        t_eager = float("nan") if a.no_eager else timed(lambda: eager_step(mods, z0, r1, r2, b, q), max(5, a.reps // 5), warmup=3)
        t_pair2 = timed(lambda: fused_step(z0, r1, r2, b, q), a.reps)   # again after the eager loop: the spread
        fb, bb = algorithmic_bytes(B, D, M, K, S)
        key = "B%d_D%d_M%d_K%d_S%d" % (B, D, M, K, S)
        res[key] = {"fwd_kernel_us": t_fwd, "bwd_kernel_us": t_bwd, "fused_fwd_bwd_us": t_pair, "fused_fwd_bwd_again_us": t_pair2,
                    "eager_fwd_bwd_us": t_eager, "speedup": t_eager / t_pair, "bytes_fwd": fb, "bytes_bwd": bb,
                    "fwd_bw_frac_of_peak": fb / (t_fwd * 1e-6) / HBM_PEAK, "bwd_bw_frac_of_peak": bb / (t_bwd * 1e-6) / HBM_PEAK}
        print("%s: fwd launch %.1f us, bwd launch %.1f us, fused fwd+bwd through autograd %.1f / %.1f us, eager loop fwd+bwd "
              "%.1f us (x%.1f); algorithmic bytes fwd %d / bwd %d: %.2f%% / %.2f%% of HBM peak"
              % (key, t_fwd, t_bwd, t_pair, t_pair2, t_eager, t_eager / t_pair, fb, bb,
                 100 * res[key]["fwd_bw_frac_of_peak"], 100 * res[key]["bwd_bw_frac_of_peak"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
