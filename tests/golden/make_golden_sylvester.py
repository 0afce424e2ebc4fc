#!/usr/bin/env python
"""Generate ``tests/golden/g19_sylvester.npz`` (G19) from the REFERENCE's Sylvester flows: ``Sylvester`` (flow.py:62-138)
and ``TriangularSylvester`` (flow.py:141-219).

Run in the build container only, like ``make_golden_flow.py``:

    HODE_REFERENCE_TREE=<checkout of the reference> python tests/golden/make_golden_sylvester.py

Every record holds the inputs, the outputs and the autograd gradients of ``sum(z' gz) + sum(ldj gl)`` for every
floating-point input, once in float32 (prefix ``f32_``) and once in float64 (``f64_``, the same numbers cast up):

    syl_sum, syl_terms      Sylvester.forward with sum_ldj True / False            (B 5, D 6, M 4)
    tri_none, tri_flip, tri_perm
                            TriangularSylvester._forward without a permutation, with the flip and with a permutation
                            that is no involution, sum_ldj True / False / True     (B 5, D 5)
    tri_quirk               TriangularSylvester.forward(zk, r1, r2, bias, perm, True): its fourth argument is the bias
    chain3                  three Sylvester.forward calls in a row, sum_ldj False: z_3, the three (B, M) term blocks
                            stacked as (B, 3, M), with parameters (B, 3, ...)

Only arrays are written (``allow_pickle=False`` loads it)."""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HODE_REFERENCE_TREE")
if not REF:
    sys.exit("set HODE_REFERENCE_TREE to a checkout of the reference code base")
sys.path.insert(0, REF)

import flow  # noqa: E402  (reference)

B, D, M, DT = 5, 6, 4, 5
PERM = [2, 0, 3, 4, 1]   # a 5-cycle: no involution
FLIP = [4, 3, 2, 1, 0]


def npy(x):
    return x.detach().cpu().numpy()


def params(g, m, k=None):
    """r1, r2: upper triangular plus a small dense perturbation, |diagonal| <= 0.9."""
    shape = (B, m, m) if k is None else (B, k, m, m)
    out = []
    for _ in range(2):
        r = torch.triu(torch.randn(*shape, generator=g), diagonal=1) / m ** 0.5 + 0.02 * torch.randn(*shape, generator=g)
        diag = (torch.rand(*shape[:-1], generator=g) * 2 - 1) * 0.9
        out.append(r - torch.diag_embed(torch.diagonal(r, dim1=-2, dim2=-1)) + torch.diag_embed(diag))
    return out


def record(out, pre, fn, ins, dtype, extra=None):
    """ins: name -> float tensor; fn(**leaves) -> (z, ldj).  Stores inputs, outputs, cotangents and gradients."""
    g = torch.Generator().manual_seed(sum(map(ord, pre[4:])))   # the same cotangents under both dtype prefixes
    leaves = {n: t.to(dtype).requires_grad_(True) for n, t in ins.items()}
    z, ldj = fn(**leaves)
    gz = torch.randn(z.shape, generator=g).to(dtype)
    gl = torch.randn(ldj.shape, generator=g).to(dtype)
    grads = torch.autograd.grad((z * gz).sum() + (ldj * gl).sum(), list(leaves.values()))
    for n, t in leaves.items():
        out[pre + "in_" + n] = npy(t)
    for (n, _), gr in zip(leaves.items(), grads):
        out[pre + "grad_" + n] = npy(gr)
    out[pre + "z"], out[pre + "ldj"], out[pre + "gz"], out[pre + "gl"] = npy(z), npy(ldj), npy(gz), npy(gl)
    for n, v in (extra or {}).items():
        out[pre + n] = np.asarray(v)


def main():
    out = {}
    for tag, dtype in (("f32_", torch.float32), ("f64_", torch.float64)):
        g = torch.Generator().manual_seed(19)
        syl, tri = flow.Sylvester(M).to(dtype), flow.TriangularSylvester(DT).to(dtype)
        r1, r2 = params(g, M)
        q = torch.linalg.qr(torch.randn(B, D, M, generator=g))[0] + 0.02 * torch.randn(B, D, M, generator=g)
        ins = {"zk": torch.randn(B, D, generator=g), "r1": r1, "r2": r2, "q": q, "b": 0.3 * torch.randn(B, 1, M, generator=g)}
        for name, sum_ldj in (("syl_sum_", True), ("syl_terms_", False)):
            record(out, tag + name, lambda zk, r1, r2, q, b, s=sum_ldj: syl(zk, r1, r2, q, b, s), ins, dtype)

        t1, t2 = params(g, DT)
        tins = {"zk": torch.randn(B, DT, generator=g), "r1": t1, "r2": t2, "b": 0.3 * torch.randn(B, 1, DT, generator=g)}
        for name, perm, sum_ldj in (("tri_none_", None, True), ("tri_flip_", FLIP, False), ("tri_perm_", PERM, True)):
            p = None if perm is None else torch.tensor(perm)
            record(out, tag + name, lambda zk, r1, r2, b, p=p, s=sum_ldj: tri._forward(zk, r1, r2, b, p, s), tins, dtype,
                   {} if perm is None else {"perm": np.asarray(perm, dtype=np.int64)})
        record(out, tag + "tri_quirk_", lambda zk, r1, r2, b: tri(zk, r1, r2, b, torch.tensor(PERM), True), tins, dtype,
               {"perm": np.asarray(PERM, dtype=np.int64)})

        c1, c2 = params(g, M, 3)
        cq = torch.linalg.qr(torch.randn(B, 3, D, M, generator=g))[0] + 0.02 * torch.randn(B, 3, D, M, generator=g)
        cins = {"zk": torch.randn(B, D, generator=g), "r1": c1, "r2": c2, "q": cq, "b": 0.3 * torch.randn(B, 3, M, generator=g)}

        def chain(zk, r1, r2, q, b):
            terms = []
            for k in range(3):
                zk, t = syl(zk, r1[:, k], r2[:, k], q[:, k], b[:, k].unsqueeze(1), False)
                terms.append(t)
            return zk, torch.stack(terms, dim=1)
        record(out, tag + "chain3_", chain, cins, dtype)
    path = os.path.join(HERE, "g19_sylvester.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
