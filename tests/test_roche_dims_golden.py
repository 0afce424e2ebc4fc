"""The CPU oracle against the reference's RocheODE at the latent sizes 5, 7, 10, 15, 16 (G16,
tests/golden/make_golden_roche_dims.py; no GPU), as tests/test_oracle_golden.py holds G1: values bit-exact, VJPs to
rtol 1e-6 (state) / 1e-5 (parameters).  The absolute floor of the state VJP is one fp32 ulp of the largest entry of the
vector, 2^-23 max|gy|, instead of G1's 1e-7: an entry is a sum of up to D products whose partial sums are as large as the
largest entry, and the oracle's matmul may add them in another order than the reference's (it does at D = 16); a reordered
sum moves by an ulp of its largest partial sum."""
import os

import numpy as np
import torch

from oracle import rhs as orhs


def _load(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_roche_dims.npz"), allow_pickle=False)


def test_g16_is_small_and_holds_the_sizes(golden_dir):
    g = _load(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "g16_roche_dims.npz")) < 200 * 1024
    assert [int(d) for d in g["dims"]] == [5, 7, 10, 15, 16]
    seen = {(int(g["c%d_meta" % ci][0]), bool(g["c%d_meta" % ci][1])) for ci in range(int(g["n_cases"]))}
    assert seen == {(D, a) for D in (5, 7, 10, 15, 16) for a in (False, True)}
    for k in g.files:
        assert g[k].dtype.kind in "fiUb", k   # arrays and short tags only


def test_g16_roche_rhs_values_and_vjp(golden_dir):
    g = _load(golden_dir)
    for ci in range(int(g["n_cases"])):
        pre = "c%d_" % ci
        D, ablate, T, B = [int(v) for v in g[pre + "meta"]]
        f = orhs.RocheRHS(D, float(g[pre + "step"]), ablate=bool(ablate))
        f.load_state_dict({k[len(pre) + 3:].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "sd_")},
                          strict=True)
        f.set_action(torch.from_numpy(g[pre + "action"]))
        np.testing.assert_array_equal(f.times.numpy(), g[pre + "times"])
        np.testing.assert_array_equal(f.dosage.numpy(), g[pre + "dosage"])
        y, cot = torch.from_numpy(g[pre + "y"]), torch.from_numpy(g[pre + "cot"])
        ts = g[pre + "t"]
        # exactly at a dose time, one ulp before it and one ulp after
        assert ts[2] < ts[3] < ts[4] and ts[3] == np.float32(1.0) and np.nextafter(ts[2], np.float32(9)) == ts[3]
        assert np.nextafter(ts[3], np.float32(9)) == ts[4]
        if not ablate:
            assert np.abs(g[pre + "dose"][2] - g[pre + "dose"][3]).max() > 0.1   # the dose at t8 is seen at t8, not one ulp before
        for ti, t in enumerate(ts):
            tt = torch.tensor(float(t), dtype=torch.float32)
            yy = y.clone().requires_grad_(True)
            out = f(tt, yy)
            np.testing.assert_array_equal(out.detach().numpy(), g[pre + "f"][ti])
            np.testing.assert_array_equal(f.dose_at_time(tt).detach().numpy(), g[pre + "dose"][ti])
            f.zero_grad()
            (out * cot).sum().backward()
            want = g[pre + "gy"][ti]
            np.testing.assert_allclose(yy.grad.numpy(), want, rtol=1e-6, atol=2.0 ** -23 * float(np.abs(want).max()))
            for n, p in f.named_parameters():
                want = g[pre + "g_" + n.replace(".", "__")][ti]
                got = p.grad.numpy() if p.grad is not None else np.zeros_like(want)
                np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=n)
