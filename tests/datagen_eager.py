"""The float64 yardstick of the synthetic data generator, independent of the code under test: the generator's right-hand
side restated in numpy and integrated by scipy DOP853 at rtol 1e-12 / atol 1e-14, restarted at every dose time (so the
right-hand side is smooth inside every call); Philox4x32-10 in uint32 arithmetic with a float64 Box-Muller; the readout,
the float32 rounding of the raw values, mean / unbiased std, the z-score and the masks."""
import numpy as np

THETA = (2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)   # sim_config.RochConfig()


def grid(t_max, step):
    """The reference's grid: int(t_max / step + 1) points i * step."""
    return np.arange(int(t_max / step + 1)) * float(step)


def make_rhs(theta, ml_coef, taus, amount):
    """dataloader.py:105-149 with the doses `taus` active (all of them given at or before the piece starts)."""
    hc, hp, ec50, emax, kdexa, kcir, kci, kprog, kid, kfb, koff, kim, kel = (float(v) for v in theta)
    taus = np.asarray(taus, dtype=np.float64)

    def f(t, y):
        dis, ir, imm, d2 = y[0], y[1], y[2], y[3]
        dose = amount * np.sum(np.exp(kel * (taus - t)))
        out = np.empty_like(y)
        out[0] = dis * kprog - dis * imm ** hc * kci - dis * ir * kcir
        out[1] = dis * kid - ir * koff + dis * ir * kfb + (ir ** hp * emax) / (ec50 ** hp + ir ** hp) - d2 * ir * kdexa
        out[2] = ir * kim
        out[3] = kel * dose - kel * d2
        if y.shape[0] > 4:
            out[4:] = np.tanh(y @ ml_coef)
        return out
    return f


def latents(init, dose_time, dose_amount, ml_coef, t_max, step, theta=THETA, method="DOP853", rtol=1e-12, atol=1e-14,
            dense=None):
    """(T, N, D) float64 states on the grid.  The integration restarts at every dose time; with `dense` (the default for
    the tight DOP853 run, whose 7th-order interpolant is then as good as its steps) the grid points between two doses are
    read from one call's dense output, otherwise the integration restarts at every grid point too."""
    from scipy.integrate import solve_ivp
    dense = (method == "DOP853" and rtol <= 1e-11) if dense is None else dense
    init = np.asarray(init, dtype=np.float64)
    dose_time = np.asarray(dose_time, dtype=np.float64).reshape(init.shape[0], -1)
    ts = grid(t_max, step)
    out = np.zeros((len(ts),) + init.shape)
    for n in range(init.shape[0]):
        y = init[n].copy()
        out[0, n] = y
        inner = {float(t) for t in dose_time[n] if ts[0] < t < ts[-1]}
        cuts = sorted(inner | ({ts[0], ts[-1]} if dense else set(ts.tolist())))
        for lo, hi in zip(cuts, cuts[1:]):
            active = dose_time[n][dose_time[n] <= lo]
            at = np.nonzero((ts > lo) & (ts <= hi))[0]
            sol = solve_ivp(make_rhs(theta, ml_coef, active, float(dose_amount[n])), (lo, hi), y, method=method, rtol=rtol,
                            atol=atol, t_eval=(ts[at] if len(at) and ts[at[-1]] == hi else np.append(ts[at], hi)) if dense else None)
            assert sol.success
            y = sol.y[:, -1]
            out[at, n] = sol.y[:, :len(at)].T if dense else y[None, :]
    return out


def actions(dose_time, dose_amount, t_max, step):
    """(T, N, 1): amount where some dose time equals the grid time (dose_at_time_discrete)."""
    ts = grid(t_max, step)
    dose_time = np.asarray(dose_time, dtype=np.float64).reshape(len(dose_amount), -1)
    hit = (dose_time[None, :, :] == ts[:, None, None]).any(axis=2)
    return (hit * np.asarray(dose_amount, dtype=np.float64)[None, :])[:, :, None]


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays: ten rounds over the counters (arrays, broadcast together) with the key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & _MASK, int(k1) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(_MASK), p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _words(seed, T, N, obs, stream):
    t, n, o = np.meshgrid(np.arange(T), np.arange(N), np.arange(obs), indexing="ij")
    return philox(t, n, o, stream, seed & _MASK, (seed >> 32) & _MASK)


def normal(seed, T, N, obs):
    """(T, N, obs) float64: Box-Muller on words 0 and 1 of stream 0."""
    w = _words(seed, T, N, obs, 0)
    u1, u2 = (w[0].astype(np.float64) + 0.5) * 2.0 ** -32, (w[1].astype(np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def uniform(seed, T, N, obs):
    """(T, N, obs) float64 in (0, 1): word 0 of stream 1."""
    return (_words(seed, T, N, obs, 1)[0].astype(np.float64) + 0.5) * 2.0 ** -32


# ---- readout -----------------------------------------------------------------------------------------------------------
def raw_outputs(lat, output_coef, sigma, eps):
    """(T, N, obs) float64, before the float32 rounding."""
    D = lat.shape[2]
    return lat @ output_coef[:, :D].T + output_coef[:, D] + sigma * eps


def zscore(raw):
    """The float32-rounded raw values, their float64 mean and unbiased std per channel, and the z-score in float64."""
    r32 = raw.astype(np.float32).astype(np.float64)
    mean, std = r32.mean(axis=(0, 1)), r32.std(axis=(0, 1), ddof=1)
    return r32, mean, std, (r32 - mean) / std
