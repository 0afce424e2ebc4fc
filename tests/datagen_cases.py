"""Inputs shared by the host and GPU tests of the synthetic data generator: the three recorded runs of the reference
(G14, tests/golden/make_golden_generator.py) and seeded cases of the other dimensions, each with its float64 yardstick
(tests/datagen_eager.py) computed once per process."""
import functools
import os

import numpy as np

import datagen_eager as eager

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_generator.npz")
RTOL, ATOL = 1e-8, 1e-10          # the kernel's defaults
FIXTURE_CASES = ("g14_dim8", "g14_dim12", "g14_dim4")
SEEDED_CASES = ("d6_half_step", "d20", "d4_lone")


@functools.lru_cache(maxsize=None)
def g14():
    return np.load(GOLDEN)


def replay_noise(state_after_draws, n, obs, T):
    """The reference's output noise: patient i's is the i-th randn(obs, T) after get_action (LSODA draws nothing)."""
    np.random.set_state(state_after_draws)
    return np.stack([np.random.randn(obs, T) for _ in range(n)]).transpose(2, 0, 1)      # (T, N, obs)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: init (N, D), dose_time (N, K), dose_amount (N,), ml_coef, output_coef (obs, D + 1), sigma, t_max, step."""
    if name in FIXTURE_CASES:
        g, p = g14(), "c%d_" % FIXTURE_CASES.index(name)
        cfg = g[p + "config"]
        return dict(init=g[p + "init"], dose_time=g[p + "dose_time"].astype(np.float64), dose_amount=g[p + "dose_amount"],
                    ml_coef=g[p + "ml_coef"], output_coef=g[p + "output_coef"], sigma=float(cfg[6]), t_max=int(cfg[2]),
                    step=float(cfg[3]), p_remove=float(cfg[8]), prefix=p)
    rng = np.random.default_rng({"d6_half_step": 61, "d20": 201, "d4_lone": 41}[name])
    D, N, obs, K, t_max, step = {"d6_half_step": (6, 65, 1, 2, 7, 0.5), "d20": (20, 65, 20, 1, 14, 1.0),
                                 "d4_lone": (4, 1, 1, 1, 14, 1.0)}[name]
    if name == "d6_half_step":   # first dose on an even grid index (every other grid point), the second off the grid
        dose_time = np.stack([rng.integers(0, t_max, N).astype(np.float64), rng.uniform(0, t_max, N)], axis=1)
    else:
        dose_time = rng.integers(0, t_max, (N, K)).astype(np.float64)
    return dict(init=rng.exponential(0.01, (N, D)), dose_time=dose_time, dose_amount=rng.uniform(0, 10, N),
                ml_coef=rng.standard_normal((D, D - 4)) * rng.binomial(1, 0.5, (D, D - 4)) / D,
                output_coef=rng.standard_normal((obs, D + 1)), sigma=0.2, t_max=t_max, step=step, p_remove=0.5, prefix=None)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """(latents (T, N, D) float64 of the tight integration, E): E is the maximum error of scipy RK45 at the kernel's own
    rtol / atol on the same inputs against it."""
    c = case(name)
    a = (c["init"], c["dose_time"], c["dose_amount"], c["ml_coef"], c["t_max"], c["step"])
    tight = eager.latents(*a)
    E = np.abs(eager.latents(*a, method="RK45", rtol=RTOL, atol=ATOL) - tight).max()
    return tight, float(E)


def latent_bound(tight, E):
    """|latents - yardstick| <= 2^-23 |yardstick| + 4 E: the float32 store, and 4 x the error of another Dormand-Prince
    controller at the same tolerances."""
    return 2.0 ** -23 * np.abs(tight) + 4.0 * E
