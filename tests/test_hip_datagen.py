"""GPU tests of the synthetic data generator (libhode_datagen.so, hode.datagen.simulate, dataloader.DataGeneratorRoche)
against the float64 yardstick of tests/datagen_eager.py and the reference's recorded runs (G14)."""
import numpy as np
import pytest
import torch

import datagen_cases as cases
import datagen_eager as eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _simulate(c, seed=5, **kw):
    from hode import datagen
    dev = torch.device(DEV)
    put = lambda x: torch.as_tensor(x).to(dev)
    out = datagen.simulate(put(c["init"]), put(c["dose_time"]), put(c["dose_amount"]), eager.THETA, put(c["ml_coef"]),
                           put(c["output_coef"]), c["sigma"], c["t_max"], c["step"], kw.pop("p_remove", c["p_remove"]), seed, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def runs():
    """One plain call per case, with the drawn noise, shared by the tests below (never modified)."""
    return {name: _simulate(cases.case(name), return_noise=True, return_steps=True)
            for name in cases.FIXTURE_CASES + cases.SEEDED_CASES}


# ---------------------------------------------------------------------------------------------------------- 1. latents
@pytest.mark.parametrize("name", cases.FIXTURE_CASES + cases.SEEDED_CASES)
def test_latents_against_the_float64_yardstick(runs, name):
    tight, E = cases.yardstick(name)
    got = runs[name]
    err = np.abs(got["latents"].astype(np.float64) - tight)
    print(name, "max err %.3e  E %.3e  steps mean %.1f max %d" % (err.max(), E, got["steps"].mean(), got["steps"].max()))
    assert got["latents"].dtype == np.float32 and got["latents"].shape == tight.shape
    assert (got["status"] == 0).all()
    assert (err <= cases.latent_bound(tight, E)).all(), (err - cases.latent_bound(tight, E)).max()


# ---------------------------------------------------------------------------------------------------- 2. dose handling
DOSE_CASES = {
    # (t_max, step, dose_time rows, amounts)
    "index0_last_zero": (14, 1.0, [[0.0], [13.0], [5.0]], [3.0, 7.0, 0.0]),
    "two_inside_same": (7, 0.5, [[1.0, 2.25], [3.3, 3.7], [2.0, 2.0], [0.0, 6.5]], [2.0, 5.0, 4.0, 9.0]),
    "eight": (14, 1.0, [[0.0, 1.5, 2.0, 2.0, 6.25, 6.75, 12.0, 13.0], [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5]], [1.5, 2.5]),
}


@pytest.mark.parametrize("name", sorted(DOSE_CASES))
def test_dose_handling(name):
    t_max, step, times, amounts = DOSE_CASES[name]
    rng = np.random.default_rng(8)
    N, D, obs = len(times), 8, 3
    c = dict(init=rng.exponential(0.01, (N, D)), dose_time=np.array(times), dose_amount=np.array(amounts),
             ml_coef=rng.standard_normal((D, 4)) / D, output_coef=rng.standard_normal((obs, D + 1)), sigma=0.2, t_max=t_max,
             step=step, p_remove=0.5)
    got = _simulate(c)
    want_a = eager.actions(c["dose_time"], c["dose_amount"], t_max, step)
    assert np.array_equal(got["actions"], want_a.astype(np.float32))
    a = (c["init"], c["dose_time"], c["dose_amount"], c["ml_coef"], t_max, step)
    tight = eager.latents(*a)
    E = np.abs(eager.latents(*a, method="RK45", rtol=cases.RTOL, atol=cases.ATOL) - tight).max()
    err = np.abs(got["latents"].astype(np.float64) - tight)
    print(name, "max err %.3e  E %.3e" % (err.max(), E))
    assert (got["status"] == 0).all() and (err <= cases.latent_bound(tight, E)).all()
    if name == "two_inside_same":
        assert not got["actions"][:, 1].any()                       # both doses off the grid: no action ...
        no_dose = eager.latents(c["init"][1:2], [[100.0, 100.0]], [0.0], c["ml_coef"], t_max, step)
        assert np.abs(tight[:, 1:2] - no_dose).max() > 1e-2          # ... and the latents still move, as the yardstick says
        assert got["actions"][4, 2, 0] == 4.0 and np.count_nonzero(got["actions"][:, 2]) == 1   # two doses at one time


# ----------------------------------------------------------------------------------------- 3. measurements, given noise
def _measurement_bound(c, lat_bound, raw, std):
    """Per element: float32 rounding of the raw value over the channel's std, float32 rounding of the result, and the
    latent bound times sum_j |output_coef[o, j]| / std_o (the offset column takes no latent error)."""
    D = c["init"].shape[1]
    z = (raw - raw.mean(axis=(0, 1))) / std
    gain = np.abs(c["output_coef"][:, :D])                                     # (obs, D)
    return 2.0 ** -24 * np.abs(raw) / std + 2.0 ** -24 * np.abs(z) + (lat_bound @ gain.T) / std


@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_measurements_with_the_recorded_noise(name):
    import sim_config
    import dataloader
    c, g = cases.case(name), cases.g14()
    p, cfg = c["prefix"], cases.g14()[c["prefix"] + "config"]
    N, val, test, seed = (int(v) for v in g["meta"][:4])
    n_noise, n_meas = int(g["meta"][4]), int(g["meta"][5])
    np.random.seed(seed)
    dg = dataloader.DataGeneratorRoche(N, int(cfg[0]), int(cfg[2]), cfg[3], sim_config.RochConfig(), cfg[6], cfg[7], int(cfg[1]),
                                       cfg[4], cfg[5], val, test, cfg[8], device=torch.device("cpu"))
    dg.get_initial_conditions()
    dg.get_action()
    T, obs, D = dg.time_dim, dg.obs_dim, dg.latent_dim
    noise = cases.replay_noise(np.random.get_state(), N, obs, T)
    assert np.array_equal(noise[:, :n_noise], g[p + "noise"])                  # the replay is the recorded draw
    fed = noise.astype(np.float32)
    got = _simulate(c, noise=torch.from_numpy(fed).to(DEV))
    tight, E = cases.yardstick(name)
    lat_bound = cases.latent_bound(tight, E)
    raw, mean, std, z = eager.zscore(eager.raw_outputs(tight, c["output_coef"], c["sigma"], fed.astype(np.float64)))
    np.testing.assert_allclose(got["mean"], mean, rtol=1e-6, atol=1e-6 * std.max())
    np.testing.assert_allclose(got["std"], std, rtol=1e-6)
    bound = _measurement_bound(c, lat_bound, raw, std)
    err = np.abs(got["measurements"].astype(np.float64) - z)
    print(name, "vs eager: max err %.3e, max err / bound %.3f" % (err.max(), (err / bound).max()))
    assert (err <= bound).all()
    # against the reference's own measurements.  Its raw values differ from the eager form's by delta: its latents' distance
    # from the yardstick, propagated the same way, the float32 rounding of the noise as fed, and its own float32 rounding of
    # the raw value.  That moves its mean by at most mean(delta) and its std by at most sqrt(sum delta^2 / (n - 1)) (the
    # std is a seminorm of the raw values), and its z-score runs in float32 (the last term: a few roundings of z, of the
    # raw value and of the mean).
    ref_lat = np.abs(g[p + "latents"].astype(np.float64) - tight)
    gain = np.abs(c["output_coef"][:, :D])
    delta = ref_lat @ gain.T + c["sigma"] * np.abs(noise) * 2.0 ** -24 + 2.0 ** -24 * np.abs(raw)
    d_mean = delta.mean(axis=(0, 1))
    d_std = np.sqrt((delta ** 2).sum(axis=(0, 1)) / (T * N - 1))
    bound_ref = bound + (delta + d_mean) / std + np.abs(z) * d_std / (std - d_std) \
        + 2.0 ** -23 * (np.abs(z) + (np.abs(raw) + np.abs(mean)) / std)
    err_ref = np.abs(got["measurements"][:, :n_meas].astype(np.float64) - g[p + "measurements"].astype(np.float64))
    print(name, "vs reference: max err %.3e, max err / bound %.3f" % (err_ref.max(), (err_ref / bound_ref[:, :n_meas]).max()))
    assert (err_ref <= bound_ref[:, :n_meas]).all()
    assert np.array_equal(got["actions"], g[p + "actions"])


# ------------------------------------------------------------------------------------------------------- 4. generator
@pytest.fixture(scope="module")
def stats_case():
    rng = np.random.default_rng(9)
    D, obs = 4, 80
    mk = lambda N: dict(init=init[:N], dose_time=dt[:N], dose_amount=am[:N], ml_coef=np.zeros((D, 0)), output_coef=oc, sigma=0.2,
                        t_max=14, step=1.0, p_remove=0.3)
    init, dt, am = rng.exponential(0.01, (200, D)), rng.integers(0, 14, (200, 1)).astype(np.float64), rng.uniform(0, 10, 200)
    oc = rng.standard_normal((obs, D + 1))
    big = _simulate(mk(200), seed=(7 << 32) + 11, return_noise=True)
    return mk, big


def test_noise_and_masks_are_the_philox_restatement(stats_case, runs):
    mk, big = stats_case
    seed = (7 << 32) + 11
    eps, u = eager.normal(seed, 15, 200, 80), eager.uniform(seed, 15, 200, 80)
    assert np.abs(big["noise"] - eps).max() <= 1e-12
    assert np.array_equal(big["masks"], (u > 0.3).astype(np.float32))
    for name in ("d6_half_step", "d20"):                     # obs 1 and 20, seed 5, p_remove 0.5
        T, N, obs = runs[name]["noise"].shape
        assert np.abs(runs[name]["noise"] - eager.normal(5, T, N, obs)).max() <= 1e-12
        assert np.array_equal(runs[name]["masks"], (eager.uniform(5, T, N, obs) > 0.5).astype(np.float32))


def test_same_seed_same_bits_other_seed_differs_and_geometry_does_not_matter(stats_case):
    mk, big = stats_case
    seed = (7 << 32) + 11
    again = _simulate(mk(200), seed=seed, return_noise=True)
    assert np.array_equal(again["measurements"], big["measurements"]) and np.array_equal(again["masks"], big["masks"])
    assert np.array_equal(again["latents"], big["latents"])
    small = _simulate(mk(65), seed=seed, return_noise=True)
    assert np.array_equal(small["noise"], big["noise"][:, :65]) and np.array_equal(small["masks"], big["masks"][:, :65])
    other = _simulate(mk(65), seed=seed + 1, return_noise=True)
    assert not np.array_equal(other["noise"], small["noise"]) and not np.array_equal(other["masks"], small["masks"])
    assert np.array_equal(other["latents"], small["latents"])


def test_mask_and_noise_moments(stats_case):
    mk, big = stats_case
    n = big["masks"].size
    assert abs(big["masks"].mean() - 0.7) <= 4 * np.sqrt(0.7 * 0.3 / n)
    eps = big["noise"]
    assert abs(eps.mean()) <= 4 / np.sqrt(n)
    assert abs(eps.var() - 1.0) <= 4 * np.sqrt(2.0 / n)


# ---------------------------------------------------------------------------------------------------- 5. failure path
def test_step_budget_stops_patients_at_their_first_interval(runs):
    c = cases.case("d6_half_step")
    got = _simulate(c, rtol=1e-12, max_steps=1)
    assert (got["status"] == 1).all()
    for k in ("latents", "actions", "measurements", "masks"):
        assert not got[k][1:].any(), k
    assert np.array_equal(got["latents"][0], c["init"].astype(np.float32))
    want_a0 = eager.actions(c["dose_time"], c["dose_amount"], c["t_max"], c["step"])[0].astype(np.float32)
    assert np.array_equal(got["actions"][0], want_a0)
    assert np.isfinite(got["measurements"][0]).all() and got["measurements"][0].any()
    assert np.array_equal(got["masks"][0], runs["d6_half_step"]["masks"][0])


def test_a_nan_initial_state_is_marked_and_leaves_the_others_alone(runs):
    c = dict(cases.case("d20"))
    init = c["init"].copy()
    init[3, 2] = np.nan
    c["init"] = init
    got = _simulate(c)
    assert got["status"][3] == -1 and (np.delete(got["status"], 3) == 0).all()
    for k in ("latents", "actions", "measurements", "masks"):
        assert not got[k][:, 3].any(), k
    keep = np.arange(65) != 3
    assert np.array_equal(got["latents"][:, keep], runs["d20"]["latents"][:, keep])
    assert np.isfinite(got["measurements"]).all()


# ---------------------------------------------------------------------------------------------------- 6. presentations
def test_presentations_and_a_side_stream(runs):
    from hode import datagen
    c, dev = cases.case("g14_dim8"), torch.device(DEV)
    plain = runs["g14_dim8"]
    N, D = c["init"].shape
    obs = c["output_coef"].shape[0]
    put = lambda x: torch.as_tensor(x).to(dev)
    wide = torch.zeros(N, 2 * D + 1, device=dev, dtype=torch.float64)
    wide[:, 1::2][:, :D] = put(c["init"])
    init_v = wide[:, 1::2][:, :D]                                             # strided, 8-byte offset
    amount_wide = torch.zeros(N, 3, device=dev, dtype=torch.float64)
    amount_wide[:, 1] = put(c["dose_amount"])
    ml_big = torch.zeros(D + 2, D, device=dev, dtype=torch.float64)
    ml_big[1:D + 1, 3:D - 1] = put(c["ml_coef"])
    oc_t = put(c["output_coef"]).t().contiguous().t()                          # column-major
    times32 = put(c["dose_time"]).to(torch.float32)                            # grid indices: exact in float32
    args = (init_v, times32, amount_wide[:, 1], eager.THETA, ml_big[1:D + 1, 3:D - 1], oc_t, c["sigma"], c["t_max"], c["step"],
            c["p_remove"], 5)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = datagen.simulate(*args)
    side.synchronize()
    for k in ("latents", "actions", "measurements", "masks", "status"):
        assert np.array_equal(got[k].cpu().numpy(), plain[k]), k
    T = plain["latents"].shape[0]
    noise = torch.randn(T, N, obs + 3, device=dev, dtype=torch.float64)
    a = datagen.simulate(*args, noise=noise[:, :, 1:obs + 1])                   # strided float64 view
    b = datagen.simulate(*args, noise=noise[:, :, 1:obs + 1].float().contiguous())
    assert torch.equal(a["measurements"], b["measurements"])
    one = datagen.simulate(put(c["init"]), put(c["dose_time"]), put(c["dose_amount"][:1]).expand(N), eager.THETA, put(c["ml_coef"]),
                           put(c["output_coef"]), c["sigma"], c["t_max"], c["step"], c["p_remove"], 5)
    c1 = dict(c)
    c1["dose_amount"] = np.full(N, c["dose_amount"][0])
    assert np.array_equal(one["latents"].cpu().numpy(), _simulate(c1)["latents"])


# ------------------------------------------------------------------------------------------------------ 7. end to end
def test_generator_end_to_end_feeds_a_training_step():
    import dataloader
    import model
    import sim_config
    from hode.batches import DeviceFolds
    dev = torch.device(DEV)
    c = sim_config.dim8_config
    np.random.seed(666)
    torch.manual_seed(666)
    dg = dataloader.DataGeneratorRoche(130, c.obs_dim, c.t_max, c.step_size, sim_config.RochConfig(kel=1), c.output_sigma,
                                       c.dose_max, c.latent_dim, c.sparsity, p_remove=c.p_remove,
                                       output_sparsity=c.output_sparsity, device=dev, val_size=20, test_size=30)
    dg.generate_data()
    dg.split_sample()
    T = dg.time_dim
    assert dg.measurements.shape == (T, 130, c.obs_dim) and dg.latents.shape == (T, 130, 8) and dg.actions.shape == (T, 130, 1)
    assert [dg.data_train["masks"].shape[1], dg.data_val["masks"].shape[1], dg.data_test["masks"].shape[1]] == [80, 20, 30]
    assert (dg.status == 0).all() and torch.isfinite(dg.measurements[dg.masks > 0]).all()
    assert 0.3 < dg.masks.mean().item() < 0.7
    folds = DeviceFolds.from_generator(dg, dev)
    batch = folds.get_mini_batch("train", 16)
    assert batch["measurements"].shape == (T, 16, c.obs_dim)
    enc = model.EncoderLSTM(c.obs_dim + 1, int(c.obs_dim * 2.0), 8, device=dev)
    dec = model.RocheExpertDecoder(c.obs_dim, 8, 1, c.t_max, c.step_size, device=dev)
    vi = model.VariationalInference(enc, dec, elbo=False)
    loss = vi.loss(batch)
    loss.backward()
    assert torch.isfinite(loss).item()
    grads = [p.grad for p in list(enc.parameters()) + list(dec.parameters()) if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
