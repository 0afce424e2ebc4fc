"""CPU checks of the synthetic data generator (no GPU): the mirror's seeded draws against the reference's recorded run
(G14), the float64 yardstick against the reference's latents, libhode_datagen.so's C ABI, build-table row and refusals, and the
fold / batch / pickle surface of dataloader.DataGeneratorRoche on hand-filled tensors."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import abi_checks
import build_hip
import datagen_cases as cases
import datagen_eager as eager
import dataloader
import sim_config

ROOT = build_hip.ROOT
LIB = "libhode_datagen.so"
FUNCTIONS = {"hode_datagen_version", "hode_datagen_last_error_string", "hode_datagen_workspace_bytes", "hode_datagen_generate"}


def _generator(name, n=None, **kw):
    g, c = cases.g14(), cases.case(name)
    cfg = g[c["prefix"] + "config"]
    N, val, test, seed = (int(v) for v in g["meta"][:4])
    np.random.seed(seed)
    return dataloader.DataGeneratorRoche(n or N, int(cfg[0]), int(cfg[2]), cfg[3], sim_config.RochConfig(), cfg[6], cfg[7],
                                         int(cfg[1]), cfg[4], cfg[5], val, test, cfg[8], device=torch.device("cpu"), **kw)


# ------------------------------------------------------------------------------------------------ 1. seed compatibility
@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_seeded_draws_are_the_references(name):
    g, p = cases.g14(), cases.case(name)["prefix"]
    dg = _generator(name)
    init = dg.get_initial_conditions()
    dose_time, dose_amount = dg.get_action()
    assert np.array_equal(dg.output_coef, g[p + "output_coef"]) and np.array_equal(dg.ml_coef, g[p + "ml_coef"])
    assert np.array_equal(init, g[p + "init"]) and init.dtype == np.float64
    assert np.array_equal(dose_time, g[p + "dose_time"]) and np.array_equal(dose_amount, g[p + "dose_amount"])
    assert dg.time_dim == g[p + "latents"].shape[0] and dg.ml_dim == dg.latent_dim - 4


def test_sim_config_cases_are_the_recorded_ones():
    g = cases.g14()
    for i, c in enumerate((sim_config.dim8_config, sim_config.dim12_config,
                           sim_config.DataConfig(latent_dim=4, dose_max=10, output_sigma=0.2))):
        want = [c.obs_dim, c.latent_dim, c.t_max, c.step_size, c.sparsity, c.output_sparsity, c.output_sigma, c.dose_max, c.p_remove]
        assert np.array_equal(g["c%d_config" % i], np.array(want, dtype=np.float64))


# ----------------------------------------------------------------------------------- 2. yardstick against the reference
@pytest.mark.parametrize("name", cases.FIXTURE_CASES)
def test_yardstick_is_within_3e_5_of_the_references_latents(name):
    g, c = cases.g14(), cases.case(name)
    tight, E = cases.yardstick(name)
    err = np.abs(tight - g[c["prefix"] + "latents"].astype(np.float64)).max()
    print(name, "yardstick vs reference %.3e, RK45 at the kernel's tolerances vs yardstick %.3e" % (err, E))
    assert err <= 3e-5
    assert E <= 1e-6
    assert np.array_equal(eager.actions(c["dose_time"], c["dose_amount"], c["t_max"], c["step"]).astype(np.float32),
                          g[c["prefix"] + "actions"])


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32-10."""
    hexes = lambda w: ["%08x" % int(x) for x in w]
    assert hexes(eager.philox(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hexes(eager.philox(f, f, f, f, f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(eager.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


# ------------------------------------------------------------------------------------------------------ 3. ABI, layout
@pytest.fixture(scope="module")
def lib():
    from hode import _datagen_lib as GL
    return abi_checks.built(GL.LIBRARY)


def test_header_functions_are_exported_and_bound(lib):
    from hode import _datagen_lib as GL
    src = abi_checks.header_text("hode_datagen.h")
    declared = abi_checks.declared_functions("hode_datagen.h", "hode_datagen_")
    assert declared == {name for name, _, _ in GL.EXPORTS} == FUNCTIONS
    for name in declared:
        assert getattr(lib, name) is not None
    define = lambda n: int(re.search(r"#define HODE_DATAGEN_%s (-?\d+)" % n, src).group(1))
    assert lib.hode_datagen_version() == GL.HODE_DATAGEN_ABI_VERSION == define("ABI_VERSION")
    assert (define("MAX_OBS"), define("MAX_DOSES"), define("N_THETA")) == (GL.MAX_OBS, GL.MAX_DOSES, GL.N_THETA)
    assert (define("E_NULL"), define("E_SIZE"), define("E_UNSUPPORTED")) == (GL.E_NULL, GL.E_SIZE, GL.E_UNSUPPORTED)
    assert GL.DIMS == build_hip.RK_DIMS


def test_struct_size_matches_the_c_header(tmp_path):
    from hode import _datagen_lib as GL
    abi_checks.assert_c_layout("hode_datagen.h", "hode_datagen_desc", GL.DatagenDesc, tmp_path)


def test_the_row_of_the_build_table():
    row = build_hip.LIBRARIES[LIB]
    assert row.header == "include/hode_datagen.h" and row.src_dir == build_hip.PKG + "/csrc/datagen"
    assert [(n, os.path.relpath(s, ROOT).replace(os.sep, "/"), e) for n, s, e in row.units()] == \
        [("hode_datagen", row.src_dir + "/hode_datagen.hip", [])]
    assert {"include/hode_datagen.h", build_hip.PKG + "/csrc/hode_side_error.hpp",
            build_hip.PKG + "/csrc/datagen/hode_datagen.hip"} <= set(build_hip.digest_files(LIB))


# ------------------------------------------------------------------------------------------ 4. refusals without a launch
def _desc(**over):
    from hode import _datagen_lib as GL
    d = GL.new_desc()
    d.n_patients, d.n_times, d.latent_dim, d.obs_dim, d.n_dose, d.max_steps = 65, 15, 8, 40, 1, 100
    d.step, d.rtol, d.atol, d.sigma, d.p_remove = 1.0, 1e-8, 1e-10, 0.2, 0.5
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_argument_errors_do_not_launch(lib):
    from hode import _datagen_lib as GL
    err = lib.hode_datagen_last_error_string
    assert lib.hode_datagen_generate(None, None) == GL.E_NULL and b"NULL" in err()
    assert lib.hode_datagen_generate(_desc(struct_size=8), None) == GL.E_SIZE and b"struct_size" in err()
    assert lib.hode_datagen_generate(_desc(latent_dim=5), None) == GL.E_UNSUPPORTED and b"latent_dim 5" in err()
    assert lib.hode_datagen_generate(_desc(flags=1), None) == GL.E_UNSUPPORTED and b"flags" in err()
    for field, bad, word in (("obs_dim", 129, b"obs_dim 129"), ("obs_dim", 0, b"obs_dim 0"), ("n_dose", 9, b"n_dose 9"),
                             ("n_dose", 0, b"n_dose 0"), ("n_times", 1, b"n_times 1"), ("n_patients", 0, b"n_patients"),
                             ("max_steps", 0, b"max_steps"), ("step", 0.0, b"step"), ("rtol", -1.0, b"rtol")):
        assert lib.hode_datagen_generate(_desc(**{field: bad}), None) == GL.E_SIZE, field
        assert word in err(), field
    assert lib.hode_datagen_generate(_desc(n_patients=2 ** 30, n_times=4), None) == GL.E_SIZE and b"2^31" in err()
    assert lib.hode_datagen_generate(_desc(), None) == GL.E_NULL        # a shape of the domain, pointers missing
    need = lib.hode_datagen_workspace_bytes(65, 40)
    assert need == 2 * 40 * (1 + 2) * 8
    assert lib.hode_datagen_workspace_bytes(0, 40) == 0 and lib.hode_datagen_workspace_bytes(65, 129) == 0
    ptrs = {f: 64 for f in ("init", "dose_times", "dose_amount", "ml_coef", "output_coef", "latents", "actions", "measurements",
                            "masks", "status", "workspace")}
    assert lib.hode_datagen_generate(_desc(workspace_bytes=need - 8, **ptrs), None) == GL.E_SIZE and b"workspace_bytes" in err()
    ptrs["ml_coef"] = 0
    assert lib.hode_datagen_generate(_desc(workspace_bytes=need, **ptrs), None) == GL.E_NULL and b"ml_coef" in err()


def test_the_binding_refuses_what_is_outside_the_domain():
    from hode import HodeConfigError, datagen
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    call = lambda N=3, D=8, K=1, obs=5, t_max=14: datagen.simulate(z(N, D), z(N, K), z(N), eager.THETA, z(D, max(D - 4, 0)),
                                                                    z(obs, D + 1), 0.2, t_max, 1.0, 0.5, 1)
    with pytest.raises(HodeConfigError, match="HIP device"):
        call()
    for kw, word in ((dict(D=5), "latent_dim 5"), (dict(obs=129), "obs 129"), (dict(K=9), "9 doses"), (dict(t_max=0), "two grid points")):
        with pytest.raises(HodeConfigError, match=word):
            call(**kw)
    with pytest.raises(HodeConfigError, match="ml_coef shape"):
        datagen.simulate(z(3, 8), z(3, 1), z(3), eager.THETA, z(8, 3), z(5, 9), 0.2, 14, 1.0, 0.5, 1)
    with pytest.raises(HodeConfigError, match="13"):
        datagen.simulate(z(3, 8), z(3, 1), z(3), eager.THETA[:12], z(8, 4), z(5, 9), 0.2, 14, 1.0, 0.5, 1)


# ---------------------------------------------------------------------------------------------- 5. surface on CPU tensors
def _filled(n=23, val=5, test=7):
    dg = _generator("g14_dim8", n=n)
    dg.val_size, dg.test_size, dg.train_size = val, test, n - val - test
    T = dg.time_dim
    gen = torch.Generator().manual_seed(4)
    dg.measurements = torch.randn(T, n, dg.obs_dim, generator=gen)
    dg.actions = torch.rand(T, n, 1, generator=gen)
    dg.latents = torch.randn(T, n, dg.latent_dim, generator=gen)
    dg.masks = (torch.rand(T, n, dg.obs_dim, generator=gen) > 0.5).float()
    return dg


def test_folds_and_batches_are_the_references_slicing(capsys):
    dg = _filled()
    dg.split_sample()
    full = {k: getattr(dg, k) for k in dataloader.FIELDS}
    tr, va = dg.train_size, dg.val_size
    for k, v in full.items():                                  # dataloader.py:272-295
        assert torch.equal(dg.data_train[k], v[:, :tr, :]) and torch.equal(dg.data_val[k], v[:, tr:tr + va, :])
        assert torch.equal(dg.data_test[k], v[:, tr + va:, :])
    for fold, data in (("train", dg.data_train), ("val", dg.data_val), ("test", dg.data_test)):
        for chunk in (0, 1):                                   # :322-341
            b = dg.get_split(fold, 3, chunk)
            assert set(b) == set(dataloader.FIELDS)
            for k in b:
                assert torch.equal(b[k], data[k][:, chunk * 3:(chunk + 1) * 3, :])
        np.random.seed(12)                                     # :297-320
        b = dg.get_mini_batch(fold, 4)
        np.random.seed(12)
        idx = torch.as_tensor(np.random.choice(data["measurements"].shape[1], 4, replace=False))
        for k in b:
            assert torch.equal(b[k], data[k][:, idx, :])
    with pytest.raises(AssertionError):
        dg.get_split("all", 3)
    dg.set_train_size(20)                                      # :82-89: n_sample counts all three folds
    assert (dg.train_size, dg.n_sample) == (8, 20) and "train_size 8" in capsys.readouterr().out
    dg.set_val_size(2)                                         # :91-94
    for k, v in full.items():
        assert torch.equal(dg.data_train[k], v[:, :8, :]) and torch.equal(dg.data_val[k], v[:, tr:tr + 2, :])
    dg.set_device(torch.device("cpu"))
    assert dg.data_test["masks"].device.type == "cpu"


def test_generate_data_on_a_cpu_device_is_refused():
    from hode import HodeConfigError
    dg = _generator("g14_dim8")
    with pytest.raises(HodeConfigError, match="HIP device"):
        dg.generate_data()
    assert dg.dose_time.shape == (48, 1) and dg.measurements is None
    with pytest.raises(ValueError):
        _generator("g14_dim8", draws="sobol")


def test_pickle_round_trip_keeps_every_attribute():
    dg = _filled()
    dg.dose_time, dg.dose_amount = dg.get_action()
    dg.split_sample()
    back = pickle.loads(pickle.dumps(dg))
    assert type(back) is dataloader.DataGeneratorRoche and set(back.__dict__) == set(dg.__dict__) - {"_gen"}
    for k, v in dg.__dict__.items():
        w = back.__dict__[k]
        if torch.is_tensor(v):
            assert torch.equal(v, w) and w.device.type == "cpu", k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, w), k
        elif isinstance(v, dict):
            assert all(torch.equal(v[f], w[f]) for f in v), k
        else:
            assert v == w, k
    assert torch.equal(back.get_split("val", 2, 1)["latents"], dg.get_split("val", 2, 1)["latents"])
