"""``DataGeneratorRoche`` with the reference's call surface (``dataloader.py:10-341``), on the GPU generator.

The constructor and the two draw methods make the reference's numpy calls in the reference's order, so a run under
``np.random.seed(s)`` has the reference's ``output_coef``, ``ml_coef``, initial states and dose schedule
(``draws="numpy"``, the default).  ``draws="device"`` draws the initial states and the schedule with a seeded torch
generator on the device instead: the reference's one ``np.random.choice`` per patient does not scale to millions.
``generate_data()`` is one ``hode.datagen.simulate`` call (per-patient adaptive float64 Dormand-Prince in place of one
LSODA loop per patient), seeded from the numpy stream at the point where the reference starts drawing its output noise.
The noise and the masks themselves come from the kernel's counter-based generator, not from numpy / torch streams.

``DataGeneratorReal`` (``dataloader.py:344-491``) is the loader ``experiments/run_real.py`` starts with: four pickles in,
the same folds, batches and numpy draws as the reference's class out."""
import os
import pickle

import numpy as np
import torch

from global_config import DTYPE, get_device
from hode import datagen

FIELDS = ("measurements", "actions", "latents", "masks")


class DataGeneratorRoche:
    FIELDS = FIELDS   # what a fold and a batch carry; DataGeneratorReal adds "statics"

    def __init__(self, n_sample, obs_dim, t_max, step_size, roche_config, output_sigma, dose_max=0, latent_dim=4, sparsity=0.5,
                 output_sparsity=0.0, val_size=100, test_size=200, p_remove=0, device=None, dtype=DTYPE, draws="numpy",
                 rtol=1e-8, atol=1e-10):
        if draws not in ("numpy", "device"):
            raise ValueError("draws must be 'numpy' (the reference's draws) or 'device'")
        self.device = get_device() if device is None else device
        self.dtype = dtype
        self.draws, self.rtol, self.atol = draws, rtol, atol

        self.n_sample = n_sample
        self.obs_dim = obs_dim
        self.latent_dim = int(latent_dim)
        self.expert_dim = int(4)
        self.ml_dim = self.latent_dim - self.expert_dim
        self.sparsity = sparsity
        self.action_dim = int(1)
        self.expanded = self.ml_dim > 0
        self.t_max = t_max
        self.step_size = step_size
        self.time_dim = int(t_max / step_size + 1)
        self.roche_config = roche_config
        self.dose_max = dose_max
        self.p_remove = p_remove
        self.output_sparsity = output_sparsity

        shape = (obs_dim, self.latent_dim + self.action_dim)
        self.output_coef = np.random.randn(*shape) * np.random.binomial(1, 1 - self.output_sparsity, shape)
        self.output_sigma = output_sigma
        shape = (self.latent_dim, self.ml_dim)
        self.ml_coef = np.random.randn(*shape) * np.random.binomial(1, 1 - self.sparsity, shape) / self.latent_dim

        self.val_size = int(val_size)
        self.test_size = int(test_size)
        self.train_size = int(n_sample - val_size - test_size)

        self.measurements = self.actions = self.latents = self.masks = None
        self.dose_time = self.dose_amount = self.status = None
        self.data_train, self.data_val, self.data_test = None, None, None

    # ---- draws -----------------------------------------------------------------------------------------------------
    def _device_generator(self):
        if getattr(self, "_gen", None) is None:
            self._gen = torch.Generator(device=self.device).manual_seed(int(np.random.randint(0, 2 ** 31 - 1)))
        return self._gen

    def get_initial_conditions(self):
        """(N, D) initial states, Exponential(scale 0.01)."""
        if self.draws == "device":
            init = torch.empty(self.n_sample, self.latent_dim, device=self.device, dtype=torch.float64)
            return init.exponential_(100.0, generator=self._device_generator())
        return np.random.exponential(scale=0.01, size=(self.n_sample, self.latent_dim))

    def get_action(self):
        """(dose_time (N, 1) from 0 .. t_max - 1, dose_amount (N,) ~ U(0, dose_max))."""
        if self.draws == "device":
            gen = self._device_generator()
            dose_time = torch.randint(0, int(self.t_max), (self.n_sample, 1), device=self.device, generator=gen)
            dose_amount = torch.rand(self.n_sample, device=self.device, dtype=torch.float64, generator=gen) * self.dose_max
            return dose_time, dose_amount
        dose_list = []
        for i in range(self.n_sample):
            dose_list.append(np.random.choice(self.t_max, size=1, replace=False))
        dose_time = np.sort(np.stack(dose_list, axis=0))
        dose_amount = np.random.rand(self.n_sample) * self.dose_max
        return dose_time, dose_amount

    def _make_tensor(self, x):
        """A numpy array or a tensor as a tensor of ``dtype`` on ``device`` (dataloader.py:224-228)."""
        if type(x) == np.ndarray:
            return torch.tensor(x, dtype=self.dtype, device=self.device)
        return x.to(dtype=self.dtype, device=self.device)

    # ---- generation ------------------------------------------------------------------------------------------------
    def generate_data(self):
        init = self.get_initial_conditions()
        dose_time, dose_amount = self.get_action()
        self.dose_time, self.dose_amount = dose_time, dose_amount
        seed = int(np.random.randint(0, 2 ** 31 - 1))     # where the reference starts drawing its output noise
        dev = torch.device(self.device)
        put = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float64)
        out = datagen.simulate(put(init), put(dose_time), put(dose_amount), self.roche_config, put(self.ml_coef),
                               put(self.output_coef[:, :self.latent_dim + 1]), self.output_sigma, self.t_max, self.step_size,
                               self.p_remove, seed, rtol=self.rtol, atol=self.atol)
        self.measurements = out["measurements"].to(self.dtype)
        self.actions = out["actions"].to(self.dtype)
        self.latents = out["latents"].to(self.dtype)
        self.masks = out["masks"].to(self.dtype)
        self.status = out["status"]
        assert self.measurements.shape == (self.time_dim, self.n_sample, self.obs_dim)
        assert self.actions.shape == (self.time_dim, self.n_sample, self.action_dim)
        assert self.latents.shape == (self.time_dim, self.n_sample, self.latent_dim)

    # ---- folds and batches (dataloader.py:71-94, 272-341) -------------------------------------------------------------
    def set_device(self, device):
        self.device = device
        for k in self.FIELDS:
            setattr(self, k, getattr(self, k).to(device))
        for a in (self.data_train, self.data_val, self.data_test):
            for k in self.FIELDS:
                a[k] = a[k].to(device)

    def set_train_size(self, n_sample):
        train_sample_size = n_sample - self.val_size - self.test_size
        self.train_size = train_sample_size
        self.n_sample = n_sample
        print("train_size", self.train_size)
        print("n_sample", self.n_sample)
        for k in self.FIELDS:
            self.data_train[k] = self.data_train[k][:, :train_sample_size, :]

    def set_val_size(self, n_val):
        self.val_size = n_val
        for k in self.FIELDS:
            self.data_val[k] = self.data_val[k][:, :n_val, :]

    def split_sample(self):
        tr, va = self.train_size, self.val_size
        cut = lambda lo, hi: {k: getattr(self, k)[:, lo:hi, :] for k in self.FIELDS}
        self.data_train, self.data_val, self.data_test = cut(0, tr), cut(tr, tr + va), cut(tr + va, None)

    def _fold(self, fold):
        assert fold in ("train", "val", "test")
        return {"train": self.data_train, "val": self.data_val, "test": self.data_test}[fold]

    def _get_index_random(self, N, k):
        return torch.as_tensor(np.random.choice(N, k, replace=False)).to(device=self.device, dtype=torch.int64)

    def get_mini_batch(self, fold, batch_size):
        data = self._fold(fold)
        indices = self._get_index_random(data["measurements"].shape[1], batch_size)
        return {k: data[k][:, indices, :] for k in self.FIELDS}

    def get_split(self, fold, batch_size, chunk=0):
        data = self._fold(fold)
        lo, hi = chunk * batch_size, (chunk + 1) * batch_size
        return {k: data[k][:, lo:hi, :] for k in self.FIELDS}

    # ---- pickling: tensors travel on the CPU, so that a file written on a GPU loads anywhere ---------------------------
    def __getstate__(self):
        cpu = lambda v: v.cpu() if torch.is_tensor(v) else v
        state = {k: cpu(v) for k, v in self.__dict__.items() if k != "_gen"}
        for k in ("data_train", "data_val", "data_test"):
            if state[k] is not None:
                state[k] = {f: cpu(v) for f, v in state[k].items()}
        state["device"] = torch.device("cpu")
        return state


class DataGeneratorReal(DataGeneratorRoche):
    """The real-data loader of ``experiments/run_real.py`` (reference ``dataloader.py:344-491``): the reference's
    constructor signature and defaults, its numpy draws, its folds and its batches, with ``"statics"`` as the fifth field.

    Four files are read from ``data_path`` with ``pickle.load``: ``array_xt_mask{data_type}.pkl`` (T, N, obs),
    ``array_xt{data_type}.pkl`` (T, N, obs), ``array_at{data_type}.pkl`` (T, N, 1) and ``array_x_constant.pkl`` (N, S), each a
    numpy array or a torch tensor.  ``pickle.load`` runs whatever code a file names: this class is for files the user wrote,
    never for files from somebody else.

    As in the reference, ``DataGeneratorRoche.__init__`` runs first with the caller's arguments (so ``output_coef`` and
    ``ml_coef`` consume the numpy stream as there, and ``train_size = n_sample - val_size - test_size`` comes from the
    ARGUMENT), then ``n_sample``, ``obs_dim``, ``t_max``, ``time_dim`` and ``step_size = 1.0`` are overwritten from the
    mask's shape.  ``train_size`` is not recomputed: the test fold is every patient behind train + val, however many the
    files hold.  ``generate_data``, ``get_initial_conditions`` and ``get_action`` stay inherited and unused.

    ``set_train_size(train_sample_size)`` takes the TRAIN size here (``DataGeneratorRoche.set_train_size`` takes the
    total of the three folds), as in the reference.

    Two differences from the reference: ``set_device`` moves ``statics`` too, in the generator and in all three folds (the
    reference's inherited one leaves them behind), and a pickled generator carries ``statics`` on the CPU like every other
    tensor, so one built on a GPU unpickles anywhere."""

    FIELDS = FIELDS + ("statics",)

    def __init__(self, n_sample, obs_dim, t_max, step_size, roche_config, output_sigma, dose_max=0, latent_dim=4, sparsity=0.5,
                 output_sparsity=0.0, val_size=100, test_size=200, p_remove=0, device=None, dtype=DTYPE, data_type="",
                 data_path="../data/"):
        super().__init__(n_sample, obs_dim, t_max, step_size, roche_config, output_sigma, dose_max, latent_dim, sparsity,
                         output_sparsity, val_size, test_size, p_remove, device, dtype)
        self.masks = self._load(data_path + "array_xt_mask{}.pkl".format(data_type))
        self.n_sample = self.masks.shape[1]
        self.obs_dim = self.masks.shape[2]
        self.t_max = self.masks.shape[0]
        self.step_size = 1.0
        self.time_dim = self.masks.shape[0]

        statics = self._load(data_path + "array_x_constant.pkl")[None, :, :]
        self.statics = torch.cat([statics] * self.time_dim, dim=0)   # the same row at every time
        self.measurements = self._load(data_path + "array_xt{}.pkl".format(data_type))
        self.actions = self._load(data_path + "array_at{}.pkl".format(data_type))
        self.latents = torch.zeros_like(self.masks)[:, :, : self.latent_dim]
        self.static_dim = self.statics.shape[2]

        for name, dim in (("measurements", self.obs_dim), ("actions", self.action_dim), ("latents", self.latent_dim)):
            got, want = tuple(getattr(self, name).shape), (self.time_dim, self.n_sample, dim)
            assert got == want, "%s has shape %s, the masks ask for %s" % (name, got, want)

    def _load(self, path):
        if not os.path.isfile(path):
            raise FileNotFoundError("DataGeneratorReal: no data file %s" % path)
        with open(path, "rb") as f:
            x = pickle.load(f)
        if type(x) != np.ndarray and not torch.is_tensor(x):
            raise TypeError("DataGeneratorReal: %s holds a %s, not a numpy array or a torch tensor" % (path, type(x).__name__))
        return self._make_tensor(x)

    def set_train_size(self, train_sample_size):
        self.train_size = train_sample_size
        self.n_sample = train_sample_size + self.val_size + self.test_size
        print("train_size", self.train_size)
        print("n_sample", self.n_sample)
        for k in self.FIELDS:
            self.data_train[k] = self.data_train[k][:, :train_sample_size, :]

    def device_folds(self, device=None, index_rng="numpy"):
        """This generator's tensors as a ``hode.batches.DeviceFolds`` on ``device`` (default: the generator's), cut at
        this generator's ``train_size`` and ``val_size`` the way ``split_sample()`` cuts them: contiguous batches from one
        device gather per field, the same ``np.random.choice`` per minibatch.  The cut is made on the whole tensors, so
        take the folds before a ``set_train_size`` / ``set_val_size`` on the generator, and shorten the folds with their
        own methods."""
        from hode.batches import DeviceFolds
        folds = DeviceFolds.from_generator(self, self.device if device is None else device, index_rng=index_rng)
        if folds.train_size != self.train_size:   # DeviceFolds counts the tensors' patients, this class the argument's
            folds.train_size = self.train_size
            folds.split_sample()
        return folds
