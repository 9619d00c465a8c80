"""Incremental PCA of the articulator contours, fitted on the device (reference train_articulatory_PCA.py, which runs one
``sklearn.decomposition.IncrementalPCA`` per articulator and calls ``partial_fit`` once per loader batch).

``IncrementalPCA`` carries sklearn's attribute names for one matrix; ``MultiArticulatorPCA`` is what the trainer uses: every
articulator of a (rows, A, F) tensor in one ``as_pca_fit`` call (artspeech_amd/csrc/pca.hip), whole chains of batches included.
The chain state is kept in float64 on the device, so ``fit`` and the loop of ``partial_fit`` calls over the same batches give the
same bits.  There is no CPU path.
"""
from collections import OrderedDict

import torch

from ... import _lib
from .models.autoencoder import MultiDecoder, MultiEncoder, _resolve


class MultiArticulatorPCA:
    """One incremental PCA per articulator; channels of the inputs in sorted-articulator order.

    indices_dict: {articulator: k or list of latent indices} (the trainers' ``model_params["indices_dict"]``);
    batch_size:   rows per chain step of ``fit``.
    After a fit, ``components_[a]`` (k, F), ``singular_values_[a]``, ``explained_variance_[a]``, ``explained_variance_ratio_[a]``
    (k,) float32, ``noise_variance_[a]`` () float32, ``mean_[a]`` / ``var_[a]`` (F,) float64 are CUDA tensors per articulator and
    ``n_samples_seen_`` an int.
    """

    def __init__(self, indices_dict, batch_size):
        self.indices_dict, self.latent_size, self.sorted_articulators = _resolve(indices_dict)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size={batch_size} must be positive")
        self.n_components = [len(self.indices_dict[a]) for a in self.sorted_articulators]
        self.k_max = max(self.n_components)
        self.n_samples_seen_ = 0
        self.in_features = None
        self._projections = None

    # ------------------------------------------------------------------------------------------------ fitting
    def _check(self, x, first_rows):
        if x.dim() != 3 or x.shape[1] != len(self.sorted_articulators):
            raise ValueError(f"inputs {tuple(x.shape)}: expected (rows, {len(self.sorted_articulators)}, features)")
        F = x.shape[2]
        if self.in_features is not None and F != self.in_features:
            raise ValueError(f"inputs have {F} features, the fit so far {self.in_features}")
        if self.k_max > F:
            raise ValueError(f"n_components={self.k_max} must be less or equal to the number of features {F}")
        if self.n_samples_seen_ == 0 and self.k_max > first_rows:
            raise ValueError(f"n_components={self.k_max} must be less or equal to the first batch's number of samples {first_rows}")
        if x.shape[0] < 1:
            raise ValueError("inputs hold no rows")
        _lib.require_gpu(x, "inputs")
        if not _lib.call("as_pca_supported", F, self.k_max):
            raise NotImplementedError(f"as_pca_fit: features={F}, n_components={self.k_max} outside the kernel's limits "
                                      "(features <= 256, n_components <= min(features, 64))")

    def _allocate(self, F, dev):
        A, K = len(self.sorted_articulators), self.k_max
        self.in_features = F
        self._k = torch.tensor(self.n_components, dtype=torch.int32, device=dev)
        self._state = torch.zeros(A, 2 * F + K + K * F, dtype=torch.float64, device=dev)
        self._components = torch.zeros(A, K, F, dtype=torch.float32, device=dev)
        self._scalars = torch.zeros(3, A, K, dtype=torch.float32, device=dev)   # singular values, variance, variance ratio
        self._noise = torch.zeros(A, dtype=torch.float32, device=dev)

    def _run(self, x, rows, batch, order):
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(2) != 1:
            x = x.contiguous()
        if self.in_features is None:
            self._allocate(x.shape[2], x.device)
        d = _lib.Pca()
        d.groups, d.features, d.k_max, d.batch = len(self.sorted_articulators), self.in_features, self.k_max, batch
        d.k, d.x, d.rows, d.x_r, d.x_g = self._k.data_ptr(), x.data_ptr(), rows, x.stride(0), x.stride(1)
        d.order = 0 if order is None else order.data_ptr()
        d.n_seen, d.state = self.n_samples_seen_, self._state.data_ptr()
        d.components, d.noise_variance = self._components.data_ptr(), self._noise.data_ptr()
        d.singular_values, d.explained_variance, d.explained_variance_ratio = (self._scalars[i].data_ptr() for i in range(3))
        n = _lib.call("as_pca_workspace_floats", d)
        if n < 0:
            raise RuntimeError("as_pca_workspace_floats: bad descriptor")
        ws = torch.empty(max(n, 2), dtype=torch.float32, device=x.device)
        d.ws, d.ws_floats = ws.data_ptr(), n
        _lib.call("as_pca_fit", d)
        self.n_samples_seen_ += rows
        self._projections = None
        return self

    def partial_fit(self, inputs):
        """One chain step on inputs (m, A, F): the reference's ``transformers[a].partial_fit(inputs[:, i, :])`` for every a."""
        self._check(inputs, inputs.shape[0] if inputs.dim() == 3 else 0)
        return self._run(inputs, inputs.shape[0], inputs.shape[0], None)

    def fit(self, frames, order=None):
        """A fresh fit on frames (N, A, F) resident on the device, in batches of ``batch_size`` rows (the last may be short, as a
        DataLoader leaves it); ``order`` (n,) integer: the rows to visit, in that order (the shuffled loader order)."""
        self.n_samples_seen_, self.in_features, self._projections = 0, None, None
        rows = frames.shape[0] if order is None else int(order.numel())
        self._check(frames, min(self.batch_size, rows))
        if order is not None:
            order = order.to(device=frames.device)
            if order.numel() and (int(order.min()) < 0 or int(order.max()) >= frames.shape[0]):
                raise ValueError(f"order holds a row outside 0..{frames.shape[0] - 1}")
            order = order.to(torch.int32).contiguous()
        return self._run(frames, rows, self.batch_size, order)

    # ------------------------------------------------------------------------------------------------ fitted attributes
    def _per_articulator(self, fn):
        self._require_fit()
        return OrderedDict((a, fn(self.sorted_articulators.index(a), len(self.indices_dict[a]))) for a in self.indices_dict)

    def _require_fit(self):
        if self.n_samples_seen_ == 0:
            raise RuntimeError("this PCA has not been fitted")

    components_ = property(lambda self: self._per_articulator(lambda i, k: self._components[i, :k]))
    singular_values_ = property(lambda self: self._per_articulator(lambda i, k: self._scalars[0, i, :k]))
    explained_variance_ = property(lambda self: self._per_articulator(lambda i, k: self._scalars[1, i, :k]))
    explained_variance_ratio_ = property(lambda self: self._per_articulator(lambda i, k: self._scalars[2, i, :k]))
    noise_variance_ = property(lambda self: self._per_articulator(lambda i, k: self._noise[i]))
    mean_ = property(lambda self: self._per_articulator(lambda i, k: self._state[i, :self.in_features]))
    var_ = property(lambda self: self._per_articulator(lambda i, k: self._state[i, self.in_features:2 * self.in_features]))

    def state_dicts(self):
        """(encoder_dict, decoder_dict) of the reference's ``make_multiarticulator_autoencoder`` (train_articulatory_PCA.py:38-51):
        they load into ``MultiEncoder(..., encoder_cls="PCA")`` / ``MultiDecoder(..., decoder_cls="PCA")``.  Like the reference's,
        they do not hold the mean: a ``PCAEncoder`` loaded from them projects without centring."""
        encoder_dict, decoder_dict = OrderedDict(), OrderedDict()
        values, vectors = self.explained_variance_, self.components_
        for a in self.indices_dict:
            encoder_dict[f"encoders.{a}.eigenvalues"] = values[a].clone()
            encoder_dict[f"encoders.{a}.eigenvectors"] = vectors[a].clone()
            decoder_dict[f"decoders.{a}.eigenvalues"] = values[a].clone().unsqueeze(dim=-1)
            decoder_dict[f"decoders.{a}.eigenvectors"] = vectors[a].clone()
        return encoder_dict, decoder_dict

    # ------------------------------------------------------------------------------------------------ projections
    def _fused(self):
        """The fused projection kernel's containers with the fitted components and the mean folded into the bias."""
        if self._projections is None:
            self._require_fit()
            dev = self._components.device
            encoder_dict, decoder_dict = self.state_dicts()
            enc = MultiEncoder(self.indices_dict, self.in_features, 0, encoder_cls="PCA")
            dec = MultiDecoder(self.indices_dict, self.in_features, 0, decoder_cls="PCA")
            enc.load_state_dict(encoder_dict, strict=True)
            dec.load_state_dict(decoder_dict, strict=True)
            enc.to(dev).requires_grad_(False)
            dec.to(dev).requires_grad_(False)
            for a, mean in self.mean_.items():
                enc.encoders[a].mean = dec.decoders[a].mean = mean.float()
            self._projections = (enc, dec)
        return self._projections

    def transform(self, inputs):
        """inputs (m, A, F) -> latent (m, latent_size): (x - mean_) components_^T of every articulator at its latent indices."""
        _lib.require_gpu(inputs, "inputs")
        with torch.no_grad():
            return self._fused()[0](inputs)

    def inverse_transform(self, latent):
        """latent (m, latent_size) -> (m, A, F): z components_ + mean_ per articulator."""
        _lib.require_gpu(latent, "latent")
        with torch.no_grad():
            return self._fused()[1](latent)


class IncrementalPCA:
    """sklearn.decomposition.IncrementalPCA's interface on CUDA tensors: ``partial_fit`` / ``fit`` / ``transform`` /
    ``inverse_transform`` and the fitted ``components_``, ``singular_values_``, ``explained_variance_``,
    ``explained_variance_ratio_``, ``noise_variance_`` (float32), ``mean_``, ``var_`` (float64), ``n_samples_seen_``."""

    def __init__(self, n_components, batch_size=None):
        if int(n_components) < 1:
            raise ValueError(f"n_components={n_components} must be positive")
        self.n_components, self.batch_size = int(n_components), batch_size
        self._multi = MultiArticulatorPCA({"x": list(range(self.n_components))}, batch_size or 1)

    @staticmethod
    def _matrix(X):
        if X.dim() != 2:
            raise ValueError(f"X {tuple(X.shape)}: expected (samples, features)")
        return X.unsqueeze(1)

    def partial_fit(self, X):
        self._multi.partial_fit(self._matrix(X))
        return self

    def fit(self, X):
        X = self._matrix(X)
        self._multi.batch_size = int(self.batch_size or 5 * X.shape[2])   # sklearn's default batch
        self._multi.fit(X)
        return self

    def transform(self, X):
        return self._multi.transform(self._matrix(X))

    def inverse_transform(self, Z):
        return self._multi.inverse_transform(Z)[:, 0]

    n_samples_seen_ = property(lambda self: self._multi.n_samples_seen_)


for _name in ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_", "mean_", "var_"):
    setattr(IncrementalPCA, _name, property(lambda self, _n=_name: getattr(self._multi, _n)["x"]))
