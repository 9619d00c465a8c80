"""Yardstick of the incremental PCA: a numpy restatement of the algorithm that the reference's trainer runs per articulator
(train_articulatory_PCA.py:91-108, sklearn's IncrementalPCA.partial_fit once per loader batch), in the SVD form, written from its
description:

  statistics   Chan's update of the column mean and variance, n' = n + m
  first batch  M = X - mean'
  later        M = [S V (k rows); X - batch_mean (m rows); sqrt(n m / n') (mean - batch_mean) (1 row)]
  SVD of M, descending; each right vector signed so that its largest-magnitude entry is positive
  components_ = Vt[:k], singular_values_ = S[:k], explained_variance_ = S[:k]^2 / (n' - 1),
  explained_variance_ratio_ = S[:k]^2 / sum(var' n'), noise_variance_ = mean of the discarded S^2 / (n' - 1) (0 if k is m or F)

``dtype=np.float64`` is the yardstick proper (the fp32 inputs promoted); ``dtype=np.float32`` centres, stacks and decomposes in
float32 while the mean and variance stay float64: the arithmetic of a float32 SVD on the same chain, whose distance from the
float64 run is the scale of the parity bounds.
"""
import numpy as np


class IncrementalPCAYardstick:
    def __init__(self, n_components, dtype=np.float64):
        self.n_components, self.dtype = int(n_components), dtype
        self.n_samples_seen_ = 0
        self.mean_ = self.var_ = None
        self.components_ = self.singular_values_ = None
        self.spectrum_ = None   # every singular value of the last step, squared and divided by n' - 1

    def partial_fit(self, X):
        X = np.asarray(X)
        m, F = X.shape
        k = self.n_components
        if k > F:
            raise ValueError(f"n_components={k} must be <= n_features={F}")
        if self.n_samples_seen_ == 0 and k > m:
            raise ValueError(f"n_components={k} must be <= the first batch's {m} samples")
        X64 = X.astype(np.float64)
        batch_mean = X64.mean(axis=0)
        batch_ss = ((X64 - batch_mean) ** 2).sum(axis=0)
        n = self.n_samples_seen_
        nn = n + m
        dt = self.dtype
        if n == 0:
            mean, var = batch_mean, batch_ss / nn
            M = (X.astype(dt) - mean.astype(dt)).astype(dt)
        else:
            delta = batch_mean - self.mean_
            mean = self.mean_ + delta * (m / nn)
            var = (self.var_ * n + batch_ss + delta * delta * (n * m / nn)) / nn
            corr = np.sqrt(n * m / nn) * (self.mean_ - batch_mean)
            M = np.vstack([(self.singular_values_.reshape(-1, 1) * self.components_).astype(dt),
                           (X.astype(dt) - batch_mean.astype(dt)).astype(dt), corr.astype(dt)[None]]).astype(dt)
        _, S, Vt = np.linalg.svd(M, full_matrices=False)
        idx = np.argmax(np.abs(Vt), axis=1)
        signs = np.sign(Vt[np.arange(Vt.shape[0]), idx])
        signs[signs == 0] = 1
        Vt = Vt * signs[:, None].astype(dt)
        ev = S.astype(np.float64) ** 2 / (nn - 1)
        self.n_samples_seen_, self.mean_, self.var_ = nn, mean, var
        self.components_, self.singular_values_ = Vt[:k], S[:k]
        self.explained_variance_ = (S[:k] ** 2 / dt(nn - 1)).astype(dt)
        self.explained_variance_ratio_ = (S[:k].astype(np.float64) ** 2 / np.sum(var * nn)).astype(dt)
        self.noise_variance_ = float(ev[k:].mean()) if k not in (m, F) and len(ev) > k else 0.0
        self.spectrum_ = ev
        return self

    def fit(self, X, batch_size, order=None):
        X = np.asarray(X)
        if order is not None:
            X = X[np.asarray(order)]
        for i in range(0, len(X), batch_size):
            self.partial_fit(X[i:i + batch_size])
        return self

    def transform(self, X):
        return (np.asarray(X, dtype=np.float64) - self.mean_) @ self.components_.astype(np.float64).T

    def inverse_transform(self, Z):
        return np.asarray(Z, dtype=np.float64) @ self.components_.astype(np.float64) + self.mean_

    def eigenvalue_gap(self):
        """smallest (lambda_i - lambda_{i+1}) / lambda_1 over i <= k of the last step: the conditioning of the k-th direction"""
        ev = self.spectrum_
        k = min(self.n_components, len(ev) - 1)
        return float(np.min(ev[:k] - ev[1:k + 1]) / ev[0])

