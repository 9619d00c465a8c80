"""Exact t-SNE on the HIP library (as_tsne_sqdist / as_tsne_joint_p / as_tsne_iterate) and the feature map it is for: the
reference's ``plot_features`` (phoneme_recognition/__init__.py:332-399), which embeds up to 100 frames per token of the recogniser's
last hidden features with ``sklearn.manifold.TSNE(n_components=2).fit_transform`` (:355-356) and colours them by phonetic class.

``TSNE`` keeps scikit-learn's keyword names, schedule and stopping rule; ``sample_features_per_class`` is the selection step
(:343-353) on device tensors, ``feature_embedding`` the two together, ``plot_features`` the figure.  The features never leave the
device; what comes back to the host is one (50, 3) log per 50 iterations, which the stopping rule reads."""
import logging
import os

import numpy as np
import torch

from .. import _lib

MAX_POINTS = 16384          # as_tsne_*: two (N, N) float32 matrices
N_ITER_CHECK = 50           # scikit-learn's _N_ITER_CHECK: the stopping rule looks at every 50th iteration
EXPLORATION_MAX_ITER = 250  # its _EXPLORATION_MAX_ITER: iterations at the early exaggeration
MIN_GAIN = 0.01


def stop_rule(log, it0, best_error, best_iter, n_iter_without_progress, min_grad_norm, n_iter_check=N_ITER_CHECK):
    """scikit-learn's convergence check (_gradient_descent) over the log rows (|grad|, |gains grad|, KL) of iterations it0,
    it0 + 1, ...  Only an iteration i with (i + 1) % n_iter_check == 0 is looked at: a KL below the best so far becomes the best;
    otherwise, more than n_iter_without_progress iterations after the best one, the descent stops; then it stops when the norm of
    the gained gradient is <= min_grad_norm.  Returns (the iteration it stops at or None, best_error, best_iter).  Host only."""
    for k, row in enumerate(np.asarray(log, dtype=np.float64).reshape(-1, 3)):
        i = it0 + k
        if (i + 1) % n_iter_check != 0:
            continue
        error = float(row[2])
        if error < best_error:
            best_error, best_iter = error, i
        elif i - best_iter > n_iter_without_progress:
            return i, best_error, best_iter
        if float(row[1]) <= min_grad_norm:
            return i, best_error, best_iter
    return None, best_error, best_iter


def _workspace(N, dev):
    nbytes = int(_lib.call("as_tsne_workspace_bytes", N))
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


def squared_distances(X):
    """(N, N) float32 squared euclidean distances of the rows of X (N, D) float32 on the device (any row stride, unit column stride),
    by direct differences: exactly symmetric, exactly zero diagonal (as_tsne_sqdist)."""
    _lib.require_gpu(X, "X")
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError("squared_distances: X must be an (N, D) float32 tensor")
    if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        X = X.contiguous()
    N, D = X.shape
    dist = torch.empty(N, N, device=X.device, dtype=torch.float32)
    _lib.call("as_tsne_sqdist", X, X.stride(0), N, D, dist)
    return dist


def joint_probabilities(dist, perplexity, ws=None):
    """(P (N, N) float32, beta (N,) float64, entropy (N,) float64, steps (N,) int32) from the squared distances: scikit-learn's
    _joint_probabilities with the bisection of _binary_search_perplexity per row (as_tsne_joint_p)."""
    _lib.require_gpu(dist, "dist")
    N = dist.shape[0]
    dev = dist.device
    dist = _lib.contiguous(dist)
    P = torch.empty(N, N, device=dev, dtype=torch.float32)
    beta = torch.empty(N, device=dev, dtype=torch.float64)
    entropy = torch.empty(N, device=dev, dtype=torch.float64)
    steps = torch.empty(N, device=dev, dtype=torch.int32)
    if ws is None:
        ws = _workspace(N, dev)
    _lib.call("as_tsne_joint_p", dist, N, float(perplexity), P, beta, entropy, steps, ws, ws.numel())
    return P, beta, entropy, steps


def iterate(P, Y, update, gains, n_iters, it0, exaggeration, momentum, learning_rate, min_gain=MIN_GAIN, kl_every=N_ITER_CHECK,
            kl_last=False, grad=None, ws=None):
    """n_iters descent iterations in place on Y, update and gains ((N, 2) float32, contiguous), enqueued without a synchronisation
    (as_tsne_iterate).  Returns the (n_iters, 3) float64 log on the device: |grad|, |gains grad|, KL or NaN."""
    N = Y.shape[0]
    log = torch.empty(n_iters, 3, device=Y.device, dtype=torch.float64)
    if ws is None:
        ws = _workspace(N, Y.device)
    _lib.call("as_tsne_iterate", P, Y, update, gains, N, n_iters, it0, kl_every, int(kl_last), float(exaggeration), float(momentum),
              float(learning_rate), float(min_gain), grad, log, ws, ws.numel())
    return log


def pca_init(X):
    """scikit-learn's init="pca": the first two principal components of X, scaled so that the first has standard deviation 1e-4.
    Set-up, not the hot path: the covariance is a float64 matmul on the device, its eigenvectors come from a float64 eigh on the
    host; a component's sign makes its largest loading positive (scikit-learn's svd_flip on the components)."""
    Xd = X.to(torch.float64)
    Xc = Xd - Xd.mean(dim=0, keepdim=True)
    cov = (Xc.T @ Xc).cpu()
    _, V = torch.linalg.eigh(cov)
    V = V.flip(1)[:, :2].contiguous()
    V = V * torch.sign(V[V.abs().argmax(dim=0), torch.arange(2)])
    Y = Xc @ V.to(X.device)
    return (Y / (Y[:, 0].std(unbiased=False) * 1e4)).to(torch.float32).contiguous()


class TSNE:
    """``sklearn.manifold.TSNE`` for two components, the exact gradient, on the device.  Keywords and attributes are
    scikit-learn's: ``fit_transform(X)`` / ``fit(X)``, then ``embedding_`` ((N, 2) float32 on the device), ``kl_divergence_``,
    ``n_iter_``, ``learning_rate_``, and besides ``P_`` ((N, N) float32) and ``beta_`` ((N,) float64).  X is an (N, D) tensor on
    the device; anything else goes through ``torch.as_tensor`` and is uploaded.

    The schedule is scikit-learn's: ``learning_rate="auto"`` is max(N / early_exaggeration / 4, 50); 250 iterations at the early
    exaggeration with momentum 0.5 (and n_iter_without_progress taken as 250), the rest at exaggeration 1 with momentum 0.8 and
    update and gains started afresh; every 50 iterations the stopping rule (``stop_rule``) reads the log.  ``init`` is "pca",
    "random" (1e-4 times a standard normal from a torch.Generator seeded with ``random_state``) or an (N, 2) array.

    Deliberate differences from scikit-learn:
      * ``method`` defaults to "exact" and "barnes_hut" raises NotImplementedError.  scikit-learn's default is Barnes-Hut; at the
        reference's N <= 4500 an exact iteration is two kernel launches, which costs less than building a tree would.
      * ``n_components`` must be 2 and ``metric`` must be "euclidean".
      * non-finite input raises ValueError (scikit-learn's validate_data does too, with another message).
      * the KL divergence the stopping rule follows is that of the unexaggerated P in both phases (scikit-learn's first phase
        reports the divergence of 12 P, which is not a distribution); ``kl_divergence_`` is the last iteration's in both.
      * arithmetic: the gradient's pair sums are float32 products added in float64; Y, update and gains are float32."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="pca", random_state=None, method="exact"):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.metric = metric
        self.init = init
        self.random_state = random_state
        self.method = method

    def _check(self, X):
        if self.method == "barnes_hut":
            raise NotImplementedError("TSNE: method='barnes_hut' is not built (the exact gradient is what runs on the device); "
                                      "use method='exact'")
        if self.method != "exact":
            raise ValueError(f"TSNE: unknown method {self.method!r}")
        if self.n_components != 2:
            raise ValueError(f"TSNE: n_components must be 2, got {self.n_components}")
        if self.metric != "euclidean":
            raise ValueError(f"TSNE: metric must be 'euclidean', got {self.metric!r}")
        if not (self.learning_rate == "auto" or float(self.learning_rate) > 0.0):
            raise ValueError(f"TSNE: learning_rate must be 'auto' or positive, got {self.learning_rate!r}")
        if int(self.max_iter) < EXPLORATION_MAX_ITER:
            raise ValueError(f"TSNE: max_iter must be at least {EXPLORATION_MAX_ITER}, got {self.max_iter}")
        if float(self.early_exaggeration) < 1.0:
            raise ValueError(f"TSNE: early_exaggeration must be at least 1, got {self.early_exaggeration}")
        X = torch.as_tensor(X)
        if X.dim() != 2 or X.shape[1] < 1:
            raise ValueError(f"TSNE: X must be (N, D), got {tuple(X.shape)}")
        N = X.shape[0]
        if N < 2:
            raise ValueError("TSNE: at least 2 points are needed")
        if not 0.0 < float(self.perplexity) < N:
            raise ValueError(f"TSNE: perplexity ({self.perplexity}) must be positive and less than n_samples ({N})")
        if N > MAX_POINTS:
            raise ValueError(f"TSNE: {N} points exceed the supported {MAX_POINTS}")
        if not bool(torch.isfinite(X).all()):
            raise ValueError("TSNE: X holds NaN or infinity")
        if not isinstance(self.init, str):
            init = torch.as_tensor(self.init)
            if tuple(init.shape) != (N, 2):
                raise ValueError(f"TSNE: init must be 'pca', 'random' or an ({N}, 2) array, got {tuple(init.shape)}")
        elif self.init not in ("pca", "random"):
            raise ValueError(f"TSNE: init must be 'pca', 'random' or an (N, 2) array, got {self.init!r}")
        return X

    def _init(self, X):
        if not isinstance(self.init, str):
            return torch.as_tensor(self.init).to(device=X.device, dtype=torch.float32).contiguous().clone()
        if self.init == "pca":
            return pca_init(X)
        gen = torch.Generator(device="cpu")
        if self.random_state is None:
            gen.seed()
        else:
            gen.manual_seed(int(self.random_state))
        return (1e-4 * torch.randn(X.shape[0], 2, generator=gen, dtype=torch.float32)).to(X.device)

    def fit(self, X):
        X = self._check(X)
        if not X.is_cuda:
            X = X.to(torch.device("cuda", torch.cuda.current_device()))
        X = X.detach().to(torch.float32)
        N = X.shape[0]
        dev = X.device
        ws = _workspace(N, dev)
        self.P_, self.beta_, self.entropy_, self.bisection_steps_ = joint_probabilities(squared_distances(X), self.perplexity, ws)
        Y = self._init(X)
        self.learning_rate_ = (max(N / float(self.early_exaggeration) / 4.0, 50.0) if self.learning_rate == "auto"
                               else float(self.learning_rate))
        logs = []
        # (first iteration, one past the last, exaggeration, momentum, n_iter_without_progress) of scikit-learn's two calls
        phases = [(0, EXPLORATION_MAX_ITER, float(self.early_exaggeration), 0.5, EXPLORATION_MAX_ITER),
                  (EXPLORATION_MAX_ITER, int(self.max_iter), 1.0, 0.8, int(self.n_iter_without_progress))]
        last, error = -1, float("nan")
        for first, end, exaggeration, momentum, patience in phases:
            start = max(first, last + 1)   # the second call begins one past the iteration the first one ended at
            if start >= end:
                continue
            update, gains = torch.zeros_like(Y), torch.ones_like(Y)
            best_error, best_iter, stopped = float("inf"), start, None
            while start < end and stopped is None:
                n = min(N_ITER_CHECK - start % N_ITER_CHECK, end - start)
                log = iterate(self.P_, Y, update, gains, n, start, exaggeration, momentum, self.learning_rate_,
                              kl_last=start + n == end, ws=ws).cpu().numpy()   # the one read-back per chunk
                logs.append(log)
                stopped, best_error, best_iter = stop_rule(log, start, best_error, best_iter, patience, float(self.min_grad_norm))
                start += n
            last = start - 1 if stopped is None else stopped
            error = float(log[-1, 2])
        self.n_iter_ = last
        self.kl_divergence_ = error
        self.log_ = np.concatenate(logs)
        self.embedding_ = Y
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_


def sample_features_per_class(features, targets, class_ids, max_items_per_class=100, generator=None):
    """The selection step of the reference's plot_features (:343-353): for every token id of ``class_ids`` (in their order) at most
    ``max_items_per_class`` of the frames whose target is that token, drawn by a seeded permutation; tokens without a frame are
    skipped.  features (M, H) and targets (M,) stay where they are (device tensors stay on the device).  Returns (the gathered
    features, their tokens).

    The reference draws WITH replacement (np.random.choice's default), which can only add coincident points to the map; here
    the draw is without replacement."""
    features, targets = torch.as_tensor(features), torch.as_tensor(targets)
    if features.dim() != 2 or targets.shape != (features.shape[0],):
        raise ValueError("sample_features_per_class: features must be (M, H) and targets (M,)")
    if int(max_items_per_class) < 1:
        raise ValueError("sample_features_per_class: max_items_per_class must be at least 1")
    picked = []
    for token in class_ids:
        idx = (targets == int(token)).nonzero().reshape(-1)
        if idx.numel() == 0:
            continue
        order = torch.randperm(idx.numel(), generator=generator)[:int(max_items_per_class)]
        picked.append(idx[order.to(idx.device)])
    if not picked:
        return features[:0], targets[:0]
    picked = torch.cat(picked)
    return features[picked], targets[picked]


def _embed_features(features, targets, vocabulary, groups, max_items_per_class, seed, tsne_kwargs):
    """feature_embedding's work; returns the fitted TSNE as well."""
    if groups is None:
        from . import PHONETIC_CLASSES as groups
    class_ids, group_of = [], {}
    for g, (_, tokens) in enumerate(groups.items()):
        for token in tokens:
            if token in vocabulary:
                class_ids.append(int(vocabulary[token]))
                group_of[int(vocabulary[token])] = g
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    feats, tokens = sample_features_per_class(features, targets, class_ids, max_items_per_class, gen)
    if feats.shape[0] < 2:
        raise ValueError(f"feature_embedding: {feats.shape[0]} frames carry a token of the groups; nothing to embed")
    tsne = TSNE(**{"random_state": seed, **tsne_kwargs})
    embedding = tsne.fit_transform(feats)
    lut = torch.full((max(group_of) + 1,), -1, dtype=torch.int64)
    for token, g in group_of.items():
        lut[token] = g
    tokens = tokens.to(torch.int64)
    return embedding, tokens, lut.to(tokens.device)[tokens], tsne


def feature_embedding(features, targets, vocabulary, groups=None, max_items_per_class=100, seed=0, **tsne_kwargs):
    """The map of plot_features without the figure: sample at most ``max_items_per_class`` frames of every token of ``groups``
    ({group: [tokens]}, PHONETIC_CLASSES by default; a token the vocabulary lacks is skipped), embed them with ``TSNE`` and return
    (embedding (M, 2) float32 on the device, tokens (M,) int64, group index (M,) int64: the position of the token's group in
    ``groups``, as the reference colours it).  ``seed`` seeds the draw and, unless ``random_state`` is given, the embedding."""
    return _embed_features(features, targets, vocabulary, groups, max_items_per_class, seed, tsne_kwargs)[:3]


def plot_features(features, targets, class_map, max_items_per_class, save_filepath, plot_groups, seed=0, **tsne_kwargs):
    """The reference's plot_features (:332-399): the scatter plot of the embedding, one colour of the "hsv" map per group, and its
    legend in ``<name>_legend.pdf``.  ``class_map`` is {token: id} for the tokens to draw.  Returns (embedding, tokens, group
    index) as ``feature_embedding`` does.  matplotlib is imported here; without it nothing is drawn and a log line says so."""
    embedding, tokens, group_idx = feature_embedding(features, targets, class_map, plot_groups, max_items_per_class, seed, **tsne_kwargs)
    draw_embedding(embedding.cpu().numpy(), group_idx.cpu().numpy(), plot_groups, save_filepath)
    return embedding, tokens, group_idx


def draw_embedding(embedding, group_idx, plot_groups, save_filepath):
    """The figure and its legend (reference :358-399) from a host embedding; False (and a log line) without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logging.info(f"matplotlib is not installed: {save_filepath} is not drawn")
        return False
    cmap = plt.get_cmap("hsv")
    fig, ax = plt.subplots(figsize=(10, 10))
    for g, (_, classes) in enumerate(plot_groups.items()):
        points = embedding[group_idx == g]
        if len(points) == 0:
            continue
        ax.scatter(*points.T, alpha=0.7, c=[cmap(g / len(plot_groups))] * len(points), label=" ".join(classes))
    ax.xaxis.set_ticklabels([])
    ax.yaxis.set_ticklabels([])
    handles, labels = ax.get_legend_handles_labels()
    fig.tight_layout()
    fig.savefig(save_filepath)
    plt.close(fig)
    legend = plt.figure(figsize=(5, 3))
    axi = legend.add_subplot(111)
    axi.legend(handles, labels, loc="center", ncol=1, fontsize=22, markerscale=2)
    axi.axis("off")
    name, ext = os.path.splitext(os.path.basename(save_filepath))
    legend.savefig(os.path.join(os.path.dirname(save_filepath), f"{name}_legend{ext}"), bbox_inches="tight")
    plt.close(legend)
    return True
