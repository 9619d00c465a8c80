"""Exact t-SNE restated in numpy float64, from the published algorithm (van der Maaten & Hinton 2008) and scikit-learn's documented
behaviour: what artspeech_amd/csrc/tsne.hip and artspeech_amd/phoneme_recognition/tsne.py are compared against.  Dense (N, N)
matrices with a zero diagonal throughout (scikit-learn works on the condensed upper triangle: the same numbers)."""
import numpy as np

EPS = float(np.finfo(np.double).eps)   # scikit-learn's MACHINE_EPSILON
PERPLEXITY_TOLERANCE = 1e-5
BISECTION_STEPS = 100
EPSILON_DBL = 1e-8                     # a row whose exponentials all underflow
N_ITER_CHECK = 50
EXPLORATION_ITERS = 250


def sqdist(X):
    """dist[i][j] = sum_k (x_ik - x_jk)^2 by direct differences, in float64 on the inputs as given."""
    X = np.asarray(X, np.float64)
    out = np.empty((len(X), len(X)))
    for i in range(len(X)):
        d = X[i] - X
        out[i] = (d * d).sum(axis=1)
    return out


def binary_search_perplexity(dist, perplexity):
    """Per row the bisection on beta: start at 1, at most 100 steps, stop at |H - log perplexity| <= 1e-5; while an end of the
    interval is still open beta doubles (H too large) or halves.  Returns (conditional P, beta, H, steps) where beta, H and the
    row of P belong to the last evaluation and steps counts the evaluations.  The distances are rounded to float32 first, as
    scikit-learn's _joint_probabilities rounds them (and as the device holds them); the search itself is float64."""
    dist = np.asarray(dist, np.float32).astype(np.float64)
    N = len(dist)
    target = np.log(perplexity)
    C = np.zeros((N, N))
    betas, Hs, steps = np.empty(N), np.empty(N), np.empty(N, np.int32)
    for i in range(N):
        d = np.delete(dist[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for step in range(1, BISECTION_STEPS + 1):
            e = np.exp(-d * beta)
            s = e.sum()
            if s == 0.0:
                s = EPSILON_DBL
            H = np.log(s) + beta * (d * e).sum() / s
            diff = H - target
            if abs(diff) <= PERPLEXITY_TOLERANCE or step == BISECTION_STEPS:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        C[i, np.arange(N) != i] = e / s
        betas[i], Hs[i], steps[i] = beta, H, step
    return C, betas, Hs, steps


def joint_probabilities(dist, perplexity):
    """(P, beta, H, steps): P = max((C + C') / max(sum(C + C'), eps), eps) off the diagonal, 0 on it."""
    C, beta, H, steps = binary_search_perplexity(dist, perplexity)
    S = C + C.T
    P = np.maximum(S / max(S.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta, H, steps


def kl_and_gradient(P, Y, exaggeration=1.0):
    """(KL of the unexaggerated P, gradient with P scaled by `exaggeration`, Z).  num_ij = 1 / (1 + |y_i - y_j|^2), num_ii = 0,
    Z = sum num;  grad_i = 4 (e sum_j p_ij num_ij (y_i - y_j) - sum_j num_ij^2 (y_i - y_j) / Z);
    KL = 2 sum_{i<j} p_ij log(max(p_ij, eps) / max(num_ij / Z, eps))."""
    P, Y = np.asarray(P, np.float64), np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    num = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    np.fill_diagonal(num, 0.0)
    Z = num.sum()
    attr = ((P * num)[:, :, None] * diff).sum(axis=1)
    rep = ((num * num)[:, :, None] * diff).sum(axis=1)
    grad = 4.0 * (exaggeration * attr - rep / Z)
    iu = np.triu_indices(len(Y), 1)
    p, q = P[iu], np.maximum(num[iu] / Z, EPS)
    kl = 2.0 * float(np.dot(p, np.log(np.maximum(p, EPS) / q)))
    return kl, grad, Z


def descent_step(P, Y, update, gains, exaggeration, momentum, learning_rate, min_gain=0.01):
    """One iteration of scikit-learn's _gradient_descent.  Returns a dict: grad, gains, update, Y (all new arrays), grad_norm (of the
    gradient), gained_norm (of gains * grad: the norm scikit-learn compares with min_grad_norm), kl (at the Y given) and
    decision = update * grad as the gains saw it."""
    kl, grad, _ = kl_and_gradient(P, Y, exaggeration)
    decision = update * grad
    inc = decision < 0.0
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, min_gain)
    gained = grad * gains
    update = momentum * update - learning_rate * gained
    return dict(grad=grad, gains=gains, update=update, Y=Y + update, grad_norm=float(np.linalg.norm(grad)),
                gained_norm=float(np.linalg.norm(gained)), kl=kl, decision=decision)


def stop_rule(log, it0, best_error, best_iter, n_iter_without_progress, min_grad_norm, n_iter_check=N_ITER_CHECK):
    """scikit-learn's convergence check walked over log rows (|grad|, |gains grad|, KL) of iterations it0, it0 + 1, ...: on every
    iteration i with (i + 1) % n_iter_check == 0 a KL below the best so far becomes the best, otherwise more than
    n_iter_without_progress iterations since the best stop the descent; then a gained norm <= min_grad_norm stops it.
    Returns (iteration it stopped at or None, best_error, best_iter)."""
    for k, (_, gained_norm, error) in enumerate(np.asarray(log, np.float64).reshape(-1, 3)):
        i = it0 + k
        if (i + 1) % n_iter_check:
            continue
        if error < best_error:
            best_error, best_iter = float(error), i
        elif i - best_iter > n_iter_without_progress:
            return i, best_error, best_iter
        if gained_norm <= min_grad_norm:
            return i, best_error, best_iter
    return None, best_error, best_iter


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def descend(P, Y0, iters, early_exaggeration=12.0, learning_rate=None, record=()):
    """The first `iters` iterations of scikit-learn's schedule from Y0 (no stopping rule): 250 at the exaggeration with momentum
    0.5, then exaggeration 1 and momentum 0.8 with update and gains started afresh.  Returns (Y, states) where states[i] is
    (Y, update, gains) as iteration i (0-based) finds them, for the i in `record`."""
    Y = np.array(Y0, np.float64)
    lr = auto_learning_rate(len(Y), early_exaggeration) if learning_rate is None else learning_rate
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    states = {}
    for i in range(iters):
        if i == EXPLORATION_ITERS:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        e, m = (early_exaggeration, 0.5) if i < EXPLORATION_ITERS else (1.0, 0.8)
        if i in record:
            states[i] = (Y.copy(), update.copy(), gains.copy())
        s = descent_step(P, Y, update, gains, e, m, lr)
        Y, update, gains = s["Y"], s["update"], s["gains"]
    return Y, states


def pca_init(X):
    """The first two principal components of X scaled so that the first has standard deviation 1e-4 (scikit-learn's init="pca");
    a component's sign makes its largest loading positive."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2]
    V = V * np.sign(V[np.abs(V).argmax(axis=0), np.arange(2)])
    Y = Xc @ V
    return Y / (Y[:, 0].std() * 1e4)


def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness with the euclidean metric: 1 - 2 / (N k (2 N - 3 k - 1)) sum_i sum_{j in kNN_Y(i)}
    max(0, rank_X(i, j) - k), rank 1 = the nearest other point in X."""
    dX, dY = sqdist(X), sqdist(Y)
    N, k = len(dX), n_neighbors
    np.fill_diagonal(dX, np.inf)
    np.fill_diagonal(dY, np.inf)
    order_X = np.argsort(dX, axis=1, kind="stable")
    rank_X = np.empty((N, N), np.int64)
    rank_X[np.arange(N)[:, None], order_X] = np.arange(1, N + 1)[None, :]
    nn_Y = np.argsort(dY, axis=1, kind="stable")[:, :k]
    excess = np.maximum(rank_X[np.arange(N)[:, None], nn_Y] - k, 0)
    return 1.0 - 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)) * float(excess.sum())


def clusters(seed=0, n_clusters=8, per_cluster=25, D=32, spread=4.0):
    """The fixture's data: Gaussian clusters of unit variance whose centres are drawn at `spread` sigma.  (X float32, labels)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, D)) * spread
    labels = np.repeat(np.arange(n_clusters), per_cluster)
    X = centres[labels] + rng.standard_normal((len(labels), D))
    return X.astype(np.float32), labels.astype(np.int64)
