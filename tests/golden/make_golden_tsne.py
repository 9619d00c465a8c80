"""Records tests/golden/tsne.npz from scikit-learn and the float64 restatement (tests/tsne_fp64.py):
    python tests/golden/make_golden_tsne.py
  X, labels        8 Gaussian clusters x 25 points, D = 32, centres drawn at 4 sigma (tsne_fp64.clusters, seed 0); X is float32
  P_sklearn        scikit-learn's _joint_probabilities for perplexity 10, as a dense (200, 200) float64 matrix
  sk_kl, sk_trust  kl_divergence_ and trustworthiness(X, Y, n_neighbors=5) of TSNE(method="exact", perplexity=10, max_iter=500) for
                   init="pca" with seeds 0-3 and init="random" with seeds 0-2 (sk_init, sk_seed name the runs)
  Y0               the restatement's PCA initialisation, float32
  it100_*, it280_* (Y, update, gains) as iterations 100 and 280 of the restatement's descent find them, stored as float32 (what the
                   device is started from); exaggeration 12 and 1.  The descent starts from the float64 PCA initialisation and
                   runs on float32(P_sklearn), the matrix that the device's step tests are given
The script asserts that no gain decision of those two states sits within rounding of zero."""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE, _t_sne, trustworthiness
from sklearn.metrics import pairwise_distances

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_fp64 as R  # noqa: E402

PERPLEXITY = 10.0


def main():
    X, labels = R.clusters()
    out = {"X": X, "labels": labels}
    d = pairwise_distances(X, metric="euclidean", squared=True)
    out["P_sklearn"] = squareform(_t_sne._joint_probabilities(d, PERPLEXITY, 0))
    runs = [("pca", s) for s in range(4)] + [("random", s) for s in range(3)]
    kl, trust = [], []
    for init, seed in runs:
        t = TSNE(method="exact", perplexity=PERPLEXITY, max_iter=500, init=init, random_state=seed)
        Y = t.fit_transform(X)
        kl.append(t.kl_divergence_)
        trust.append(trustworthiness(X, Y, n_neighbors=5))
        print(f"scikit-learn init={init} seed={seed}: KL {kl[-1]:.4f} trustworthiness {trust[-1]:.4f}")
    out.update(sk_kl=np.array(kl), sk_trust=np.array(trust), sk_init=np.array([r[0] for r in runs]), sk_seed=np.array([r[1] for r in runs]))
    Y0 = R.pca_init(X)                  # float64: the restatement descends from it as it is
    out["Y0"] = Y0.astype(np.float32)   # what the device (and the five-step comparison) starts from
    P = out["P_sklearn"].astype(np.float32).astype(np.float64)   # the matrix the step tests hand to the device, bit for bit
    _, states = R.descend(P, Y0, 281, record=(100, 280))
    for it, e in ((100, 12.0), (280, 1.0)):
        Y, update, gains = (a.astype(np.float32) for a in states[it])
        decision = np.abs(update.astype(np.float64) * R.kl_and_gradient(P, Y, e)[1])
        margin = decision.min() / np.median(decision)
        print(f"iteration {it}: min |update grad| / median |update grad| = {margin:.2e}")
        assert margin > 1e-4, margin   # float32 rounding (6e-8) cannot flip a gain decision
        out.update({f"it{it}_Y": Y, f"it{it}_update": update, f"it{it}_gains": gains})
    path = os.path.join(HERE, "tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
