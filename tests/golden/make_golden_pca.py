"""Writes tests/golden/pca_fit.npz with the REFERENCE's code: sklearn.decomposition.IncrementalPCA driven exactly as the
reference's train_articulatory_PCA.py:91-108 drives it (one partial_fit per loader batch on inputs[:, i, :], float32 batches) and
the reference's own make_multiarticulator_autoencoder (:38-51) for the two state dicts.  Runs only where the reference checkout
and scikit-learn are installed; the tests read the fixture, never the reference.

    python tests/golden/make_golden_pca.py [reference root]

The inputs are not stored: they are low_rank_frames(N, A, F, rank, seed) of this repository's dataset module, which the tests
regenerate; stored are the shapes and seeds, the batch order, every fitted attribute, the state dicts and the reconstruction of 64
held-out frames (low_rank_frames with seed + 1).
"""
import ast
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
from sklearn.decomposition import IncrementalPCA

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import low_rank_frames  # noqa: E402

ATTRS = ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_", "mean_", "var_")
# (N, F, batch, seed, rank, {articulator: k} in the trainer's dict order)
CASES = [(2048, 100, 256, 21, 24, OrderedDict([("tongue", 8), ("lower-lip", 4), ("pharynx", 3)])),
         (1000, 100, 13, 22, 24, OrderedDict([("upper-lip", 12), ("epiglottis", 2)]))]


def reference_function(reference_root, name):
    """one function of the reference's trainer, taken from the file without running the module's imports (mlflow is absent)"""
    path = os.path.join(reference_root, "train_articulatory_PCA.py")
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    scope = {"OrderedDict": OrderedDict, "torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    return scope[name]


def main(reference_root):
    make_multiarticulator_autoencoder = reference_function(reference_root, "make_multiarticulator_autoencoder")
    out = {"n_cases": np.int64(len(CASES))}
    for case, (N, F, batch_size, seed, rank, indices_dict) in enumerate(CASES):
        pre = f"c{case}."
        articulators = sorted(indices_dict.keys())
        frames = low_rank_frames(N, len(articulators), F, rank, torch.Generator().manual_seed(seed)).float()
        order = torch.randperm(N, generator=torch.Generator().manual_seed(seed)).numpy()
        transformers = {}
        for articulator, num_indices in indices_dict.items():
            transformers[articulator] = IncrementalPCA(n_components=num_indices, batch_size=batch_size)
        for start in range(0, N, batch_size):                           # the loader's batches, the last one short
            inputs = frames[order[start:start + batch_size]].numpy()
            for i, articulator in enumerate(articulators):
                transformers[articulator].partial_fit(inputs[:, i, :])
        encoder_dict, decoder_dict = make_multiarticulator_autoencoder(transformers)
        held = low_rank_frames(64, len(articulators), F, rank, torch.Generator().manual_seed(seed + 1)).float().numpy()
        outputs = []
        for i, articulator in enumerate(articulators):
            latents = transformers[articulator].transform(held[:, i, :])
            outputs.append(transformers[articulator].inverse_transform(latents))
        out[pre + "shape"] = np.array([N, len(articulators), F, batch_size, seed, rank], np.int64)
        out[pre + "articulators"] = np.array(list(indices_dict.keys()))
        out[pre + "k"] = np.array(list(indices_dict.values()), np.int64)
        out[pre + "order"] = order.astype(np.int32)
        out[pre + "reconstruction"] = np.stack(outputs, axis=1).astype(np.float32)
        for articulator, transformer in transformers.items():
            for name in ATTRS:
                out[f"{pre}{articulator}.{name}"] = np.asarray(getattr(transformer, name))
            out[f"{pre}{articulator}.n_samples_seen_"] = np.int64(transformer.n_samples_seen_)
        for which, sd in (("enc", encoder_dict), ("dec", decoder_dict)):
            out[f"{pre}{which}.keys"] = np.array(list(sd.keys()))
            for i, value in enumerate(sd.values()):
                out[f"{pre}{which}.{i}"] = value.numpy()
    path = os.path.join(HERE, "pca_fit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    from make_golden import REF  # noqa: E402  (the reference checkout the other fixture writers use)
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
