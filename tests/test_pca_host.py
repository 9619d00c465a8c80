"""CPU tests of the incremental PCA's host side: the float64 yardstick against scikit-learn and against the fixture written with
the reference's own code, the C ABI's limits (refused before any launch), loud failure without a GPU, the shape errors, the
trainer's config contract, the ``rank=`` extension of the synthetic dataset and the ctypes mirror of ``as_pca``."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, load_golden
from pca_fp64 import IncrementalPCAYardstick

EPS32 = float(np.finfo(np.float32).eps)
ATTRS = ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_")


def _frames(N, A, F, seed, rank=24):
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import low_rank_frames
    return low_rank_frames(N, A, F, rank, torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("N,F,k,b", [(2048, 100, 12, 256), (1000, 100, 12, 13), (640, 20, 4, 32), (1024, 100, 8, 8)])
def test_yardstick_equals_sklearn_on_float64_input(N, F, k, b):
    sklearn_pca = pytest.importorskip("sklearn.decomposition").IncrementalPCA
    x = _frames(N, 1, F, seed=N + k)[:, 0].numpy().astype(np.float64)
    ref = sklearn_pca(n_components=k, batch_size=b)
    for i in range(0, N, b):
        ref.partial_fit(x[i:i + b].copy())
    y = IncrementalPCAYardstick(k).fit(x, b)
    assert y.eigenvalue_gap() >= 1e-4
    for name in ATTRS + ("mean_", "var_"):
        want = np.asarray(getattr(ref, name))
        assert np.abs(np.asarray(getattr(y, name)) - want).max() <= 1e-9 * max(1.0, float(np.abs(want).max())), name
    assert y.n_samples_seen_ == ref.n_samples_seen_
    held = _frames(16, 1, F, seed=1)[:, 0].numpy().astype(np.float64)
    assert np.abs(y.inverse_transform(y.transform(held)) - ref.inverse_transform(ref.transform(held))).max() <= 1e-9


def test_yardstick_reproduces_the_reference_fixture():
    g = load_golden("pca_fit")
    assert int(g["n_cases"]) == 2
    for case in range(int(g["n_cases"])):
        pre = f"c{case}."
        N, A, F, b, seed, rank = (int(v) for v in g[pre + "shape"])
        names = [str(s) for s in g[pre + "articulators"]]
        x = _frames(N, A, F, seed, rank).numpy()
        held = _frames(64, A, F, seed + 1, rank).numpy()
        for a, k in zip(names, g[pre + "k"]):
            i = sorted(names).index(a)
            y64 = IncrementalPCAYardstick(int(k)).fit(x[:, i], b, g[pre + "order"])
            y32 = IncrementalPCAYardstick(int(k), dtype=np.float32).fit(x[:, i], b, g[pre + "order"])
            assert y64.eigenvalue_gap() >= 1e-4
            for name in ATTRS:
                want = np.asarray(g[f"{pre}{a}.{name}"], np.float64)
                d_ref = float(np.abs(np.asarray(getattr(y32, name), np.float64) - np.asarray(getattr(y64, name), np.float64)).max())
                scale = 1.0 if name == "components_" else float(np.abs(want).max())
                bound = max(4.0 * d_ref, 8.0 * EPS32 * scale)
                err = float(np.abs(np.asarray(getattr(y64, name)) - want).max())
                assert err <= bound, (case, a, name, err, bound)
            for name in ("mean_", "var_"):
                want = g[f"{pre}{a}.{name}"]
                assert (np.abs(getattr(y64, name) - want) <= 1e-12 * np.abs(want)).all(), (case, a, name)
            assert int(g[f"{pre}{a}.n_samples_seen_"]) == y64.n_samples_seen_ == N
            rec = y64.inverse_transform(y64.transform(held[:, i]))
            assert np.abs(rec - g[pre + "reconstruction"][:, i]).max() <= 1e-4 * float(np.abs(held).max())
        for which, shapes in (("enc", lambda k: ((k,), (k, F))), ("dec", lambda k: ((k, 1), (k, F)))):   # the reference's layout
            keys = [str(s) for s in g[f"{pre}{which}.keys"]]
            assert keys == [f"{which}oders.{a}.{p}" for a in names for p in ("eigenvalues", "eigenvectors")]
            for j, (a, k) in enumerate(zip(names, g[pre + "k"])):
                assert (g[f"{pre}{which}.{2 * j}"].shape, g[f"{pre}{which}.{2 * j + 1}"].shape) == shapes(int(k))
                assert g[f"{pre}{which}.{2 * j}"].dtype == g[f"{pre}{which}.{2 * j + 1}"].dtype == np.float32


def test_limits_are_refused_before_any_launch():
    from artspeech_amd import _lib
    L = _lib.lib()
    assert L.as_pca_supported(100, 12) == 1 and L.as_pca_supported(256, 64) == 1 and L.as_pca_supported(8, 8) == 1
    assert L.as_pca_supported(257, 12) == 0 and L.as_pca_supported(100, 65) == 0 and L.as_pca_supported(8, 9) == 0
    assert L.as_pca_supported(0, 1) == 0 and L.as_pca_supported(100, 0) == 0
    d = _lib.Pca()
    d.groups, d.features, d.k_max, d.batch, d.rows = 1, 300, 12, 256, 1024   # no pointer is set: nothing may be touched
    assert L.as_pca_workspace_floats(C.byref(d)) == -1
    assert L.as_pca_fit(C.byref(d), None) == -2                     # AS_ERR_UNSUPPORTED
    assert b"limits" in L.as_last_error()
    d.features, d.k_max = 100, 65
    assert L.as_pca_fit(C.byref(d), None) == -2
    d.k_max = 12
    assert L.as_pca_workspace_floats(C.byref(d)) > 0
    assert L.as_pca_fit(C.byref(d), None) == -1                     # AS_ERR_BAD_ARG: null pointers, still no launch


def test_cpu_tensors_raise_and_shape_errors_are_value_errors():
    from artspeech_amd.phoneme_to_articulation.principal_components.pca import IncrementalPCA, MultiArticulatorPCA
    with pytest.raises(RuntimeError, match="no CPU path"):
        IncrementalPCA(4).partial_fit(torch.rand(32, 20))
    with pytest.raises(RuntimeError, match="no CPU path"):
        IncrementalPCA(4, batch_size=16).fit(torch.rand(32, 20))
    with pytest.raises(RuntimeError, match="no CPU path"):
        MultiArticulatorPCA({"tongue": 4, "pharynx": 2}, 16).fit(torch.rand(64, 2, 20))
    with pytest.raises(ValueError, match="number of features"):     # k > F
        IncrementalPCA(21).partial_fit(torch.rand(32, 20))
    with pytest.raises(ValueError, match="first batch"):            # first batch: k > m
        IncrementalPCA(8).partial_fit(torch.rand(4, 20))
    with pytest.raises(ValueError, match="first batch"):
        MultiArticulatorPCA({"tongue": 8, "pharynx": 2}, 4).fit(torch.rand(64, 2, 20))
    with pytest.raises(ValueError):
        MultiArticulatorPCA({"tongue": 4, "pharynx": 2}, 16).partial_fit(torch.rand(64, 3, 20))
    pca = MultiArticulatorPCA({"tongue": 4, "pharynx": 2}, 16)
    with pytest.raises(RuntimeError, match="not been fitted"):
        pca.components_
    with pytest.raises(RuntimeError, match="no CPU path"):
        pca.transform(torch.rand(4, 2, 20))


def test_config_keys_are_keyword_arguments_of_main():
    import train_articulatory_PCA as T
    with open(os.path.join(ROOT, "configs", "train_articulatory_pca_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    params = inspect.signature(T.main).parameters
    named = {n for n, p in params.items() if p.kind is not inspect.Parameter.VAR_KEYWORD}
    assert set(cfg) <= named, set(cfg) - named
    for name in ("database_name", "datadir", "batch_size", "train_seq_dict", "test_seq_dict", "model_params", "num_workers",
                 "clip_tails", "seed", "synthetic", "results_dir"):   # the reference's arguments plus the sibling trainers' extras
        assert name in params, name
    assert params["synthetic"].default is None and params["results_dir"].default is None
    thesis = {"tongue": 8, "lower-lip": 4, "upper-lip": 4, "soft-palate-midline": 3, "thyroid-cartilage": 2, "arytenoid-cartilage": 4,
              "epiglottis": 3, "lower-incisor": 3, "pharynx": 2, "vocal-folds": 2}
    assert cfg["model_params"]["indices_dict"] == thesis and list(cfg["model_params"]["indices_dict"]) == list(thesis)
    assert cfg["model_params"]["in_features"] == 100 and cfg["batch_size"] == 256 and cfg["datadir"] == "synthetic"
    ds = T._make_dataset("synthetic", "artspeech2", {"num_frames": 8}, sorted(thesis), True, cfg["synthetic"], 0)
    assert ds[0][1].shape == (10, 100)                               # the `synthetic:` key reaches the dataset's rank


def test_rank_none_dataset_is_unchanged_and_rank_gives_a_spectrum():
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import SyntheticPrincipalComponentsAutoencoderDataset as DS
    arts = ["tongue", "lower-lip", "pharynx"]
    a, b = DS(32, arts, seed=3), DS(32, arts, seed=3, rank=None)
    assert torch.equal(a._frames, b._frames) and a._phonemes == b._phonemes
    g = torch.Generator().manual_seed(3)                             # today's draw order: normalisers, phonemes, then the frames
    for _ in arts:
        torch.rand(2, 50, generator=g), torch.rand(2, 50, generator=g)
    torch.randint(0, 8, (32,), generator=g)
    assert torch.equal(a._frames, torch.rand(32, 3, 100, generator=g))
    assert a._frames.min() >= 0 and a._frames.max() <= 1
    r = DS(2048, arts, seed=3, rank=24)
    assert r._phonemes[:32] != [] and r._frames.shape == (2048, 3, 100) and r._frames.dtype == torch.float32
    assert torch.equal(r._frames, DS(2048, arts, seed=3, rank=24)._frames)
    for name in arts:
        assert torch.equal(r.normalize[name].mean, DS(2048, arts, seed=3).normalize[name].mean)
    s = torch.linalg.svdvals((r._frames[:, 0] - r._frames[:, 0].mean(0)).double()) / np.sqrt(2047)
    want = 0.25 * 0.7 ** np.arange(24)
    assert np.abs(s[:12].numpy() / want[:12] - 1).max() < 0.15       # the geometric spectrum ...
    assert 0.0015 < float(s[40]) < 0.003                             # ... over the 0.002 noise floor
    assert abs(float(r._frames.mean()) - 0.5) < 0.01
    item = r[5]
    assert item[0] == "synthetic_S1_00005" and item[1].shape == (3, 100)


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    from artspeech_amd import _lib
    fields = [name for name, _ in _lib.Pca._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "artspeech_hip.h"\nint main(void) {\n    printf("%zu", sizeof(as_pca));\n'
           + "".join(f'    printf(" %zu", offsetof(as_pca, {f}));\n' for f in fields) + '    printf("\\n");\n    return 0;\n}\n')
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    with open(c, "w") as f:
        f.write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [C.sizeof(_lib.Pca)] + [getattr(_lib.Pca, f).offset for f in fields]
    assert got == want, (got, want)
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    body = header[header.index("typedef struct as_pca {"):header.index("} as_pca;")]
    import re
    declared = re.findall(r"[\s\*]([a-z_0-9]+)\s*[,;]", body)
    assert declared == fields, (declared, fields)                    # every member mirrored, in order
