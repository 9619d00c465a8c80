"""Host-side checks of the contour preparation (no GPU): the index-arithmetic restatement tests/contours_ref.py against the
fixture recorded from the reference's own TailClipper and prepare_articulator_array (tests/golden/make_golden_contours.py), the
nearest-index table against F.interpolate, the loader on a file tree, the names the reference exposes, the new entry points of
the header and the statistics script's import."""
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import contours_ref as Y
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def fx():
    return load_golden("contours")


def fixture_inputs(fx):
    """(articulators, raw (F, A, 50, 2), refs (F, 3, 50, 2), kinds, thresholds) of the fixture"""
    from artspeech_amd.settings import DATASET_CONFIG
    arts = [str(a) for a in fx["articulators"]]
    refs = np.stack([fx["lower_incisor"], fx["raw"][:, arts.index("upper-incisor")], fx["epiglottis"]], axis=1)
    return arts, fx["raw"], refs, Y.kinds_of(arts), Y.thresholds(DATASET_CONFIG[str(fx["database_name"])])


def test_fixture_covers_the_counts_and_the_reference_raised_nowhere(fx):
    arts = [str(a) for a in fx["articulators"]]
    assert fx["raw"].shape == (96, 5, 50, 2) and arts == sorted(arts)
    for kind, lowest in (("tongue", 1), ("lower-lip", 25), ("upper-lip", 1)):   # the lower lip always keeps one half
        seen = set(fx["counts"][:, arts.index(kind)].tolist())
        assert {50, 49, 26, 25, lowest} <= seen and 0 not in seen, (kind, sorted(seen))
    assert not np.isnan(fx["clipped"]).any() and not np.isnan(fx["prepared_norm"]).any()
    assert fx["empty_raised"].tolist() == ["RuntimeError", "RuntimeError"]


def test_restatement_equals_the_reference_bit_for_bit(fx):
    arts, raw, refs, kinds, thr = fixture_inputs(fx)
    clipped, counts = Y.clip_batched(raw, refs, kinds, thr)
    at = [arts.index(str(k)) for k in fx["clipped_articulators"]]
    assert clipped[:, at].tobytes() == fx["clipped"].tobytes()
    assert np.array_equal(counts, fx["counts"])
    for a, kind in enumerate(kinds):
        if kind == 0:
            assert clipped[:, a].tobytes() == raw[:, a].tobytes() and (counts[:, a] == 50).all()
    targets, references, counts2 = Y.prepare(raw, refs, kinds, thr)
    assert targets.tobytes() == fx["prepared"].tobytes() and references.tobytes() == fx["references"].tobytes()
    assert np.array_equal(counts2, counts)
    targets, references, _ = Y.prepare(raw, refs, kinds, thr, fx["norm_mean"], fx["norm_std"])
    assert targets.tobytes() == fx["prepared_norm"].tobytes() and references.tobytes() == fx["references"].tobytes()
    targets, _, counts0 = Y.prepare(raw, refs, [0] * len(arts), thr)
    assert targets[:, arts.index("tongue")].tobytes() == fx["unclipped_tongue"].tobytes() and (counts0 == 50).all()


def test_restatement_marks_the_emptied_contours(fx):
    arts, _, _, kinds, thr = fixture_inputs(fx)
    clipped, counts = Y.clip_batched(fx["empty_raw"][None], fx["empty_refs"][None], kinds, thr)
    assert counts[0, arts.index("tongue")] == 0 and counts[0, arts.index("upper-lip")] == 0
    assert np.isnan(clipped[0, arts.index("tongue")]).all() and not np.isnan(clipped[0, arts.index("lower-lip")]).any()


def test_nearest_index_table_is_interpolates():
    for n in range(1, 51):
        want = F.interpolate(torch.arange(n, dtype=torch.float32)[None, None], size=50)[0, 0].numpy().astype(np.int64)
        assert np.array_equal(Y.nearest_index(n), want), n


def test_statistics_fixture_is_torchs_view_of_the_fp64_values(fx):
    """the recorded torch mean / std of the prepared contours lie within float32 accumulation error of the fp64 restatement"""
    mean, std = Y.column_stats_fp64(fx["prepared"].reshape(96, -1))
    assert np.abs(fx["stats_mean"].reshape(-1) - mean).max() <= 1e-5 * np.abs(mean).max()
    assert np.abs(fx["stats_std"].reshape(-1) - std).max() <= 1e-5 * np.abs(std).max()
    m1, s1 = Y.column_stats_fp64(np.ones((1, 3), np.float32))
    assert (m1 == 1).all() and np.isnan(s1).all()


def test_load_raw_contours_reads_both_orientations(tmp_path):
    from artspeech_amd.phoneme_to_articulation import cached_load_articulator_array, load_articulator_array, load_raw_contours
    rng = np.random.RandomState(0)
    names = ["tongue", "pharynx"] + Y.REFERENCES
    directory = tmp_path / "S1" / "seq" / "inference_contours"
    os.makedirs(directory)
    pixels = {}
    for frame in ("0001", "0002"):
        for i, name in enumerate(names):
            pixels[frame, name] = rng.rand(50, 2) * 136
            np.save(directory / f"{frame}_{name}.npy", pixels[frame, name] if i % 2 else pixels[frame, name].T)
    raw, refs = load_raw_contours(str(tmp_path), "S1", "seq", ["0001", "0002"], ["tongue", "pharynx"])
    assert raw.shape == (2, 2, 50, 2) and refs.shape == (2, 3, 50, 2) and raw.dtype == refs.dtype == torch.float32
    for f, frame in enumerate(("0001", "0002")):
        for a, name in enumerate(("tongue", "pharynx")):
            assert np.array_equal(raw[f, a].numpy(), (pixels[frame, name] / 136).astype(np.float32))
        for r, name in enumerate(Y.REFERENCES):
            assert np.array_equal(refs[f, r].numpy(), (pixels[frame, name] / 136).astype(np.float32))
    one = load_articulator_array(str(directory / "0001_tongue.npy"), 136)
    assert one.shape == (50, 2) and one.dtype == np.float64
    path = str(directory / "0001_tongue.npy")
    assert cached_load_articulator_array(path, 136) is cached_load_articulator_array(path, 136), "the file read is cached"
    with pytest.raises(FileNotFoundError, match="0003_tongue.npy"):
        load_raw_contours(str(tmp_path), "S1", "seq", ["0003"], ["tongue"])


def test_tail_clipper_exposes_the_references_names():
    from artspeech_amd.phoneme_to_articulation import InputLoaderMixin, TailClipper
    from artspeech_amd.phoneme_to_articulation import tail_clipper
    from artspeech_amd.settings import DATASET_CONFIG
    assert TailClipper.TAIL_CLIP_REFERENCES == Y.REFERENCES and tail_clipper.CLIP_KINDS == Y.KINDS
    clipper = TailClipper(DATASET_CONFIG["artspeech2"])
    assert clipper.dataset_config is DATASET_CONFIG["artspeech2"]
    every = {name.replace("-", "_"): None for name in Y.REFERENCES}
    for method, first in (("clip_tongue_tails", "tongue"), ("clip_lower_lip_tails", "lower_lip"), ("clip_upper_lip_tails", "upper_lip")):
        sig = inspect.signature(getattr(clipper, method))
        assert list(sig.parameters)[0] == first and list(sig.parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD
        sig.bind(None, **every)   # the references a method does not use are accepted
    assert getattr(clipper, "clip_pharynx_tails", None) is None
    params = list(inspect.signature(InputLoaderMixin.prepare_articulator_array).parameters)
    assert params == ["datadir", "subject", "sequence", "frame_id", "articulator", "dataset_config", "normalize_fn", "clip_tails"]
    got = tuple(np.float32(t) for t in tail_clipper.clip_thresholds(DATASET_CONFIG["artspeech2"]))
    assert got == Y.thresholds(DATASET_CONFIG["artspeech2"])
    assert tail_clipper.clip_kinds(["lower-lip", "pharynx", "tongue", "upper-lip"]) == [2, 0, 1, 3]
    assert tail_clipper.clip_kinds(["lower-lip", "tongue"], clip_tails=False) == [0, 0]


def test_synthetic_raw_contours_are_clipped_and_never_emptied():
    from artspeech_amd.phoneme_to_articulation import SyntheticRawContours
    from artspeech_amd.settings import DATASET_CONFIG
    arts = ["lower-lip", "pharynx", "tongue", "upper-lip"]
    data = SyntheticRawContours(512, arts, seed=0)
    again = SyntheticRawContours(512, arts, seed=0)
    assert len(data) == 512 and data.raw.shape == (512, 4, 50, 2) and data.refs.shape == (512, 3, 50, 2)
    assert torch.equal(data.raw, again.raw) and torch.equal(data.refs, again.refs)
    li_y, ep_y = data.refs[:, 0, :, 1], data.refs[:, 2, :, 1]
    assert 0.3 <= li_y.min() and li_y.max() <= 0.7 and 0.2 <= ep_y.min() and ep_y.max() <= 0.7
    _, counts = Y.clip_batched(data.raw.numpy(), data.refs.numpy(), Y.kinds_of(arts), Y.thresholds(DATASET_CONFIG["artspeech2"]))
    assert counts.min() >= 1 and (counts[:, arts.index("upper-lip")] == 50).all(), "RES-normalised upper lips keep every point"
    assert (counts[:, arts.index("tongue")] < 50).mean() > 0.5 and (counts[:, arts.index("lower-lip")] < 50).mean() > 0.5


def test_header_declares_and_binding_binds_the_entry_points():
    from artspeech_amd import _lib
    with open(os.path.join(ROOT, "include", "artspeech_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = _lib.lib()
    for name, n_args in (("as_prepare_contours", 17), ("as_column_mean_std", 8)):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.PROTOTYPES and hasattr(L, name), f"{name} is not bound / exported"
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    part_rows = int(re.search(r"#define AS_COLUMN_STATS_PART_ROWS (\d+)", header).group(1))
    assert part_rows == _lib.COLUMN_STATS_PART_ROWS
    from artspeech_amd import build
    assert build.SOURCES["contours.hip"] == ["-ffp-contract=off"]


def test_statistics_script_imports_without_a_gpu_and_config_has_the_references_keys(monkeypatch):
    """a fresh import touches no device (this test runs where there is none) and main() takes the reference's YAML keys"""
    monkeypatch.delitem(sys.modules, "calculate_normalization_statistics", raising=False)
    script = importlib.import_module("calculate_normalization_statistics")
    keys = ["database_name", "datadir", "save_to", "sequences_dict", "articulators", "num_samples"]
    assert list(inspect.signature(script.main).parameters)[:6] == keys
    with open(os.path.join(ROOT, "configs", "normalization_statistics_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(keys) and cfg["datadir"] == "synthetic" and "num_frames" in cfg["sequences_dict"]


def test_host_tensors_mean_a_loud_error_not_a_host_path():
    from artspeech_amd.phoneme_to_articulation import contour_statistics, prepare_contours
    from artspeech_amd.settings import DATASET_CONFIG
    with pytest.raises(RuntimeError, match="MI355X"):
        prepare_contours(torch.zeros(1, 1, 50, 2), torch.zeros(1, 3, 50, 2), ["tongue"], DATASET_CONFIG["artspeech2"])
    with pytest.raises(RuntimeError, match="MI355X"):
        contour_statistics(torch.zeros(4, 3))
