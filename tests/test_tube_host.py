"""Host-side pieces of the vocal-tract tube (no GPU): the restatement of tests/tube_fp64.py against independent formulations and
against the properties its definition promises, the library's argument checks, the data set that reads a synthesised tree and
the script that fills in its air columns."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import tube_fp64 as R
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("K,N,M", [(2, 7, 10), (6, 50, 100), (8, 33, 257), (3, 2, 5)])
def test_restatement_against_cdist_and_interp(K, N, M):
    distance = pytest.importorskip("scipy.spatial.distance")
    rng = np.random.default_rng(K * 100 + N)
    chain = rng.random((K, N, 2)).astype(np.float32)
    assert all(len(np.unique(c, axis=0)) == N for c in chain)                      # no duplicate points
    r = R.wall(chain, M)
    for k in range(K - 1):
        d = distance.cdist(chain[k].astype(np.float64), chain[k + 1].astype(np.float64), "sqeuclidean")
        two = np.sort(d, axis=None)[:2]
        assert two[1] - two[0] > 1e-5 * two[1], "the inputs must not leave the junction to rounding"
        assert tuple(r["junctions"][k]) == np.unravel_index(np.argmin(d), d.shape)
    assert (r["junctions"][K - 1:] == -1).all()
    q = r["q"]
    s = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(q, axis=0).T))])
    t = np.linspace(0.0, s[-1], M)
    want = np.stack([np.interp(t, s, q[:, 0]), np.interp(t, s, q[:, 1])], axis=1)
    assert r["P"] == len(q) and K <= r["P"] <= K * N
    assert np.abs(r["out"] - want).max() <= R.bound(r["P"], r["L"])
    assert np.array_equal(r["out"][0], q[0]) and np.array_equal(r["out"][-1], q[-1])


def test_reversing_any_subset_of_a_chain_gives_the_same_wall_bit_for_bit():
    rng = np.random.default_rng(1)
    chain = R.random_chain(rng, 4, 20)          # N even: neither end rule meets its tie
    want = R.wall(chain, 37)
    for subset in itertools.chain.from_iterable(itertools.combinations(range(4), n) for n in range(1, 5)):
        flipped = chain.copy()
        for k in subset:
            flipped[k] = flipped[k][::-1]
        got = R.wall(flipped, 37)
        assert np.array_equal(got["out"], want["out"]) and got["L"] == want["L"] and got["P"] == want["P"], subset


def test_an_arc_cut_into_overlapping_pieces_comes_back_as_one_wall_on_the_circle():
    rng = np.random.default_rng(2)
    for K in (2, 6, 8):
        chain = R.random_chain(rng, K, 50, noise=1e-3, reverse={1, 2, 4, 5})
        r = R.wall(chain, 100)
        radius = np.hypot(r["out"][:, 0], r["out"][:, 1])
        assert np.abs(radius - 1.0).max() <= 3e-3
        angle = np.arctan2(-r["out"][:, 0], r["out"][:, 1])   # measured from the arc's middle: no wrap at its ends
        arc = abs(angle[-1] - angle[0])                      # the arc between the wall's two ends, radius 1
        assert arc >= np.pi - 0.01 and r["L"] >= arc         # the whole half circle, and no shorter than it
        assert (np.diff(angle) > 0).all() or (np.diff(angle) < 0).all()


def _line(points):
    return np.asarray(points, dtype=np.float32)


def test_end_rules_and_a_chain_of_one():
    c0 = _line([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)])
    # three contours; the third stored backwards.  Junctions (4, 0) and (4, 4); runs 0..4, 0..4, 4..0
    c1 = _line([(4, .5), (5, .5), (6, .5), (7, .5), (8, .5)])
    c2 = _line([(12, 1), (11, 1), (10, 1), (9, 1), (8, 1)])
    r = R.wall(np.stack([c0, c1, c2]), 4)
    assert r["junctions"][:2].tolist() == [[4, 0], [4, 4]] and R.runs([(4, 0), (4, 4)], 3, 5) == [(0, 4), (0, 4), (4, 0)]
    assert r["q"].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [4, .5], [5, .5], [6, .5], [7, .5], [8, .5],
                               [8, 1], [9, 1], [10, 1], [11, 1], [12, 1]]
    assert r["P"] == 15 and r["L"] == 4 + .5 + 4 + .5 + 4 and r["out"][0].tolist() == [0, 0] and r["out"][-1].tolist() == [12, 1]
    # the first contour's tie: exit 2 of 5 leaves two points on either side, the run starts at index 0; the last contour's
    # entry 0 runs to N-1
    up = _line([(2, .5), (2, 1.5), (2, 2.5), (2, 3.5), (2, 4.5)])
    r = R.wall(np.stack([c0, up]), 3)
    assert r["junctions"][0].tolist() == [2, 0]
    assert r["q"].tolist() == [[0, 0], [1, 0], [2, 0], [2, .5], [2, 1.5], [2, 2.5], [2, 3.5], [2, 4.5]]
    # exit 1: more points behind it, the run starts at N-1 and descends; the last contour's tie (entry 2) runs to N-1
    mid = _line([(1, 2.5), (1, 1.5), (1, .5), (1, 3.5), (1, 4.5)])
    r = R.wall(np.stack([c0, mid]), 3)
    assert r["junctions"][0].tolist() == [1, 2]
    assert r["q"].tolist() == [[4, 0], [3, 0], [2, 0], [1, 0], [1, .5], [1, 3.5], [1, 4.5]]
    # entry 3: more points before it, the last run descends to 0
    low = _line([(1, 4.5), (1, 3.5), (1, 2.5), (1, .5), (1, 1.5)])
    r = R.wall(np.stack([c0, low]), 3)
    assert r["junctions"][0].tolist() == [1, 3]
    assert r["q"].tolist() == [[4, 0], [3, 0], [2, 0], [1, 0], [1, .5], [1, 2.5], [1, 3.5], [1, 4.5]]
    # one contour: the whole of it from 0 to N-1, resampled at equal arc length
    r = R.wall(c0[None], 9)
    assert (r["junctions"] == -1).all() and r["P"] == 5 and r["L"] == 4.0
    assert r["out"].tolist() == [[.5 * m, 0] for m in range(9)]


def test_resampling_of_a_hand_made_wall():
    """An L-shaped wall of length 8 at 5 outputs: one every 2 units, the corner between the second and the third."""
    a = _line([(0, 0), (1, 0), (3, 0), (4, 0)])
    b = _line([(4, 4), (4, 3), (4, 1), (4, 0)])   # stored backwards, and its junction point repeats a's: a segment of zero length
    r = R.wall(np.stack([a, b]), 5)
    assert r["junctions"][0].tolist() == [3, 3] and r["P"] == 8 and r["L"] == 8.0 and r["status"] == 0
    assert r["out"].tolist() == [[0, 0], [2, 0], [4, 0], [4, 2], [4, 4]]


def test_ties_take_the_first_minimum_in_row_major_order():
    rng = np.random.default_rng(3)
    ties = 0
    for _ in range(20):
        a, b = rng.integers(0, 9, (2, 12, 2))
        best = None
        for i in range(12):                  # exact integer arithmetic, strict <: the first minimum
            for j in range(12):
                d = int((a[i, 0] - b[j, 0]) ** 2 + (a[i, 1] - b[j, 1]) ** 2)
                if best is None or d < best[0]:
                    best = (d, i, j)
        d_all = ((a[:, None] - b[None]) ** 2).sum(-1)
        ties += int((d_all == best[0]).sum() > 1)
        assert R.junction(a / 8.0, b / 8.0) == best[1:]
    assert ties >= 10   # the draws do hold equal minima


def test_status_bits():
    still = np.repeat(np.array([[[0.3, 0.6]]], dtype=np.float32), 6, axis=1).repeat(3, axis=0)
    r = R.wall(still, 9)
    assert r["status"] == R.STATUS_ZERO_LENGTH and r["L"] == 0 and r["junctions"][:2].tolist() == [[0, 0], [0, 0]]
    assert np.array_equal(r["out"], np.repeat(still[0, :1].astype(np.float64), 9, axis=0))
    for bad in (np.nan, np.inf, -np.inf):
        chain = R.random_chain(np.random.default_rng(4), 3, 10)
        chain[1, 4, 1] = bad
        r = R.wall(chain, 9)
        assert r["status"] == R.STATUS_NON_FINITE and np.isnan(r["out"]).all() and (r["junctions"] == -1).all()
    from artspeech_amd.phoneme_to_articulation import vocal_tract_tube as V
    assert (V.STATUS_ZERO_LENGTH, V.STATUS_NON_FINITE) == (R.STATUS_ZERO_LENGTH, R.STATUS_NON_FINITE) == (1, 2)


# ---------------------------------------------------------------------------------------------------- the library
def _call(**change):
    from artspeech_amd import _lib
    a = dict(N=50, A=11, k_int=6, k_ext=6, M=100, ld=100, chains=[0, 1, 2, 3, 4, 5, -1, -1, 0, 6, 7, 8, 9, 10, -1, -1], frames=4,
             lengths=None, T=0)
    a.update(change)
    table = (ctypes.c_int32 * 16)(*a["chains"])
    _lib.call("as_vocal_tract_tube", 16, a["A"] * 2 * a["N"], 2 * a["N"], a["N"], 1, a["frames"], a["A"], a["N"], table, a["k_int"],
              a["k_ext"], a["lengths"], a["T"], a["M"], 16, a["ld"], None, None, None, stream=0)


def test_limits_are_refused_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail otherwise (or crash); these return the library's message."""
    bad = [dict(N=1), dict(N=129), dict(k_int=0), dict(k_int=9), dict(k_ext=0), dict(k_ext=9), dict(M=1, ld=100), dict(M=1025, ld=2000),
           dict(ld=99), dict(chains=[0, 1, 2, 3, 4, 11, -1, -1, 0, 6, 7, 8, 9, 10, -1, -1]),
           dict(chains=[0, 1, 2, 3, 4, 5, -1, -1, -1, 6, 7, 8, 9, 10, -1, -1]), dict(frames=-1), dict(lengths=16, T=3)]
    for change in bad:
        with pytest.raises(RuntimeError, match="as_vocal_tract_tube failed"):
            _call(**change)
    with pytest.raises(RuntimeError, match="articulator 11 at position 5 of the internal chain"):
        _call(chains=[0, 1, 2, 3, 4, 11, -1, -1, 0, 6, 7, 8, 9, 10, -1, -1])
    _call(frames=0)                                                   # nothing to do: no launch, no error
    _call(frames=0, chains=[0, 1, 2, 3, 4, 5, 99, 99, 0, 6, 7, 8, 9, 10, 99, 99])   # the unused entries are not looked at


def test_symbol_is_declared_bound_and_built_without_contraction():
    from artspeech_amd import _lib, build
    L = _lib.lib()
    assert "as_vocal_tract_tube" in _lib.PROTOTYPES and hasattr(L, "as_vocal_tract_tube")
    res, args = _lib.PROTOTYPES["as_vocal_tract_tube"]
    assert len(args) == 20 and args[-1] is _lib.Stream and res is _lib.C.c_int32
    assert build.SOURCES["vocal_tract_tube.hip"] == ["-ffp-contract=off"]
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    source = open(os.path.join(build.CSRC, "vocal_tract_tube.hip")).read()
    for text in (header, source):
        for site in ("generate_vocal_tract_shape_v2.py:426", "generate_vocal_tract_shape.py:34", "shape_to_air_column.py:77", "unpinned",
                     "ASSUMPTION"):
            assert site in text, site


def test_chains_and_cpu_tensors():
    from artspeech_amd.phoneme_to_articulation import vocal_tract_tube as V
    assert len(V.INTERNAL_WALL) == len(V.EXTERNAL_WALL) == 6 and V.INTERNAL_WALL[0] == V.EXTERNAL_WALL[0] == "vocal-folds"
    arts = sorted(set(V.INTERNAL_WALL + V.EXTERNAL_WALL) - {"epiglottis", "upper-incisor"})
    assert [arts[i] for i in V.chain_indices(arts, V.INTERNAL_WALL)] == ["vocal-folds", "thyroid-cartilage", "tongue", "lower-incisor",
                                                                         "lower-lip"]
    with pytest.raises(ValueError, match="none of its articulators"):
        V.chain_indices(["tongue", "lower-lip"], V.EXTERNAL_WALL, "external")
    with pytest.raises(RuntimeError, match="MI355X"):
        V.vocal_tract_tube(torch.zeros(3, len(arts), 2, 50), arts)


# ---------------------------------------------------------------------------------------------------- the data set
TEN = ("arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline", "thyroid-cartilage",
       "tongue", "upper-lip", "vocal-folds")


def _write_sequence(root, subject, name, tokens, n_frames, rng, articulators=TEN, n=5, n_wall=7, air=True):
    seq = root / subject / name
    (seq / "inference_contours").mkdir(parents=True)
    (seq / "air_column").mkdir()
    (seq / "target_sequence.txt").write_text(" ".join(tokens))
    airs, shapes = [], []
    for t in range(1, n_frames + 1):
        frame = rng.random((len(articulators), 2, n)).astype(np.float32)
        for a, c in zip(articulators, frame):
            np.save(seq / "inference_contours" / f"{'%04d' % t}_{a}.npy", c)
        shapes.append(frame)
        if air:
            airs.append(rng.random((2, 2, n_wall)))
            np.save(seq / "air_column" / f"{'%04d' % t}.npy", airs[-1])
    return np.array(airs), np.array(shapes)


def test_shape_tree_dataset_items(tmp_path, caplog):
    from artspeech_amd.phoneme_recognition.datasets import ShapeTreeRecognitionDataset
    rng = np.random.default_rng(0)
    vocabulary = {"<blank>": 0, "<unk>": 1, "a": 2, "b": 3, "c": 4}
    tokens = ["a", "a", "b", "zz", "zz", "a"]
    airs, shapes = _write_sequence(tmp_path, "S1", "one", tokens, 6, rng, articulators=TEN + ("upper-incisor",))
    _write_sequence(tmp_path, "S1", "two", ["a"], 1, rng, air=False)       # no air column: skipped
    _write_sequence(tmp_path, "S1", "three", ["c", "b"], 2, rng)
    with caplog.at_level("WARNING"):
        ds = ShapeTreeRecognitionDataset("artspeech2", str(tmp_path), vocabulary, [("S1", "one"), ("S1", "two"), ("S1", "three")], ["a"])
    assert len(ds) == 2 and "Skipping S1/two" in caplog.text
    assert ds.articulators == sorted(TEN) and ds.database_config.RES == 136
    item = ds[0]
    assert list(item) == ["air_column", "air_column_length", "vocal_tract", "vocal_tract_length", "articulatory_target",
                          "articulatory_target_length", "voicing", "ctc_target", "ctc_target_length"]
    assert item["air_column"].shape == (2, 2 * 7, 6) and item["air_column"].dtype == torch.float32
    assert item["vocal_tract"].shape == (2, 10 * 5, 6) and item["vocal_tract"].dtype == torch.float32
    # air_column[c, w * Nw + i, t] = file t [w, c, i]; vocal_tract[c, a * N + i, t] = contour of sorted articulator a, frame t
    want_air = torch.from_numpy(airs).float().permute(2, 1, 3, 0).reshape(2, 14, 6)
    order = [list(TEN + ("upper-incisor",)).index(a) for a in sorted(TEN)]
    want_vt = torch.from_numpy(shapes[:, order]).permute(2, 1, 3, 0).reshape(2, 50, 6)
    assert torch.equal(item["air_column"], want_air) and torch.equal(item["vocal_tract"], want_vt)
    assert item["air_column"][1, 7 + 3, 4] == np.float32(airs[4, 1, 1, 3])
    assert item["articulatory_target"].tolist() == [2, 2, 3, 0, 0, 2] and item["articulatory_target"].dtype == torch.long
    assert item["ctc_target"].tolist() == [2, 3, 0, 2] and item["ctc_target_length"] == 4
    assert item["voicing"].tolist() == [1, 1, 0, 0, 0, 1] and item["voicing"].dtype == torch.float32
    assert (item["air_column_length"], item["vocal_tract_length"], item["articulatory_target_length"]) == (6, 6, 6)
    assert ds[1]["ctc_target"].tolist() == [4, 3]


def test_recogniser_scripts_select_the_shape_tree(tmp_path):
    import inspect
    import yaml
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition import Feature
    from artspeech_amd.phoneme_recognition.datasets import ShapeTreeRecognitionDataset
    _write_sequence(tmp_path, "S1", "one", ["a", "b"], 2, np.random.default_rng(1))
    ds = T._make_dataset(str(tmp_path), "artspeech2", {"S1": []}, {"a": 2, "b": 3}, Feature.AIR_COLUMN, None, None, 0, dataset="shape_tree")
    assert isinstance(ds, ShapeTreeRecognitionDataset) and len(ds) == 1
    with pytest.raises(ValueError, match="shape_tree"):
        T._make_dataset(str(tmp_path), "artspeech2", {"S1": []}, {}, Feature.AIR_COLUMN, None, None, 0, dataset="other")
    assert "dataset" in inspect.signature(T.main).parameters
    # test_phoneme_recognition.py has no such keyword and is left as it is: its configs say synthetic: {dataset: shape_tree}
    ds = T._make_dataset(str(tmp_path), "artspeech2", {"S1": []}, {"a": 2, "b": 3}, Feature.AIR_COLUMN, ["a"], {"dataset": "shape_tree"}, 2)
    assert isinstance(ds, ShapeTreeRecognitionDataset) and len(ds) == 1 and ds.voiced_tokens == ["a"]
    with pytest.raises(ValueError, match="disagree"):
        T._make_dataset(str(tmp_path), "artspeech2", {"S1": []}, {}, Feature.AIR_COLUMN, None, {"dataset": "other"}, 0, dataset="shape_tree")
    with open(os.path.join(ROOT, "configs", "train_recognizer_shape_tree_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(T.main).parameters) and cfg["dataset"] == "shape_tree" and cfg["feature"] == "air_column"
    with open(os.path.join(ROOT, "configs", "generate_vocal_tract_shape_air_column_synthetic.yaml")) as f:
        gen = yaml.safe_load(f)
    assert os.path.dirname(gen["save_to"]) == cfg["datadir"] and list(cfg["train_seq_dict"]) == [os.path.basename(gen["save_to"])]
    assert cfg["model_params"]["num_features"] == 2 * gen["n_wall"]


# ---------------------------------------------------------------------------------------------------- the scripts
def test_generate_config_is_the_autoencoder_config_with_air_columns():
    import inspect
    import yaml
    import generate_vocal_tract_shape as S
    with open(os.path.join(ROOT, "configs", "generate_vocal_tract_shape_air_column_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", "generate_vocal_tract_shape_synthetic.yaml")) as f:
        base = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(S.main).parameters)
    assert cfg["air_column"] is True and cfg["method"] == "autoencoder"
    same = set(base) - {"save_to", "synthetic"}
    assert {k: cfg[k] for k in same} == {k: base[k] for k in same}
    defaults = inspect.signature(S.main).parameters
    assert defaults["air_column"].default is False and defaults["n_wall"].default == 100
    from artspeech_amd.phoneme_to_articulation import synthesis
    for fn in (synthesis.synthesize, synthesis.save_sentence):
        p = inspect.signature(fn).parameters
        assert p["air_column"].default is False and p["n_wall"].default == 100


def test_shape_to_air_column_selects_frames_and_honours_overwrite(tmp_path, monkeypatch):
    import inspect
    import yaml
    import shape_to_air_column as S
    assert not S.__name__.startswith(("train_", "test_"))
    internal, external = ["vocal-folds", "tongue", "lower-lip"], ["vocal-folds", "pharynx", "upper-lip"]
    needed = sorted(set(internal) | set(external))
    rng = np.random.default_rng(5)
    seq = tmp_path / "S1" / "one"
    (seq / "inference_contours").mkdir(parents=True)
    (tmp_path / "S1" / "no_contours").mkdir()
    frames = {}
    for frame_id in ("0001", "0002", "0003"):
        frames[frame_id] = R.random_frames(rng, 1, 6, 8)[0] * 136
        for a, c in zip(needed + ["epiglottis"], frames[frame_id]):
            if frame_id == "0002" and a == "pharynx":
                continue                                   # frame 0002 lacks an articulator of the external chain
            np.save(seq / "inference_contours" / f"{frame_id}_{a}.npy", c.T if a == "tongue" else c)   # (N, 2) files are read too
    (seq / "air_column").mkdir()
    np.save(seq / "air_column" / "0003.npy", np.full((2, 2, 9), 7.5))
    launches = []

    def restated(contours, articulators, internal, external, n_wall):
        launches.append(contours.shape)
        return R.tube(contours, [articulators.index(a) for a in internal], [articulators.index(a) for a in external], n_wall)[0]
    monkeypatch.setattr(S, "build_walls", restated)
    table = S.frame_table(str(seq / "inference_contours"))
    assert sorted(table) == ["0001", "0002", "0003"] and "pharynx" not in table["0002"] and "epiglottis" in table["0001"]
    assert S.select_frames(table, needed, str(seq / "air_column"), overwrite=True) == ["0001", "0003"]
    assert S.select_frames(table, needed, str(seq / "air_column"), overwrite=False) == ["0001"]
    info = S.main(str(tmp_path), "artspeech2", overwrite=False, n_wall=9, internal=internal, external=external)
    assert info["written"] == 1 and launches == [(1, 5, 2, 8)]                        # one launch for the sequence
    assert sorted(os.listdir(seq / "air_column")) == ["0001.npy", "0003.npy"]
    assert (np.load(seq / "air_column" / "0003.npy") == 7.5).all()                    # left alone
    idx = [[needed.index(a) for a in chain] for chain in (internal, external)]
    want = R.tube((frames["0001"][:5] / np.float32(136))[None], idx[0], idx[1], 9)[0][0]
    got = np.load(seq / "air_column" / "0001.npy")
    assert got.shape == (2, 2, 9) and got.dtype == np.float64 and np.array_equal(got, want)
    info = S.main(str(tmp_path), "artspeech2", overwrite=True, n_wall=9, internal=internal, external=external)
    assert info["written"] == 2 and launches[-1] == (2, 5, 2, 8)
    assert np.load(seq / "air_column" / "0003.npy").shape == (2, 2, 9) and not (np.load(seq / "air_column" / "0003.npy") == 7.5).any()
    assert not os.path.exists(seq / "air_column" / "0002.npy")
    with open(os.path.join(ROOT, "configs", "shape_to_air_column_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(S.main).parameters)
    with open(os.path.join(ROOT, "configs", "generate_vocal_tract_shape_air_column_synthetic.yaml")) as f:
        gen = yaml.safe_load(f)
    assert cfg["datadir"] == os.path.dirname(gen["save_to"]) and set(cfg["internal"]) | set(cfg["external"]) <= set(gen["articulators"])
