"""CPU tests of the phoneme-wise mean contour's host side (artspeech_amd/phoneme_to_articulation/phoneme_wise_mean_contour): the
per-token sampler against the indices pandas drew (tests/golden/mean_contour.npz, written by the reference's own functions), the
float64 yardstick tests/mean_contour_fp64.py against the same fixture, the table file, the C-ABI surface and the entry points."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT, load_golden
from mean_contour_fp64 import MeanContourYardstick, mean_euclidean, run_positions, sample

SYMBOLS = ("as_token_runs_workspace_ints", "as_token_runs", "as_mean_contour_fit", "as_mean_contour_fwd", "as_mean_contour_weighted_fwd")


def _splits():
    """the fixture and the data sets it was made from: (fixture, config, train tokens, first rows, lengths, train contours, test set)"""
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import SyntheticSegmentedArtSpeechDataset
    g = load_golden("mean_contour")
    cfg = json.loads(str(g["config"]))
    train = SyntheticSegmentedArtSpeechDataset(vocabulary=cfg["vocabulary"], articulators=cfg["articulators"], **cfg["train"])
    test = SyntheticSegmentedArtSpeechDataset(vocabulary=cfg["vocabulary"], articulators=cfg["articulators"], **cfg["test"])
    items = [train[i] for i in range(len(train))]
    lengths = [len(item[1]) for item in items]
    first = np.cumsum([0] + lengths)[:-1]
    return (g, cfg, np.concatenate([item[1].numpy() for item in items]), first, lengths,
            np.concatenate([item[2].numpy() for item in items]), test)


def test_host_sampler_equals_the_pandas_indices():
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import sample_rows
    g, cfg, tokens, *_ = _splits()
    assert np.array_equal(tokens, g["train.token"])          # the data set regenerates from its constructor arguments
    V = len(cfg["vocabulary"])
    rows, offsets = sample_rows(tokens, V, 0.1, 0, sort=False)
    ascending, offsets2 = sample_rows(tokens, V, 0.1, 0)
    assert np.array_equal(offsets, offsets2) and offsets[-1] == len(rows)
    sizes = []
    for v in range(V):
        got = rows[offsets[v]:offsets[v + 1]]
        want = g[f"sample.{v}"] if f"sample.{v}" in g else np.zeros(0, np.int64)
        assert np.array_equal(got, want), v                  # pandas' rows in pandas' order
        assert np.array_equal(ascending[offsets[v]:offsets[v + 1]], np.sort(want)), v
        assert np.array_equal(sample(tokens, v), want), v    # the yardstick's sampler too
        sizes.append(len(want))
    assert 1 in sizes and max(sizes) > 20                    # the fixture holds a one-row sample and large ones
    every, offsets = sample_rows(tokens, V, 1.0, 0)          # frac = 1 keeps every frame, in table order inside a token
    assert len(every) == len(tokens) and all(np.array_equal(every[offsets[v]:offsets[v + 1]], np.flatnonzero(tokens == v)) for v in range(V))


def test_yardstick_reproduces_the_fixture():
    """Positions exactly; the weighted output (float64 in the reference) to 1e-12.  The reference's unweighted output is a float32
    mean of float32 contours in [0, 1.3]: a sequential fp32 sum of n <= 47 terms is within n * 2^-24 * max|x| = 3.7e-6 of the
    exact mean, the bound used for it (observed 1.0e-7)."""
    g, cfg, tokens, first, lengths, contours, test = _splits()
    abs_pos, seq_len, rel_pos = run_positions(tokens, first, lengths)
    assert np.array_equal(abs_pos, g["train.abs_pos"]) and np.array_equal(seq_len, g["train.seq_len"])
    assert np.array_equal(rel_pos, g["train.rel_pos"])
    assert (seq_len == 1).any() and (seq_len >= 25).any()
    y = MeanContourYardstick().fit(tokens, rel_pos, contours)
    for s in range(len(test)):
        sentence = test[s][1].numpy()
        weighted, plain = y.forward_weighted(sentence), y.forward(sentence)
        assert g[f"weighted.out.{s}"].dtype == np.float64 and g[f"unweighted.out.{s}"].dtype == np.float32
        assert np.abs(weighted - g[f"weighted.out.{s}"]).max() <= 1e-12
        assert np.abs(plain - g[f"unweighted.out.{s}"]).max() <= 47 * 2.0 ** -24 * 1.3
        assert abs(mean_euclidean(weighted, test[s][2].numpy()) - g["weighted.losses"][s]) <= 1e-12
        assert abs(mean_euclidean(plain, test[s][2].numpy()) - g["unweighted.losses"][s]) <= 1e-7
    assert g["unweighted.reference_seconds_per_frame"] > 0 and g["weighted.reference_seconds_per_frame"] > 0


def test_weighted_method_is_better_on_the_segmented_synthetic_data():
    """a property of SyntheticSegmentedArtSpeechDataset (a smooth trajectory in rel_pos), shown on the yardstick"""
    g, cfg, tokens, first, lengths, contours, test = _splits()
    y = MeanContourYardstick().fit(tokens, run_positions(tokens, first, lengths)[2], contours)
    plain = np.mean([mean_euclidean(y.forward(test[s][1].numpy()), test[s][2].numpy()) for s in range(len(test))])
    weighted = np.mean([mean_euclidean(y.forward_weighted(test[s][1].numpy()), test[s][2].numpy()) for s in range(len(test))])
    assert weighted < 0.95 * plain, (weighted, plain)
    assert g["weighted.info.loss"] < 0.95 * g["unweighted.info.loss"]    # and in the reference's own numbers


def test_segmented_synthetic_dataset_items():
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import SyntheticSegmentedArtSpeechDataset
    voc = {"<blank>": 0, "<unk>": 1, "a": 2, "b": 3, "c": 4}
    ds = SyntheticSegmentedArtSpeechDataset(4, voc, ["tongue", "lower-lip"], n_samples=7, min_len=30, max_len=60, max_duration=9, seed=3)
    assert ds.articulators == ["lower-lip", "tongue"] and len(ds) == 4
    item = ds[1]
    length = len(item[1])
    assert len(item) == 8 and item[1].dtype == torch.long and item[2].shape == (length, 2, 2, 7) and item[2].dtype == torch.float32
    assert 30 <= length <= 60 and item[1].min() >= 2 and item[3] == [{v: k for k, v in voc.items()}[int(i)] for i in item[1]]
    assert item[4].shape == (length, 1, 2, 7) and len(item[6]) == length and item[7].shape == (length,)
    assert torch.equal(ds[1][2], item[2]) and torch.equal(ds[1][1], item[1])        # deterministic
    seq_len = run_positions(item[1].numpy())[1]
    assert seq_len.max() <= 9 and seq_len.max() > 1                                   # runs, bounded by max_duration
    other = SyntheticSegmentedArtSpeechDataset(4, voc, ["tongue", "lower-lip"], n_samples=7, min_len=30, max_len=60, seed=4)
    assert torch.equal(other._shape, ds._shape)                                       # the splits share the token shapes


def test_table_file_reads_the_reference_layout_and_round_trips(tmp_path):
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import read_table, write_table
    g = load_golden("mean_contour")
    path = os.path.join(GOLDEN, "mean_contour_table.csv")            # written by pandas from the reference's rows
    data = read_table(path)
    assert data["tokens"] == [str(t) for t in g["table.token"]]
    assert np.array_equal(data["positions"][:, 0], g["table.abs_pos"]) and np.array_equal(data["positions"][:, 1], g["table.seq_len"])
    assert data["contours"].dtype == np.float32 and np.array_equal(data["contours"], g["table.contours"])
    assert data["articulators"] == json.loads(str(g["config"]))["articulators"]
    again = write_table(str(tmp_path / "table.csv"), data["tokens"], data["positions"], data["contours"], data["articulators"])
    assert open(again).read() == open(path).read()                    # the very bytes pandas wrote
    back = read_table(again)
    assert back["tokens"] == data["tokens"] and np.array_equal(back["contours"], data["contours"])
    plain = write_table(str(tmp_path / "plain.csv"), data["tokens"], None, data["contours"], data["articulators"])
    back = read_table(plain)                                          # the unweighted method's table: no position columns
    assert back["positions"] is None and np.array_equal(back["contours"], data["contours"])
    assert open(plain).readline().strip() == "token," + ",".join(data["articulators"])
    import pandas as pd
    df = pd.read_csv(plain)                                           # and pandas reads ours
    assert list(df.token) == data["tokens"] and json.loads(df[data["articulators"][0]][3]) == data["contours"][3, 0].tolist()
    (tmp_path / "bad.csv").write_text("phoneme,tongue\na,\"[[0.0], [1.0]]\"\n")
    with pytest.raises(ValueError, match="token"):
        read_table(str(tmp_path / "bad.csv"))


def test_new_symbols_are_declared_exported_and_bound():
    from artspeech_amd import _lib
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    declared = set(re.findall(r"\b(as_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name), f"{name} is not bound / exported"
    assert L.as_token_runs_workspace_ints(1) == 4 and L.as_token_runs_workspace_ints(1025) == 8 and L.as_token_runs_workspace_ints(0) == 0
    assert re.search(r"phoneme_wise_mean_contour/__init__\.py", header)      # the prototypes cite their reference call sites


def test_entry_points_parse_their_configs():
    import test_phoneme_wise_mean_contour as tester
    import train_phoneme_wise_mean_contour as trainer
    for module, name in ((trainer, "train_mean_contour_synthetic.yaml"), (tester, "test_mean_contour_synthetic.yaml")):
        path = os.path.join(ROOT, "configs", name)
        assert module.parse_args(["--config", path]).config_filepath == path
        with open(path) as f:
            cfg = yaml.safe_load(f)
        bound = inspect.signature(module.main).bind(**cfg)                   # every key is an argument of main()
        assert bound.arguments["datadir"] == "synthetic" and bound.arguments["weighted"] is True
    args = trainer.parse_args(["--config", "c.yaml", "--mlflow", "uri", "--experiment", "e", "--run_id", "r", "--run_name", "n"])
    assert (args.mlflow_tracking_uri, args.experiment_name, args.run_id, args.run_name) == ("uri", "e", "r", "n")
    reference_keys = {"database_name", "datadir", "train_seq_dict", "test_seq_dict", "vocab_filepath", "articulators",
                      "state_dict_filepath", "clip_tails", "weighted"}
    assert reference_keys <= set(inspect.signature(trainer.main).parameters)
    assert {"seq_dict", "state_dict_filepath", "save_to", "weighted"} <= set(inspect.signature(tester.main).parameters)
    voc = trainer.build_vocabulary(None)
    assert len(voc) == 45 and voc["<unk>"] == 1


def test_empty_sample_is_an_error_naming_the_token():
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import require_bank, sample_rows
    voc = {"<blank>": 0, "<unk>": 1, "a": 2, "rare": 3, "never": 4}
    tokens = np.array([2] * 40 + [3] * 5)                    # round(0.1 * 5) = 0: an empty sample; 'never' is absent
    rows, offsets = sample_rows(tokens, len(voc), 0.1, 0)
    assert offsets[3] - offsets[2] == 4 and offsets[4] == offsets[3]
    require_bank(offsets, [2, 2, 2], voc)
    with pytest.raises(IndexError, match=r"'rare' \(id 3\)"):
        require_bank(offsets, [2, 3, 2], voc)
    with pytest.raises(IndexError, match=r"'never' \(id 4\).*id 9"):
        require_bank(offsets, [4, 9], voc)
    with pytest.raises(IndexError, match="id -1"):
        require_bank(offsets, [-1], voc)
