"""Writes tests/golden/mean_contour.npz and tests/golden/mean_contour_table.csv with the REFERENCE's code: the functions of
phoneme_to_articulation/phoneme_wise_mean_contour/__init__.py, taken from the file with ``ast`` and run unmodified on seeded
``SyntheticSegmentedArtSpeechDataset`` splits, and the reference's own metric functions.  Runs only where the reference checkout and
pandas are installed; the tests read the fixtures, never the reference.

    python tests/golden/make_golden_mean_contour.py [reference root]

``forward_weighted_mean_contour`` does not run as committed: its ``functools.reduce(`` call (:89-95) lost the function argument that
its twin in ``process_sentence_with_pos`` (:36-42) still has.  It is run unmodified with the name ``functools`` in its scope bound to
a shim whose one-argument ``reduce(seq)`` concatenates the lists and whose other forms forward to the real one.

The data sets are not stored: the tests regenerate them from the stored constructor arguments.  Stored: the reference's run positions
per train frame, ``df.sample(frac=0.1, random_state=0).index`` per token, both forwards of every test sentence (the weighted one is
float64, as the reference returns it), the per-sentence metrics computed the way ``test()`` (:180-186) computes them, their means
(the info dict), and the reference's wall time per output frame (information only).  For the weighted method the targets are cast
to the outputs' float64 before the metrics (``torch.cdist`` refuses mixed dtypes).  The small table file is the reference's
``pd.DataFrame(data).to_csv(index=False)`` (:155-157) of a third, tiny split.
"""
import ast
import functools
import json
import os
import sys
import time
import types
from itertools import groupby

import numpy as np
import pandas as pd
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import SyntheticSegmentedArtSpeechDataset  # noqa: E402

ARTICULATORS = ["lower-lip", "tongue", "upper-lip"]
VOCABULARY = {t: i for i, t in enumerate(["<blank>", "<unk>", "a", "e", "i", "o", "u", "s", "t", "k"])}
TRAIN = dict(num_sentences=12, n_samples=50, min_len=120, max_len=120, max_duration=30, token_skew=0.55)
TEST = dict(num_sentences=3, n_samples=50, min_len=10, max_len=20, max_duration=12, token_skew=0.3)
TABLE = dict(num_sentences=2, n_samples=20, min_len=25, max_len=30, max_duration=8, seed=5)
FUNCTIONS = ("_calculate_tokens_lengths_and_positions", "process_sentence_with_pos", "process_sentence",
             "forward_weighted_mean_contour", "forward_mean_contour")


def reference_functions(reference_root):
    """the reference's functions, taken from the file without running the module's imports (funcy, vt_tools, tqdm are absent)"""
    path = os.path.join(reference_root, "phoneme_to_articulation", "phoneme_wise_mean_contour", "__init__.py")
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    shim = types.SimpleNamespace(reduce=lambda *args: functools.reduce(lambda l1, l2: l1 + l2, args[0]) if len(args) == 1
                                 else functools.reduce(*args))
    scope = {"functools": shim, "groupby": groupby, "torch": torch, "F": F, "pd": pd, "np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), scope)
    return {name: scope[name] for name in FUNCTIONS}


def reference_metrics(reference_root):
    from make_golden import _load, install_shims
    install_shims()
    pkg = types.ModuleType("phoneme_to_articulation")
    pkg.__path__ = [os.path.join(reference_root, "phoneme_to_articulation")]
    sys.modules["phoneme_to_articulation"] = pkg
    p2a = _load("phoneme_to_articulation.metrics", "phoneme_to_articulation/metrics.py")
    root = _load("ref_root_metrics", "metrics.py")
    return p2a.EuclideanDistance, root


def table_of(fn, dataset):
    return pd.DataFrame([row for sentence in dataset for row in fn(sentence, articulators=dataset.articulators)])


def conditions(train_df, test_sets):
    """the conditions on the inputs; returns None or the reason they fail"""
    counts = train_df.token.value_counts()
    test_tokens = {t for ds in test_sets for s in ds for t in s[3]}
    if any(counts.get(t, 0) < 6 for t in test_tokens):
        return "a test token has fewer than 6 train rows"
    if not any(6 <= counts.get(t, 0) <= 14 for t in test_tokens):
        return "no test token with 6..14 train rows (a sample of exactly one row)"
    if not (train_df.seq_len == 1).any():
        return "no run of length 1"
    if not (train_df.seq_len >= 25).any():
        return "no run of length >= 25"
    return None


def main(reference_root):
    ref = reference_functions(reference_root)
    EuclideanDistance, root_metrics = reference_metrics(reference_root)
    for seed in range(400):   # the first seed whose splits satisfy the conditions
        train_set = SyntheticSegmentedArtSpeechDataset(vocabulary=VOCABULARY, articulators=ARTICULATORS, seed=seed, **TRAIN)
        test_set = SyntheticSegmentedArtSpeechDataset(vocabulary=VOCABULARY, articulators=ARTICULATORS, seed=seed + 1000, **TEST)
        train_df = table_of(ref["process_sentence_with_pos"], train_set)
        why = conditions(train_df, [test_set])
        if why is None:
            break
    else:
        raise SystemExit(f"no seed satisfies the conditions: {why}")
    assert conditions(train_df, [test_set]) is None
    plain_df = table_of(ref["process_sentence"], train_set)
    assert list(plain_df.token) == list(train_df.token)

    out = {"config": np.array(json.dumps({"vocabulary": VOCABULARY, "articulators": ARTICULATORS, "train": dict(TRAIN, seed=seed),
                                          "test": dict(TEST, seed=seed + 1000), "table": TABLE})),
           "train.token": np.array([VOCABULARY[t] for t in train_df.token], np.int64),
           "train.abs_pos": train_df.abs_pos.to_numpy(np.int64), "train.seq_len": train_df.seq_len.to_numpy(np.int64),
           "train.rel_pos": train_df.rel_pos.to_numpy(np.float64)}
    for token in sorted(set(train_df.token)):
        out[f"sample.{VOCABULARY[token]}"] = train_df[train_df.token == token].sample(frac=0.1, random_state=0).index.to_numpy(np.int64)

    criterion = EuclideanDistance()
    for tag, fn, df in (("unweighted", ref["forward_mean_contour"], plain_df), ("weighted", ref["forward_weighted_mean_contour"], train_df)):
        losses, x_corrs, y_corrs, seconds, frames = [], [], [], 0.0, 0
        for s, (_, _, sentence_targets, sentence_tokens, _, _, _, _) in enumerate(test_set):
            t0 = time.perf_counter()
            sentence_outputs = fn(sentence_tokens, df, test_set.articulators)
            seconds += time.perf_counter() - t0
            frames += len(sentence_tokens)
            out[f"{tag}.out.{s}"] = sentence_outputs.numpy()
            sentence_outputs = sentence_outputs.unsqueeze(dim=0)
            sentence_targets = sentence_targets.unsqueeze(dim=0).to(sentence_outputs.dtype)
            loss = criterion(sentence_outputs, sentence_targets)
            p2cp = root_metrics.p2cp_distance(sentence_outputs, sentence_targets).mean(dim=1)
            euclidean = root_metrics.euclidean_distance(sentence_outputs, sentence_targets).mean(dim=1)
            x_corr, y_corr = root_metrics.pearsons_correlation(sentence_outputs, sentence_targets)
            x_corr, y_corr = x_corr.mean(dim=-1)[0], y_corr.mean(dim=-1)[0]
            losses.append(loss.item())
            x_corrs.append(x_corr.numpy())
            y_corrs.append(y_corr.numpy())
            out[f"{tag}.p2cp.{s}"], out[f"{tag}.euclidean.{s}"] = p2cp[0].numpy(), euclidean[0].numpy()
        out[f"{tag}.losses"] = np.array(losses, np.float64)
        out[f"{tag}.x_corrs"], out[f"{tag}.y_corrs"] = np.array(x_corrs, np.float64), np.array(y_corrs, np.float64)
        out[f"{tag}.info.loss"] = np.float64(np.mean(losses))
        out[f"{tag}.info.x_corr"], out[f"{tag}.info.y_corr"] = np.mean(x_corrs, axis=0), np.mean(y_corrs, axis=0)
        out[f"{tag}.reference_seconds_per_frame"] = np.float64(seconds / frames)
    assert out["unweighted.out.0"].dtype == np.float32 and out["weighted.out.0"].dtype == np.float64

    table_set = SyntheticSegmentedArtSpeechDataset(vocabulary=VOCABULARY, articulators=ARTICULATORS, **TABLE)
    table_df = table_of(ref["process_sentence_with_pos"], table_set)
    table_path = os.path.join(HERE, "mean_contour_table.csv")
    table_df.to_csv(table_path, index=False)
    out["table.token"] = np.array(list(table_df.token))
    out["table.abs_pos"], out["table.seq_len"] = table_df.abs_pos.to_numpy(np.int64), table_df.seq_len.to_numpy(np.int64)
    out["table.rel_pos"] = table_df.rel_pos.to_numpy(np.float64)
    out["table.contours"] = np.array([[row[a] for a in table_set.articulators] for _, row in table_df.iterrows()], np.float32)

    path = os.path.join(HERE, "mean_contour.npz")
    np.savez_compressed(path, **out)
    total = os.path.getsize(path) + os.path.getsize(table_path)
    print(path, table_path, total, "bytes; seed", seed, "; reference s/frame",
          float(out["unweighted.reference_seconds_per_frame"]), float(out["weighted.reference_seconds_per_frame"]))
    assert total < 1_000_000


if __name__ == "__main__":
    from make_golden import REF  # noqa: E402  (the reference checkout the other fixture writers use)
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
