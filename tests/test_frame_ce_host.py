"""Host-side pieces of the frame-level criterion and metrics (no GPU): the restatements of tests/frame_ce_fp64.py against
scikit-learn, the divisions of metrics.py against the restatements, the class-weight order, the refusals that come before any
device call, and the new entry script's config contract."""
import inspect
import json
import os

import numpy as np
import pytest
import torch
import yaml

import frame_ce_fp64 as F
from conftest import ROOT

AVERAGES = ("macro", "micro", "weighted", "none", None)


def tied_case(seed, N, C, absent=()):
    """Scores on the grid k / 64 in [0, 1] (heavy ties) and labels that never take the classes in ``absent``."""
    rng = np.random.default_rng(seed)
    scores = (rng.integers(0, 65, size=(N, C)) / 64.0).astype(np.float32)
    present = [c for c in range(C) if c not in absent]
    return scores, rng.choice(present, size=N)


@pytest.mark.parametrize("N,C", [(2, 2), (37, 3), (300, 5)])
def test_auroc_restatement_is_sklearns_per_class(N, C):
    from sklearn.metrics import roc_auc_score
    from artspeech_amd.phoneme_recognition.metrics import auroc_from_counts
    scores, labels = tied_case(N, N, C)
    labels[:C] = np.arange(C)[:N]   # every class present where N allows
    n_pos, n_neg, u2 = F.auroc_counts(scores, labels)
    per = F.auroc(n_pos, n_neg, u2, "none")
    for c in range(C):
        if n_pos[c] and n_neg[c]:
            assert abs(per[c] - roc_auc_score(labels == c, scores[:, c])) <= 1e-12, c
        else:
            assert np.isnan(per[c])
    mine = auroc_from_counts(n_pos, n_neg, u2, "none")
    assert np.array_equal(mine, per, equal_nan=True)
    for average in ("macro", "weighted"):
        assert auroc_from_counts(n_pos, n_neg, u2, average) == pytest.approx(F.auroc(n_pos, n_neg, u2, average), abs=1e-15)


def test_auroc_degenerate_classes_are_nan_and_left_out():
    from artspeech_amd.phoneme_recognition.metrics import auroc_from_counts
    scores, labels = tied_case(5, 40, 4, absent=(2,))
    n_pos, n_neg, u2 = F.auroc_counts(scores, labels)
    assert n_pos[2] == 0 and u2[2] == 0
    per = auroc_from_counts(n_pos, n_neg, u2, None)
    assert np.isnan(per[2]) and not np.isnan(np.delete(per, 2)).any()
    assert auroc_from_counts(n_pos, n_neg, u2, "macro") == pytest.approx(float(np.delete(per, 2).mean()), abs=1e-15)
    one = F.auroc_counts(np.full((7, 1), 0.5, np.float32), np.zeros(7, dtype=np.int64))   # C = 1: no negatives
    assert one[0][0] == 7 and one[1][0] == 0 and np.isnan(auroc_from_counts(*one, "macro"))
    flat = F.auroc_counts(np.full((6, 2), 0.25, np.float32), np.array([0, 1, 0, 1, 1, 1]))   # all scores equal: 0.5
    assert auroc_from_counts(*flat, "none").tolist() == [0.5, 0.5]
    with pytest.raises(ValueError):
        auroc_from_counts(*flat, "micro")


@pytest.mark.parametrize("absent", [(), (1, 3)])
def test_accuracy_and_f1_are_sklearns_over_the_present_classes(absent):
    from sklearn.metrics import f1_score, recall_score
    from artspeech_amd.phoneme_recognition.metrics import accuracy_from_counts, f1_from_counts
    C = 6
    scores, labels = tied_case(11, 200, C, absent)
    scores[:, list(absent)] = -1.0   # never predicted either
    pred = scores.argmax(axis=1)
    cm = F.confusion(pred, labels, C)
    present = sorted(set(labels.tolist()) | set(pred.tolist()))
    assert len(present) == C - len(absent)
    for average in ("macro", "micro", "weighted"):
        want_acc = recall_score(labels, pred, labels=present, average=average, zero_division=0)
        want_f1 = f1_score(labels, pred, labels=present, average=average, zero_division=0)
        assert F.accuracy(cm, average) == pytest.approx(want_acc, abs=1e-12), average
        assert F.f1(cm, average) == pytest.approx(want_f1, abs=1e-12), average
    per_acc = recall_score(labels, pred, labels=list(range(C)), average=None, zero_division=0)
    per_f1 = f1_score(labels, pred, labels=list(range(C)), average=None, zero_division=0)
    assert np.allclose(F.accuracy(cm, "none"), per_acc, atol=1e-12) and np.allclose(F.f1(cm, None), per_f1, atol=1e-12)
    assert all(F.accuracy(cm, "none")[c] == 0 and F.f1(cm, "none")[c] == 0 for c in absent)
    for average in AVERAGES:
        assert np.array_equal(np.asarray(accuracy_from_counts(cm, average)), np.asarray(F.accuracy(cm, average))), average
        assert np.array_equal(np.asarray(f1_from_counts(cm, average)), np.asarray(F.f1(cm, average))), average
    with pytest.raises(ValueError):
        accuracy_from_counts(cm, "samples")


def test_class_weights_are_sorted_by_token_name_with_one_first(tmp_path):
    from artspeech_amd.phoneme_recognition import CrossEntropyLoss
    weights = {"z": 3.0, "a": 0.5, "m": 2.0}   # insertion order differs from name order
    want = [1.0, 0.5, 2.0, 3.0]
    assert CrossEntropyLoss(class_weights=weights).weight.tolist() == want
    path = tmp_path / "w.json"
    path.write_text(json.dumps(weights))
    ce = CrossEntropyLoss(class_weights=str(path), ignore_index=-1, label_smoothing=0.1, reduction="sum")
    assert ce.weight.tolist() == want and ce.weight.dtype == torch.float32
    assert (ce.ignore_index, ce.label_smoothing, ce.reduction) == (-1, 0.1, "sum")
    plain = CrossEntropyLoss()
    assert plain.weight is None and (plain.ignore_index, plain.label_smoothing, plain.reduction) == (-100, 0.0, "mean")
    assert CrossEntropyLoss(torch.tensor([1.0, 2.0])).weight.tolist() == [1.0, 2.0]   # nn.CrossEntropyLoss's first positional
    with pytest.raises(TypeError, match="weight"):
        CrossEntropyLoss(class_weights=weights, weight=torch.ones(4))


def test_refusals_come_before_any_device_call():
    """CPU tensors throughout: a device call would raise RuntimeError (no CPU path), so these errors were raised ahead of it."""
    from artspeech_amd.phoneme_recognition import CrossEntropyLoss, frame_cross_entropy
    x = torch.randn(5, 3, 4)
    tg = torch.zeros(3, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="utterance 1 has 4 frames and 3 target"):
        frame_cross_entropy(x, tg, [5, 4, 2], [5, 3, 1])
    with pytest.raises(ValueError, match="utterance 2"):
        CrossEntropyLoss()(x, tg, torch.tensor([5, 4, 2]), torch.tensor([5, 4, 5]))
    with pytest.raises(NotImplementedError, match="none"):
        frame_cross_entropy(x, tg, [5, 4, 2], [5, 4, 2], reduction="none")
    with pytest.raises(NotImplementedError, match="none"):
        CrossEntropyLoss(reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        frame_cross_entropy(x, tg, [5, 4, 2], [5, 4, 2], reduction="batchmean")
    with pytest.raises(ValueError, match=r"\[0, 5\]"):
        frame_cross_entropy(x, tg, [6, 4, 2], [6, 4, 2])
    with pytest.raises(RuntimeError, match="MI355X"):   # and with everything in order the device is what is missing
        frame_cross_entropy(x, tg, [5, 4, 2], [5, 4, 2])


def test_fp64_cross_entropy_restatement_masks_like_the_reference():
    """The oracle itself: on a batch without padding it is F.cross_entropy over all rows; padded rows and ignored frames get a
    zero gradient and do not count."""
    rng = np.random.default_rng(0)
    T, B, C = 6, 2, 5
    x = rng.standard_normal((T, B, C))
    tg = rng.integers(0, C, size=(B, T))
    loss, grad, n, den = F.cross_entropy(x, tg, [T, T])
    want = torch.nn.functional.cross_entropy(torch.from_numpy(x).permute(1, 0, 2).reshape(-1, C), torch.from_numpy(tg).reshape(-1))
    assert abs(loss - float(want)) <= 1e-14 and n == T * B and den == T * B
    tg[0, 1] = -1
    loss, grad, n, den = F.cross_entropy(x, tg, [4, 0], ignore_index=-1, reduction="sum")
    assert n == 3 and den == 3 and np.all(grad[4:] == 0) and np.all(grad[:, 1] == 0) and np.all(grad[1, 0] == 0) and np.any(grad[0, 0] != 0)


def test_importing_the_new_script_creates_nothing(tmp_path, monkeypatch):
    """The rule tests/test_training_host.py holds the train_*.py / test_*.py files to, for the package beside them."""
    import importlib
    import sys
    import tempfile
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    for name in ("train_frame_recognition", "train_phoneme_recognition"):   # a fresh import of the script and of the one it imports
        monkeypatch.delitem(sys.modules, name, raising=False)
    module = importlib.import_module("train_frame_recognition")
    assert callable(module.main) and os.path.dirname(os.path.dirname(module.__file__)) == ROOT
    assert os.listdir(tmp_path) == []
    assert not hasattr(module, "TMP_DIR") and not hasattr(module, "RESULTS_DIR")
    assert os.path.exists(os.path.join(os.path.dirname(module.__file__), "__main__.py"))   # python -m train_frame_recognition


def test_new_config_parses_and_the_script_refuses_ctc(tmp_path):
    import train_frame_recognition as S
    import train_phoneme_recognition as T
    params = set(inspect.signature(S.main).parameters)
    assert params == set(inspect.signature(T.main).parameters)   # the same config keys as the CTC trainer
    with open(os.path.join(ROOT, "configs", "train_frame_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= params, set(cfg) - params
    assert cfg["loss"] == "CE" and cfg["feature"] == "vocal_tract" and cfg["target"] == "articulatory_target"
    assert cfg["datadir"] == "synthetic" and cfg["synthetic"]["num_special"] == 1
    vocabulary = T.build_vocabulary(cfg["vocab_filepath"], T.Criterion.CE)
    assert len(vocabulary) == 44 and vocabulary["<unk>"] == 0 and "<blank>" not in vocabulary
    with pytest.raises(NotImplementedError, match="train_phoneme_recognition.py"):
        S.main(**dict(cfg, loss="CTC", results_dir=str(tmp_path)))
    with pytest.raises(ValueError, match="one target per frame"):
        S.main(**dict(cfg, target="ctc_target", results_dir=str(tmp_path)))
