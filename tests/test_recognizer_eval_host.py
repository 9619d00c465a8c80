"""Host-side pieces of the recogniser's evaluation (no GPU): the string-level alignment API against the reference's own results
(tests/golden/recognizer_eval.npz, part (a)), WordInfoLost on a hand-worked case, the class maps of the two matrices, run_test's
signature, the new config and the header's new entry points."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, load_golden

SETS = ["doc", "v2", "v5", "v12"]
NEW_SYMBOLS = ["as_decode_top1", "as_edit_distance", "as_align_workspace_bytes", "as_align_counts", "as_confusion_counts"]


@pytest.fixture(scope="module")
def fx():
    return load_golden("recognizer_eval")


def _set(fx, name):
    return ([str(s) for s in fx[f"a/{name}/vocab"]], [str(s) for s in fx[f"a/{name}/preds"]],
            [str(s) for s in fx[f"a/{name}/targets"]])


@pytest.mark.parametrize("name", SETS)
def test_compute_transitions_reproduces_the_reference(name, fx):
    from artspeech_amd.phoneme_recognition.metrics import _levenshtein, compute_transitions, edit_matrix
    _, preds, targets = _set(fx, name)
    want = json.loads(str(fx[f"a/{name}/transitions"]))
    got = compute_transitions(preds, targets)
    assert len(got) == len(want) >= 4
    for k, (g, w) in enumerate(zip(got, want)):
        assert [list(g[0]), list(g[1]), [list(s) for s in g[2]]] == w, (name, k, preds[k], targets[k])
    for p, t in zip(preds, targets):   # the table's corner is the distance the metric uses
        assert edit_matrix(p.split(), t.split())[-1][-1] == _levenshtein(p.split(), t.split())


@pytest.mark.parametrize("name", SETS)
def test_substitution_matrix_reproduces_the_reference(name, fx):
    from artspeech_amd.phoneme_recognition.metrics import substitution_matrix
    vocab, preds, targets = _set(fx, name)
    counts = substitution_matrix(preds, targets, vocab, "both", None)
    assert counts.dtype == np.float64 and np.array_equal(counts, fx[f"a/{name}/counts"])
    assert np.abs(substitution_matrix(preds, targets, vocab, "both", "true") - fx[f"a/{name}/true"]).max() <= 1e-12
    # without the extra row and column the insertions and deletions are left out, nothing else changes
    plain = substitution_matrix(preds, targets, vocab)
    assert np.array_equal(plain[:-1, :-1], counts[:-1, :-1]) and not plain[-1].any() and not plain[:, -1].any()


def test_compute_transitions_docstring_and_single_strings():
    from artspeech_amd.phoneme_recognition.metrics import compute_transitions
    assert compute_transitions("b c", "a b c") == [([0], [], [(1, 0), (2, 1)])]
    assert compute_transitions("", "") == [([], [], [])]
    assert compute_transitions("a b", "") == [([], [0, 1], [])]
    assert compute_transitions("", "a b") == [([0, 1], [], [])]


def test_word_info_lost_hand_worked():
    """preds "1 2 3" / "4" against targets "1 3" / "4 5": distances 1 + 1, longest 3 + 2, so H = 3, N_target = 4, N_pred = 4 and
    WIL = 1 - (3 / 4) (3 / 4) = 7 / 16."""
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost, word_information_lost
    assert word_information_lost(["1 2 3", "4"], ["1 3", "4 5"]) == 1 - (3 / 4) * (3 / 4) == 7 / 16
    assert word_information_lost(["1 2"], ["1 2"]) == 0.0
    dec = GreedyCTCDecoder(["<blank>", "a", "b", "c", "d", "e"], blank_token="<blank>")
    frames = torch.tensor([[1, 1, 0, 2, 3, 3], [4, 4, 4, 0, 0, 0]])
    em = torch.nn.functional.one_hot(frames, 6).float()
    targets, il, tl = torch.tensor([[1, 3], [4, 5]]), torch.tensor([6, 6]), torch.tensor([2, 2])
    assert WordInfoLost(dec)(em, targets, il, tl) == 7 / 16           # CPU tensors: the host path
    assert EditDistance(dec)(em, targets, il, tl) == 2 / 4
    assert np.isnan(word_information_lost([""], [""]))                # 0 / 0, as torchmetrics' tensors give


def test_class_maps_of_the_two_matrices():
    from artspeech_amd.phoneme_recognition import (CLASSES_NAMES, PHONETIC_CLASSES, _confusion_classes, _finish_confusion,
                                                   _substitution_classes)
    assert len(CLASSES_NAMES) == len(PHONETIC_CLASSES) + 1 == 8 and CLASSES_NAMES[7] == "other"
    assert sum(len(v) for v in PHONETIC_CLASSES.values()) == 33
    vocab = {"<blank>": 0, "<unk>": 1, "t": 2, "a": 4, "p": 5, "q": 7}   # ids 3 and 6 have no token
    assert _substitution_classes(vocab, None) == ([0, 1, 2, -1, 3, 4, -1, 5], 6)
    assert _substitution_classes(vocab, PHONETIC_CLASSES) == ([7, 7, 0, -1, 5, 1, -1, 7], 8)
    cmap, labels = _confusion_classes(vocab, None)
    assert labels == sorted(vocab) and [labels[c] for c in cmap] == ["<blank>", "<unk>", "t", "<unk>", "a", "p", "<unk>", "q", "<unk>"]
    cmap, labels = _confusion_classes(vocab, PHONETIC_CLASSES)
    assert labels == [0, 1, 5, 7] and [labels[c] for c in cmap] == [7, 7, 0, 7, 5, 1, 7, 7, 7]
    counts = np.array([[2, 0, 1], [0, 0, 0], [0, 0, 3]])                 # label 1 never occurs: dropped, as scikit-learn does
    assert np.array_equal(_finish_confusion(counts, None), [[2, 1], [0, 3]]) and _finish_confusion(counts, None).dtype == np.int64
    assert np.array_equal(_finish_confusion(counts, "true"), [[2 / 3, 1 / 3], [0.0, 1.0]])


def test_run_test_keeps_its_call_form_and_gains_keyword_only_arguments():
    from artspeech_amd.phoneme_recognition import PHONETIC_CLASSES, Feature, Target, run_test
    sig = inspect.signature(run_test)
    bound = sig.bind("model", "loader", {}, Target.CTC, feature=Feature.VOCAL_TRACT, use_voicing=False, device="dev", criterion=None)
    assert list(bound.arguments)[:4] == ["model", "dataloader", "fn_metrics", "target"]
    bound = sig.bind("model", "loader", {}, Target.CTC, Feature.VOCAL_TRACT, False, "dev", None)   # positionally, as before
    for name in ("decoder", "plot_target", "save_dir", "groups"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["groups"].default is PHONETIC_CLASSES and sig.parameters["save_dir"].default is None
    with pytest.raises(ValueError, match="decoder"):
        run_test(torch.nn.Identity(), [], {}, Target.CTC, device="cpu", save_dir="unused")


def test_new_config_parses_and_reads_the_trainers_model():
    import test_phoneme_recognition as E
    import train_phoneme_recognition as T
    with open(os.path.join(ROOT, "configs", "test_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthetic.yaml")) as f:
        train = yaml.safe_load(f)
    params = inspect.signature(E.main).parameters
    assert set(cfg) <= set(params), set(cfg) - set(params)
    reference_keywords = ["database_name", "datadir", "batch_size", "seq_dict", "vocab_filepath", "pretrained", "feature", "loss",
                          "model_params", "target", "state_dict_filepath", "plot_target", "voicing_filepath", "num_workers", "save_dir"]
    assert list(params)[: len(reference_keywords)] == reference_keywords
    assert cfg["state_dict_filepath"] == os.path.join(train["results_dir"], "best_model.pt")
    for key in ("model_params", "feature", "target", "plot_target", "synthetic", "datadir", "loss"):
        assert cfg[key] == train[key], key
    assert cfg["seq_dict"] == train["test_seq_dict"] and cfg["plot_target"] == "articulatory_target"
    assert "plot_target" in inspect.signature(T.main).parameters
    with pytest.raises(NotImplementedError, match="CTC"):
        E.main(**dict(cfg, loss="CE"))


def test_new_symbols_are_declared_and_bound():
    from artspeech_amd import _lib
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    assert "recog_eval.hip" in __import__("artspeech_amd.build", fromlist=["SOURCES"]).SOURCES
    # the sizing call needs no device: no workspace while the uint16 table fits the workgroup's LDS, the whole batch's tables past it
    assert L.as_align_workspace_bytes(32, 200, 60) == 0
    assert L.as_align_workspace_bytes(3, 4096, 2047) == 2 * 3 * 4097 * 2048


def test_device_wrappers_refuse_cpu_tensors():
    from artspeech_amd.phoneme_recognition import align
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    em = torch.rand(2, 5, 4)
    tok, cnt = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([1, 2])
    for call in (lambda: align.decode_top1(em), lambda: GreedyCTCDecoder(list("_abc"), blank_token="_").decode_device(em, [5, 5]),
                 lambda: TopKDecoder(list("_abc"), blank_token=0).decode_device(em, None),
                 lambda: align.edit_distance(tok, cnt, tok, cnt), lambda: align.align_counts(tok, cnt, tok, cnt, 4),
                 lambda: align.confusion_counts(tok, tok, None, 4)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
