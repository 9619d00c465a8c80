"""Fixture of the recogniser's evaluation (test_phoneme_recognition.py), produced by the reference's own functions:
phoneme_recognition/metrics.py (compute_transitions, substitution_matrix), decoders.py (TopKDecoder) and __init__.py
(compute_substitution_matrix, compute_confusion_matrix).  Run from the repository root with the reference checkout at
make_golden.REF:

    python tests/golden/make_golden_recognizer_eval.py

Writes tests/golden/recognizer_eval.npz (data only):

(a) ``a/<set>/...``: string pairs per vocabulary -- the four pairs of compute_transitions' docstring, pairs over 2 tokens (nearly
    every back-trace step is a tie), over 5 and over 12 tokens, half of them a corrupted copy of the target and half independent,
    lengths 0 - 14 -- with compute_transitions' result per pair (JSON) and substitution_matrix("both") with normalize None and
    "true".
(b) ``b/...``: 12 utterances of soft emissions (T = 40 frames at most, 12 classes whose names come from PHONETIC_CLASSES) with
    their CTC targets, and compute_substitution_matrix through TopKDecoder(blank_token=0), with and without groups: once with the
    emissions trimmed to their lengths (best-path decoding over the lengths) and once untrimmed (TopKDecoder decodes the padding
    too).
(c) ``c/...``: compute_confusion_matrix of the per-frame arg-max against the per-frame targets with groups=None (normalize None
    and "true"), and with groups on frames whose tokens all lie in a group -- the only grouped case the reference can run.

Absent packages (torchmetrics, ujson, seaborn, funcy, ...) are name-only shims; np.int (removed from numpy) is int."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load, _shim, install_shims, save  # noqa: E402

NAMES = ["t", "d", "p", "b", "k", "i", "u", "a", "y", "2"]   # two dentals, two labials, one of every other group


def _pairs(rng, vocab, n, max_len):
    preds, targets = [], []
    for k in range(n):
        tgt = [vocab[i] for i in rng.integers(0, len(vocab), rng.integers(0, max_len + 1))]
        if k % 2:   # independent
            pred = [vocab[i] for i in rng.integers(0, len(vocab), rng.integers(0, max_len + 1))]
        else:       # the target with random substitutions, deletions and insertions
            pred = []
            for tok in tgt:
                r = rng.random()
                if r < 0.15:
                    continue
                pred.append(vocab[rng.integers(0, len(vocab))] if r < 0.35 else tok)
                if rng.random() < 0.15:
                    pred.append(vocab[rng.integers(0, len(vocab))])
        preds.append(" ".join(pred))
        targets.append(" ".join(tgt))
    return preds, targets


def main():
    install_shims()
    sys.modules["funcy"].lflatten = lambda seq: [x for sub in seq for x in sub]
    _shim("ujson", load=json.load, dump=json.dump)
    _shim("seaborn")
    tm = _shim("torchmetrics")
    tm.classification = _shim("torchmetrics.classification", MulticlassAccuracy=None, MulticlassAUROC=None, MulticlassF1Score=None)
    tm.functional = _shim("torchmetrics.functional", word_error_rate=None, word_information_lost=None)
    if not hasattr(np, "int"):
        np.int = int
    sys.path.insert(0, REF)
    settings = _load("settings", "settings.py")
    pkg = types.ModuleType("phoneme_recognition")
    pkg.__path__ = [os.path.join(REF, "phoneme_recognition")]
    sys.modules["phoneme_recognition"] = pkg
    metrics = _load("phoneme_recognition.metrics", "phoneme_recognition/metrics.py")
    decoders = _load("phoneme_recognition.decoders", "phoneme_recognition/decoders.py")
    ref = _load("phoneme_recognition", "phoneme_recognition/__init__.py")
    out = {}

    # ---- (a) string pairs
    rng = np.random.default_rng(0)
    sets = {
        "doc": (["a", "b", "c", "d", "e"], ["a b c", "b c", "a b c d", "c b d e"], ["a b c", "a b c", "a b c", "a b d e a"]),
        "v2": (["x", "y"], *_pairs(rng, ["x", "y"], 80, 14)),
        "v5": (["a", "b", "c", "d", "e"], *_pairs(rng, ["a", "b", "c", "d", "e"], 60, 12)),
        "v12": ([settings.BLANK, settings.UNKNOWN] + NAMES, *_pairs(rng, NAMES, 60, 14)),
    }
    for name, (vocab, preds, targets) in sets.items():
        out[f"a/{name}/vocab"] = np.array(vocab)
        out[f"a/{name}/preds"] = np.array(preds)
        out[f"a/{name}/targets"] = np.array(targets)
        out[f"a/{name}/transitions"] = np.array(json.dumps(metrics.compute_transitions(preds, targets)))
        out[f"a/{name}/counts"] = metrics.substitution_matrix(preds, targets, vocab, "both", None)
        out[f"a/{name}/true"] = metrics.substitution_matrix(preds, targets, vocab, "both", "true")
    doc = json.loads(str(out["a/doc/transitions"]))
    assert doc == [[[], [], [[0, 0], [1, 1], [2, 2]]], [[0], [], [[1, 0], [2, 1]]], [[], [3], [[0, 0], [1, 1], [2, 2]]],
                   [[4], [], [[0, 0], [1, 1], [2, 2], [3, 3]]]], doc

    # ---- (b) emissions -> substitution matrix
    vocabulary = {tok: i for i, tok in enumerate([settings.BLANK, settings.UNKNOWN] + NAMES)}
    C, B, T = len(vocabulary), 12, 40
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(8, T + 1, (B,), generator=g)
    lengths[0], lengths[1] = T, 1
    frame_targets = torch.full((B, T), -1, dtype=torch.long)
    logits = 1.5 * torch.randn(B, T, C, generator=g)   # the padding frames are noise: decoding them changes the result
    for b in range(B):
        frames = []
        while len(frames) < int(lengths[b]):
            tok = int(torch.randint(1 if b % 4 == 3 else 2, C, (1,), generator=g))   # every fourth utterance may hold <unk>
            frames += [tok] * int(torch.randint(1, 6, (1,), generator=g))
        frame_targets[b, : lengths[b]] = torch.tensor(frames[: int(lengths[b])])
        for t in range(int(lengths[b])):
            r = float(torch.rand(1, generator=g))
            hot = 0 if r < 0.25 else int(frame_targets[b, t])   # blanks inside and between the runs
            logits[b, t, hot] += 4.0
    emissions = torch.softmax(logits, dim=-1)
    ctc_targets = [torch.unique_consecutive(frame_targets[b, : lengths[b]]) for b in range(B)]
    target_lengths = torch.tensor([len(t) for t in ctc_targets])
    targets = torch.nn.utils.rnn.pad_sequence(ctc_targets, batch_first=True, padding_value=-1)
    decoder = decoders.TopKDecoder(tokens=list(vocabulary), blank_token=0)
    trimmed = [emissions[b, : lengths[b]] for b in range(B)]
    for tag, ems in (("trimmed", trimmed), ("untrimmed", list(emissions))):
        for gtag, groups in (("tokens", None), ("groups", ref.PHONETIC_CLASSES)):
            out[f"b/{tag}/{gtag}"] = ref.compute_substitution_matrix(ems, list(targets), list(lengths), list(target_lengths), decoder,
                                                                     vocabulary, groups=groups)
    assert not np.array_equal(out["b/trimmed/tokens"], out["b/untrimmed/tokens"])
    out.update({"b/vocab": np.array(list(vocabulary)), "b/emissions": emissions.numpy(), "b/lengths": lengths.numpy(),
                "b/targets": targets.numpy(), "b/target_lengths": target_lengths.numpy(), "b/frame_targets": frame_targets.numpy()})

    # ---- (c) confusion matrices
    top = emissions.argmax(dim=-1)
    preds_flat = torch.cat([top[b, : lengths[b]] for b in range(B)]).numpy().astype(np.float32)   # run_test hands floats over
    tgts_flat = torch.cat([frame_targets[b, : lengths[b]] for b in range(B)]).numpy().astype(np.float32)
    out["c/tokens/counts"] = ref.compute_confusion_matrix(preds_flat, tgts_flat, vocabulary, groups=None, normalize=None)
    out["c/tokens/true"] = ref.compute_confusion_matrix(preds_flat, tgts_flat, vocabulary, groups=None, normalize="true")
    grouped = (preds_flat >= 2) & (tgts_flat >= 2)   # frames whose two tokens lie in a group
    out["c/groups/mask"] = grouped
    out["c/groups/counts"] = ref.compute_confusion_matrix(preds_flat[grouped], tgts_flat[grouped], vocabulary,
                                                          groups=ref.PHONETIC_CLASSES, normalize=None)
    out["c/groups/true"] = ref.compute_confusion_matrix(preds_flat[grouped], tgts_flat[grouped], vocabulary,
                                                        groups=ref.PHONETIC_CLASSES, normalize="true")
    save("recognizer_eval", **out)


if __name__ == "__main__":
    main()
