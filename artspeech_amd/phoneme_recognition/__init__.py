"""Phoneme recognition (reference ``phoneme_recognition``): the DeepSpeech2 scorer -- frozen (``DeepSpeech2``, the forward + top-1
decoding that config 5 of BASELINE.json puts behind the phoneme-to-articulation models, with its input gradient) and trainable
(``TrainableDeepSpeech2``) -- the CTC loss, the decoders, the edit-distance metric, the data sets and the training loop of
train_phoneme_recognition.py (``run_epoch`` / ``run_test``, reference :63-153 and :156-329), and the evaluation products of
test_phoneme_recognition.py: the substitution matrix (``compute_substitution_matrix``, :470-526) and the frame-level confusion
matrix (``compute_confusion_matrix``, :410-432), counted on the device (align.py) and normalised on the host in float64 as the
reference does.  The frame-level criterion and metrics of the reference's ``loss: CE`` branch (``CrossEntropyLoss`` /
``frame_cross_entropy``, and ``Accuracy``, ``F1Score``, ``AUROC`` in metrics.py) run on the device too and are trained by
`python -m train_frame_recognition`; ``Criterion.CE`` and the five CTC entry scripts still refuse ``loss: CE``.  The t-SNE map of the
recogniser's features (``plot_features``, :332-399) is embedded on the device (tsne.py) and written by ``run_test`` where it is
asked for (embed_phoneme_recognition.py); the plots of the two matrices are not ported."""
import json
import os
from enum import Enum

import numpy as np
import torch

from ..settings import BLANK, SIL, TRAIN, UNKNOWN  # noqa: F401
from .align import align_counts, confusion_counts, decode_top1, edit_distance  # noqa: F401
from .beam_search import BeamResult, ctc_beam_search  # noqa: F401
from .ctc import CTCLoss, ctc_loss
from .decoders import GreedyCTCDecoder, TopKDecoder
from .deepspeech2 import DeepSpeech2, TrainableDeepSpeech2, top1_phonemes  # noqa: F401
from .forced_align import Alignment, align_test, forced_align  # noqa: F401
from .frame_ce import frame_cross_entropy  # noqa: F401
from .metrics import CrossEntropyLoss, normalize_counts  # noqa: F401
from .tsne import TSNE, _embed_features, draw_embedding, feature_embedding, plot_features, sample_features_per_class  # noqa: F401

CLASSES_NAMES = {
    0: "dental",
    1: "labial",
    2: "palatal",
    3: "front vowels",
    4: "back vowels",
    5: "open vowels",
    6: "rounded vowels",
    7: "other",
}

PHONETIC_CLASSES = {
    0: ["t", "d", "n", "l", "z", "s"],
    1: ["p", "b", "m", "f", "v"],
    2: ["k", "g", "Z", "S"],
    3: ["i", "e", "E", "E/", "U~/", "j"],
    4: ["u", "o", "O", "O/", "o~", "w"],
    5: ["a", "a~"],
    6: ["y", "2", "9", "H"],
}


class _CrossEntropyUnsupported:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("phoneme recognition: only the CTC criterion (loss: CTC) is ported; CE is not supported")


class Criterion(Enum):
    CE = _CrossEntropyUnsupported
    CTC = CTCLoss


class Feature(Enum):
    MELSPEC = "melspec"
    VOCAL_TRACT = "vocal_tract"
    AIR_COLUMN = "air_column"


class Target(Enum):
    CTC = "ctc_target"
    ACOUSTIC = "acoustic_target"
    ARTICULATORY = "articulatory_target"


def _loss(model, outputs, criterion, targets, input_lengths, target_lengths, normalize_outputs, use_log_prob):
    """criterion(log_softmax(outputs).permute(1, 0, 2), ...) (reference :114-120); with the engine's CTCLoss the log-softmax is
    fused into the kernel (the gradient with respect to the logits is the same)."""
    if isinstance(criterion, CTCLoss) and normalize_outputs and use_log_prob:
        return ctc_loss(outputs.permute(1, 0, 2), targets, input_lengths, target_lengths, criterion.blank, criterion.reduction,
                        criterion.zero_infinity, logits=True)
    if normalize_outputs:
        outputs = model.get_normalized_outputs(outputs, use_log_prob=use_log_prob)
    return criterion(outputs.permute(1, 0, 2), targets, input_lengths, target_lengths)


def run_epoch(phase, epoch, model, dataloader, optimizer, criterion, normalize_outputs, use_log_prob, target, feature=Feature.MELSPEC,
              use_voicing=False, logits_large_margins=0.0, scheduler=None, fn_metrics=None, device=None):
    """One epoch (reference :63-153): in training, Gaussian noise of scale logits_large_margins on the logits (:112), the loss on
    their log-softmax, backward, optimizer and per-batch scheduler steps; the metrics on the softmax (:130-132)."""
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    training = phase == TRAIN
    model.train(training)
    losses = []
    metrics_values = {name: [] for name in fn_metrics}
    for batch in dataloader:
        inputs = batch[feature.value].to(device)
        input_lengths = batch[f"{feature.value}_length"]
        targets = batch[target.value].to(device)
        target_lengths = batch[f"{target.value}_length"]
        voicing = batch["voicing"].to(device) if use_voicing else None
        optimizer.zero_grad()
        with torch.set_grad_enabled(training):
            outputs = model(inputs, voicing)
            if training and logits_large_margins > 0.0:
                outputs = model.get_noise_logits(outputs, logits_large_margins)
            loss = _loss(model, outputs, criterion, targets, input_lengths, target_lengths, normalize_outputs, use_log_prob)
            if training:
                loss.backward()
                optimizer.step()
                if scheduler is not None:
                    scheduler.step()
            losses.append(loss.item())
        norm_outputs = model.get_normalized_outputs(outputs.detach())
        for name, fn_metric in fn_metrics.items():
            metrics_values[name].append(float(fn_metric(norm_outputs, targets, input_lengths, target_lengths)))
    info = {"loss": float(np.mean(losses))}
    info.update({name: float(np.mean(v)) for name, v in metrics_values.items()})
    return info


def _groups_transposed(groups):
    return {symbol: group for group, symbols in groups.items() for symbol in symbols}


def _first_position(labels):
    pos = {}
    for k, label in enumerate(labels):
        pos.setdefault(label, k)   # list.index: the first occurrence
    return pos


def _substitution_classes(vocabulary, groups):
    """(class per token id 0 .. max id, number of classes) of the substitution matrix: without groups a token's class is its
    position in list(vocabulary) (reference :483); with groups it is its group's position in list(groups) + [max(groups) + 1],
    tokens outside every group falling into that last "other" class (:456, :486).  An id without a token gets -1."""
    names = {i: token for token, i in vocabulary.items()}
    if groups is None:
        pos = _first_position(list(vocabulary))
        token_class = lambda token: pos[token]   # noqa: E731
        n = len(vocabulary)
    else:
        other = max(groups.keys()) + 1
        pos = _first_position(list(groups.keys()) + [other])
        groups_T = _groups_transposed(groups)
        token_class = lambda token: pos[groups_T.get(token, other)]   # noqa: E731
        n = len(groups) + 1
    return [token_class(names[i]) if i in names else -1 for i in range(max(names) + 1)], n


def _confusion_classes(vocabulary, groups):
    """(class per token id 0 .. max id plus one last entry for every other id, sorted labels) of the confusion matrix: an id
    without a token counts as UNKNOWN (reference :418-419); labels are the token names, or with groups the group numbers and
    "other" = max(groups) + 1."""
    names = {i: token for token, i in vocabulary.items()}
    ids = list(range(max(names) + 1)) + [None]
    tokens = [names.get(i, UNKNOWN) for i in ids]
    if groups is not None:
        other = max(groups.keys()) + 1
        groups_T = _groups_transposed(groups)
        tokens = [groups_T.get(token, other) for token in tokens]
    labels = sorted(set(tokens))
    pos = {label: k for k, label in enumerate(labels)}
    return [pos[token] for token in tokens], labels


def _pad(rows, value):
    return torch.nn.utils.rnn.pad_sequence([torch.as_tensor(r) for r in rows], batch_first=True, padding_value=value)


def substitution_counts(emissions, targets, input_lengths, target_lengths, decoder, class_map, n_classes, out=None):
    """Decode on the device and add the batch's alignment counts to ``out`` ((n_classes + 1)-square int32 on the device; see
    align.align_counts).  emissions: (B, T, C) on the device, or a list of per-utterance (T_b, C) tensors, each decoded over its
    own rows (and no further than its input length when the decoder uses lengths) -- by decode_top1 for the two top-1 decoders,
    by its own decode_device for any other (BeamSearchCTCDecoder); targets: (B, S) or a list of 1-D tensors."""
    if not hasattr(decoder, "decode_device"):
        raise TypeError("substitution_counts: the decoder has no decode_device (TopKDecoder and GreedyCTCDecoder have)")
    if isinstance(emissions, (list, tuple)):
        rows = torch.tensor([e.shape[0] for e in emissions], dtype=torch.int64)
        if decoder.uses_lengths:
            rows = torch.minimum(rows, torch.as_tensor([int(n) for n in input_lengths], dtype=torch.int64))
        if isinstance(decoder, (TopKDecoder, GreedyCTCDecoder)):
            tokens, counts = decode_top1(_pad(emissions, 0.0), rows, decoder.blank_index)
        else:   # a decoder of its own kind (the beam search) decodes the padded batch itself, over each utterance's rows
            tokens, counts = decoder.decode_device(_pad(emissions, 0.0), rows)
    else:
        tokens, counts = decoder.decode_device(emissions, input_lengths)
    if isinstance(targets, (list, tuple)):
        targets = _pad(targets, -1)
    target_lengths = torch.as_tensor([int(n) for n in target_lengths]).clamp(0, targets.shape[1])
    return align_counts(tokens, counts, targets, target_lengths, n_classes, class_map, out)[0]


def compute_substitution_matrix(emissions, targets, input_lengths, target_lengths, decoder, vocabulary, groups=None):
    """The reference's compute_substitution_matrix (:470-526): substitution_matrix(decoded predictions, targets,
    insertions_and_deletions="both", normalize="true") over the vocabulary's tokens or, with ``groups`` ({class: [tokens]}), over
    the groups plus "other" = max(groups) + 1.  The counts are taken on the device (as_decode_top1 + as_align_counts); the row
    normalisation and nan_to_num run on the host in float64.  Inputs as in ``substitution_counts``."""
    class_map, n = _substitution_classes(vocabulary, groups)
    counts = substitution_counts(emissions, targets, input_lengths, target_lengths, decoder, class_map, n)
    return normalize_counts(counts.cpu().numpy(), "true")


def _finish_confusion(counts, normalize):
    """sklearn.metrics.confusion_matrix from the counts over every label: labels that occur neither as a target nor as a
    prediction are dropped; normalize "true" / "pred" / "all" in float64 with NaN -> 0, else int64 counts."""
    cm = np.asarray(counts, dtype=np.int64)
    keep = (cm.sum(axis=0) + cm.sum(axis=1)) > 0
    cm = cm[keep][:, keep]
    return normalize_counts(cm, normalize) if normalize in ("true", "pred", "all") else cm


def compute_confusion_matrix(predictions, targets, vocabulary, groups=None, normalize=None):
    """The reference's compute_confusion_matrix (:410-432): sklearn's confusion_matrix of the per-frame target tokens (rows) and
    predicted tokens (columns), labels sorted, or of their groups.  predictions, targets: flat per-frame token ids (device
    tensors, or anything torch.as_tensor takes, which is uploaded); the counts are taken on the device (as_confusion_counts).

    With ``groups`` the class of a token outside every group is ``max(groups) + 1``, as in the substitution matrix.  The
    reference takes ``max`` over the symbol strings there, which scikit-learn rejects as soon as one token lies outside the
    groups (labels of mixed type), so only the case in which every token is grouped can be compared with it."""
    dev = predictions.device if torch.is_tensor(predictions) and predictions.is_cuda else torch.device("cuda", torch.cuda.current_device())
    class_map, labels = _confusion_classes(vocabulary, groups)
    n_ids = len(class_map) - 1

    def ids(x):
        x = torch.as_tensor(x).to(dev).reshape(1, -1).to(torch.int64)
        return torch.where((x < 0) | (x >= n_ids), torch.full_like(x, n_ids), x)

    predictions, targets = ids(predictions), ids(targets)
    if predictions.shape != targets.shape:
        raise ValueError(f"compute_confusion_matrix: {predictions.shape[1]} predictions but {targets.shape[1]} targets")
    counts = confusion_counts(predictions, targets, None, len(labels), class_map)
    return _finish_confusion(counts.cpu().numpy(), normalize)


def _save_model_features(features, targets, vocabulary, groups, options, save_dir):
    """The files of run_test's ``model_features`` (see there)."""
    max_items = int(options.pop("max_items_per_class", 100))
    seed = int(options.pop("seed", 0))
    groups = options.pop("groups", None) or groups
    embedding, tokens, group_idx, tsne = _embed_features(features.detach(), targets, vocabulary, groups, max_items, seed, options)
    embedding, tokens, group_idx = embedding.cpu().numpy(), tokens.cpu().numpy(), group_idx.cpu().numpy()
    np.save(os.path.join(save_dir, "model_features_tsne.npy"), embedding.astype(np.float32))
    np.save(os.path.join(save_dir, "model_features_tokens.npy"), tokens.astype(np.int64))
    np.save(os.path.join(save_dir, "model_features_groups.npy"), group_idx.astype(np.int64))
    with open(os.path.join(save_dir, "model_features.json"), "w") as f:
        json.dump({"kl_divergence": tsne.kl_divergence_, "n_iter": tsne.n_iter_, "learning_rate": tsne.learning_rate_,
                   "perplexity": float(tsne.perplexity), "seed": seed, "max_items_per_class": max_items, "points": int(len(tokens)),
                   "points_per_group": {str(key): int((group_idx == g).sum()) for g, key in enumerate(groups)}}, f, indent=2)
    draw_embedding(embedding, group_idx, groups, os.path.join(save_dir, "model_features.pdf"))


def run_test(model, dataloader, fn_metrics, target, feature=Feature.MELSPEC, use_voicing=False, device=None, criterion=None, *,
             decoder=None, plot_target=None, save_dir=None, groups=PHONETIC_CLASSES, model_features=None):
    """The test pass of train_phoneme_recognition.py / test_phoneme_recognition.py (reference run_test :156-329): eval-mode
    outputs, the metrics on their softmax and, with a criterion, the loss on their log-softmax.  Returns {"loss": ..., metric: ...}.

    With ``save_dir`` (and a ``decoder``) the counts of both matrices are accumulated on the device across the batches and
    written as the reference writes them: ``substitution_matrix.npy`` (decoded predictions against ``target``, over ``groups``,
    row-normalised) and, with a ``plot_target``, ``confusion_matrix.npy`` (the per-frame arg-max against ``plot_target``, frame by
    frame, over ``groups``, normalize="true").  The plots of the two matrices are not ported.

    ``model_features`` (a dict; needs ``save_dir`` and ``plot_target``) asks for the reference's third product, the t-SNE map of
    the last hidden features (:228-233, :246-261): the model is called with ``return_features=True``, the valid frames' features
    and plot targets stay on the device, and after the loop ``feature_embedding`` (tsne.py) samples ``max_items_per_class``
    (100) frames per token of ``groups`` with ``seed`` (0) and embeds them; a ``groups`` key of its own ({group: [tokens]}) replaces
    ``groups`` for the map alone (a synthetic vocabulary has none of the phonetic tokens); every other key is a ``TSNE`` keyword
    (perplexity, max_iter, ...).  Written: ``model_features_tsne.npy`` (M x 2 float32), ``model_features_tokens.npy``,
    ``model_features_groups.npy`` (int64), ``model_features.json`` (KL divergence, iterations, learning rate, perplexity, seed,
    points per group) and, with matplotlib, ``model_features.pdf`` and its legend.  With None nothing of this runs."""
    if model_features is not None and (save_dir is None or plot_target is None):
        raise ValueError("run_test: model_features needs a save_dir and a plot_target")
    feats, feat_targets = [], []
    if device is None:
        device = torch.device("cuda")
    model.eval()
    losses, metrics_values = [], {name: [] for name in fn_metrics}
    sub_counts = conf_counts = None
    if save_dir is not None:
        if decoder is None:
            raise ValueError("run_test: save_dir needs the decoder whose predictions the substitution matrix aligns")
        vocabulary = dataloader.dataset.vocabulary
        sub_map, n_sub = _substitution_classes(vocabulary, groups)
        sub_map = torch.tensor(sub_map, dtype=torch.int32, device=device)
        sub_counts = torch.zeros(n_sub + 1, n_sub + 1, dtype=torch.int32, device=device)
        if plot_target is not None:
            conf_map, conf_labels = _confusion_classes(vocabulary, groups)
            conf_map = torch.tensor(conf_map[:-1], dtype=torch.int32, device=device)
            conf_counts = torch.zeros(len(conf_labels), len(conf_labels), dtype=torch.int32, device=device)
    with torch.no_grad():
        for batch in dataloader:
            inputs = batch[feature.value].to(device)
            input_lengths = batch[f"{feature.value}_length"]
            targets = batch[target.value].to(device)
            target_lengths = batch[f"{target.value}_length"]
            voicing = batch["voicing"].to(device) if use_voicing else None
            if model_features is None:
                outputs = model(inputs, voicing)
            else:
                outputs, features = model(inputs, voicing, return_features=True)
                frame_targets = batch[plot_target.value].to(device)
                for b, (n_in, n_tgt) in enumerate(zip(input_lengths, batch[f"{plot_target.value}_length"])):
                    n = min(int(n_in), int(n_tgt), features.shape[1], frame_targets.shape[1])   # a frame with its target
                    feats.append(features[b, :n])
                    feat_targets.append(frame_targets[b, :n])
            if criterion is not None:
                losses.append(_loss(model, outputs, criterion, targets, input_lengths, target_lengths, True, True).item())
            norm_outputs = model.get_normalized_outputs(outputs)
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].append(float(fn_metric(norm_outputs, targets, input_lengths, target_lengths)))
            if sub_counts is not None:
                substitution_counts(norm_outputs, targets, input_lengths, target_lengths, decoder, sub_map, n_sub, sub_counts)
            if conf_counts is not None:
                plot_lengths = torch.minimum(torch.as_tensor(input_lengths), torch.as_tensor(batch[f"{plot_target.value}_length"]))
                argmax = decode_top1(norm_outputs, plot_lengths, return_argmax=True)[2]
                confusion_counts(argmax, batch[plot_target.value].to(device), plot_lengths, len(conf_labels), conf_map, conf_counts)
    if sub_counts is not None:
        os.makedirs(save_dir, exist_ok=True)
        np.save(os.path.join(save_dir, "substitution_matrix.npy"), normalize_counts(sub_counts.cpu().numpy(), "true"))
    if conf_counts is not None:
        np.save(os.path.join(save_dir, "confusion_matrix.npy"), _finish_confusion(conf_counts.cpu().numpy(), "true"))
    if model_features is not None:
        _save_model_features(torch.cat(feats), torch.cat(feat_targets), vocabulary, groups, dict(model_features), save_dir)
    info = {name: float(np.mean(v)) for name, v in metrics_values.items()}
    if criterion is not None:
        info["loss"] = float(np.mean(losses))
    return info
