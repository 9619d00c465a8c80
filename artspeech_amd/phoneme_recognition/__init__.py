"""Phoneme recognition (reference ``phoneme_recognition``): the DeepSpeech2 scorer -- frozen (``DeepSpeech2``, the forward + top-1
decoding that config 5 of BASELINE.json puts behind the phoneme-to-articulation models, with its input gradient) and trainable
(``TrainableDeepSpeech2``) -- the CTC loss, the decoders, the edit-distance metric, the data sets and the training loop of
train_phoneme_recognition.py (``run_epoch`` / ``run_test``, reference :63-153 and :156-...).  CTC only: the reference's CE
criterion, the confusion / substitution matrices and their plots are not ported."""
from enum import Enum

import numpy as np
import torch

from ..settings import BLANK, SIL, TRAIN, UNKNOWN  # noqa: F401
from .ctc import CTCLoss, ctc_loss
from .deepspeech2 import DeepSpeech2, TrainableDeepSpeech2, top1_phonemes  # noqa: F401


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


def run_test(model, dataloader, fn_metrics, target, feature=Feature.MELSPEC, use_voicing=False, device=None, criterion=None):
    """The test pass of train_phoneme_recognition.py (reference run_test :156-...): eval-mode outputs, the metrics on their softmax
    and, with a criterion, the loss on their log-softmax.  Returns {"loss": ..., metric: ...}."""
    if device is None:
        device = torch.device("cuda")
    model.eval()
    losses, metrics_values = [], {name: [] for name in fn_metrics}
    with torch.no_grad():
        for batch in dataloader:
            inputs = batch[feature.value].to(device)
            input_lengths = batch[f"{feature.value}_length"]
            targets = batch[target.value].to(device)
            target_lengths = batch[f"{target.value}_length"]
            voicing = batch["voicing"].to(device) if use_voicing else None
            outputs = model(inputs, voicing)
            if criterion is not None:
                losses.append(_loss(model, outputs, criterion, targets, input_lengths, target_lengths, True, True).item())
            norm_outputs = model.get_normalized_outputs(outputs)
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].append(float(fn_metric(norm_outputs, targets, input_lengths, target_lengths)))
    info = {name: float(np.mean(v)) for name, v in metrics_values.items()}
    if criterion is not None:
        info["loss"] = float(np.mean(losses))
    return info
