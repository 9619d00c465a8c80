####################################################################################################
#
# Train the DeepSpeech2 phoneme recogniser with CTC (reference train_phoneme_recognition.py) on the
# MI355X engine:
#   python train_phoneme_recognition.py --config cfg.yaml [--mlflow URI --experiment NAME
#          --run_id ID --run_name NAME --checkpoint checkpoint.pt]
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPhonemeRecognitionDataset, sized by `synthetic:` and the sequence dicts' `num_sentences`) and
# `results_dir`; `dataset: shape_tree` reads datadir as a tree of synthesised shapes (ShapeTreeRecognitionDataset, the
# reference's phoneme_recognition/synthetic_shapes.py; test_phoneme_recognition.py, whose main() has no such keyword, takes
# `synthetic: {dataset: shape_tree}`).  With `feature: melspec` the synthetic data set is SyntheticAcousticRecognitionDataset
# (waveforms) and a batch's log-mel features are computed on the device while collating
# (datasets.acoustic_collate_fn); `melspec:` holds the MelSpectrogram keywords (default
# the reference's: 16 kHz, n_fft 1024, win_length 1024, hop_length 256, 80 mels; `synthetic: {melspec: ...}`
# is read too, which is how test_phoneme_recognition.py's config passes them).  Waveforms at another rate -- `synthetic:
# {orig_sample_rate: 44100}`, or WAV recordings listed in a JSON manifest with `datadir: recordings` and `manifest:` in each
# sequence dict -- are resampled to the transform's rate on the device first (features.Resample).  TrainableDeepSpeech2 + the engine's CTCLoss(**loss_params), Adam(lr, weight_decay) and
# CyclicLR(lr / 25, lr, cycle_momentum=False) stepped per batch; early stopping on the validation edit
# distance (greedy CTC decoding); best_model.pt, last_model.pt and checkpoint.pt like the reference, then
# a test-split pass of the best model written to info_test.json, with substitution_matrix.npy and (given `plot_target`)
# confusion_matrix.npy beside it.  CTC only (`loss: CE` raises).
#
####################################################################################################
import json
import logging
import os
from functools import partial

import torch
from torch.optim import Adam
from torch.optim.lr_scheduler import CyclicLR
from torch.utils.data import DataLoader

from artspeech_amd.helpers import sequences_from_dict, set_seeds
from artspeech_amd.phoneme_recognition import (BLANK, SIL, UNKNOWN, Criterion, Feature, Target, TrainableDeepSpeech2, run_epoch,
                                               run_test)
from artspeech_amd.phoneme_recognition.datasets import (PhonemeRecognitionDataset, RecordedAcousticRecognitionDataset,
                                                        ShapeTreeRecognitionDataset, SyntheticAcousticRecognitionDataset,
                                                        SyntheticPhonemeRecognitionDataset, acoustic_collate_fn, collate_fn)
from artspeech_amd.phoneme_recognition.features import MelSpectrogram
from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
from artspeech_amd.phoneme_recognition.metrics import EditDistance
from artspeech_amd.settings import TRAIN, VALID
from artspeech_amd import training
from artspeech_amd.training import fit, load_checkpoint, load_json, mlflow_call, results_paths, run_cli, synthetic_size


def build_vocabulary(vocab_filepath, criterion):
    """{token: index}: blank (CTC only) and unknown first, then the JSON list (reference :84-90)"""
    return training.build_vocabulary(vocab_filepath, (BLANK, UNKNOWN) if criterion == Criterion.CTC else (UNKNOWN,))


MELSPEC_DEFAULTS = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=256, n_mels=80)   # reference datasets.py:59-63
VOICING_WITH_MELSPEC = "feature: melspec takes no voicing_filepath: voicing is per articulatory frame, not per spectrogram frame"


def _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, seed, melspec=None, dataset=None):
    """The split's data set.  With datadir: synthetic and feature: melspec it is the waveform data set, carrying the MelSpectrogram
    that collate_fn launches on its batches: MELSPEC_DEFAULTS, overridden by `synthetic: {melspec: {...}}` (the way
    test_phoneme_recognition.py passes it, whose main() has no melspec keyword), then by `melspec`.  `synthetic: {orig_sample_rate:
    44100}` generates the waveforms at that rate, and `datadir: recordings` reads the WAV files of the sequence dict's `manifest:`
    (RecordedAcousticRecognitionDataset; `synthetic:` then holds its keywords and `melspec`): either way the collate function
    resamples a batch to the transform's rate on the device before the log-mel launch.  `dataset: shape_tree` reads datadir as a
    tree of synthesised shapes (ShapeTreeRecognitionDataset: the output of generate_vocal_tract_shape.py with air_column: true);
    `synthetic: {dataset: shape_tree}` says the same, for test_phoneme_recognition.py and the scripts whose main() follows its
    keywords (decode_, embed_), which have no dataset keyword -- the way they pass `melspec`."""
    options = dict(synthetic or {})
    nested = options.pop("dataset", None)
    if dataset is not None and nested is not None and nested != dataset:
        raise ValueError(f"dataset: {dataset!r} and synthetic: {{dataset: {nested!r}}} disagree")
    dataset = nested if dataset is None else dataset
    if dataset == "shape_tree":
        return ShapeTreeRecognitionDataset(database_name, datadir, vocabulary, sequences_from_dict(datadir, seq_dict), voiced_tokens,
                                           **options)
    if dataset is not None:
        raise ValueError(f"dataset: {dataset!r} (shape_tree, or leave it out)")
    if datadir == "synthetic":
        n, cfg = synthetic_size(seq_dict, synthetic, "num_sentences", 32)
        mel_kw = {**MELSPEC_DEFAULTS, **(cfg.pop("melspec", None) or {}), **(melspec or {})}
        if feature == Feature.MELSPEC:
            if voiced_tokens is not None:
                raise ValueError(VOICING_WITH_MELSPEC)
            ds = SyntheticAcousticRecognitionDataset(n, vocabulary, sample_rate=mel_kw["sample_rate"], seed=seed, **cfg)
            ds.melspectrogram = MelSpectrogram(**mel_kw)
            return ds
        return SyntheticPhonemeRecognitionDataset(n, vocabulary, seed=seed, voiced_tokens=voiced_tokens, **cfg)
    if datadir == "recordings":
        manifest, cfg = synthetic_size(seq_dict, synthetic, "manifest", None)
        if feature != Feature.MELSPEC or manifest is None:
            raise ValueError("datadir: recordings reads `manifest:` from the sequence dict and takes feature: melspec alone")
        if voiced_tokens is not None:
            raise ValueError(VOICING_WITH_MELSPEC)
        mel_kw = {**MELSPEC_DEFAULTS, **(cfg.pop("melspec", None) or {}), **(melspec or {})}
        ds = RecordedAcousticRecognitionDataset(manifest, vocabulary, **cfg)
        ds.melspectrogram = MelSpectrogram(**mel_kw)
        return ds
    return PhonemeRecognitionDataset(datadir=datadir, database_name=database_name, sequences=sequences_from_dict(datadir, seq_dict),
                                     vocabulary=vocabulary, features=[feature], voiced_tokens=voiced_tokens)


def make_collate_fn(datadir, feature, num_workers, dataset=None):
    """collate_fn over the feature; on the synthetic waveforms of feature: melspec, acoustic_collate_fn around the data set's
    MelSpectrogram and vocabulary (its launch has to happen in the main process)."""
    if feature != Feature.MELSPEC or datadir not in ("synthetic", "recordings"):
        return partial(collate_fn, features_names=[feature])
    if num_workers != 0:
        raise ValueError("feature: melspec computes its features on the device while collating: num_workers must be 0")
    return partial(acoustic_collate_fn, melspectrogram=dataset.melspectrogram, vocabulary=dataset.vocabulary)


def main(database_name, datadir, num_epochs, batch_size, patience, learning_rate, weight_decay, feature, target, vocab_filepath,
         train_seq_dict, valid_seq_dict, test_seq_dict, model_params, loss, plot_target=None, loss_params=None, num_workers=0,
         logits_large_margins=0.0, pretrained=False, voicing_filepath=None, state_dict_filepath=None, checkpoint_filepath=None,
         seed=0, synthetic=None, results_dir=None, dataset=None, melspec=None):
    criterion = Criterion[loss]
    if criterion != Criterion.CTC:
        raise NotImplementedError(f"train_phoneme_recognition: loss {loss!r} is not supported; only CTC is ported")
    if Feature(feature) == Feature.MELSPEC and voicing_filepath is not None:
        raise ValueError(VOICING_WITH_MELSPEC)
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    results_dir, best_model_path, last_model_path, save_checkpoint_path = results_paths(results_dir, "artspeech_recognizer_")

    feature = Feature(feature)
    target = Target(target)
    plot_target = Target(plot_target) if plot_target is not None else None
    if pretrained:
        raise NotImplementedError("train_phoneme_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    vocabulary = build_vocabulary(vocab_filepath, criterion)
    voiced_tokens = load_json(voicing_filepath)
    tokens = [k for k, _ in sorted(vocabulary.items(), key=lambda t: t[1])]
    decoder = GreedyCTCDecoder(tokens=tokens, sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN)

    model = TrainableDeepSpeech2(num_classes=len(vocabulary), **model_params)
    if state_dict_filepath is not None:
        model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)
    print(f"\nDeepSpeech2 -- {model.total_parameters} parameters\n")
    mlflow_call("log_param", "num_network_params", model.total_parameters)

    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    def loader(seq_dict, ds_seed):
        ds = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, ds_seed, melspec, dataset)
        return DataLoader(ds, batch_size=batch_size, shuffle=True, num_workers=num_workers, worker_init_fn=set_seeds,
                          collate_fn=make_collate_fn(datadir, feature, num_workers, ds), generator=gen)

    train_dataloader = loader(train_seq_dict, seed)
    valid_dataloader = loader(valid_seq_dict, seed + 1)

    loss_fn = criterion.value(**(loss_params or {}))
    optimizer = Adam(model.parameters(), lr=learning_rate, weight_decay=weight_decay)
    scheduler = CyclicLR(optimizer, base_lr=learning_rate / 25, max_lr=learning_rate, cycle_momentum=False)
    metrics = {"edit_distance": EditDistance(decoder)}
    use_voicing = voicing_filepath is not None
    common = dict(model=model, criterion=loss_fn, fn_metrics=metrics, device=device, feature=feature, target=target,
                  use_voicing=use_voicing, normalize_outputs=True, use_log_prob=True, optimizer=optimizer, scheduler=scheduler)

    # CyclicLR steps per batch inside run_epoch and is not part of the checkpoint
    first_epoch, best_metric, epochs_since_best, _ = load_checkpoint(checkpoint_filepath, model, optimizer, map_location=device)
    history = fit(range(first_epoch, num_epochs + 1),
                  lambda epoch: run_epoch(phase=TRAIN, epoch=epoch, dataloader=train_dataloader,
                                          logits_large_margins=logits_large_margins, **common),
                  lambda epoch: run_epoch(phase=VALID, epoch=epoch, dataloader=valid_dataloader, **common),
                  metric="edit_distance", patience=patience, best_files=[(best_model_path, model.state_dict)],
                  last_files=[(last_model_path, model.state_dict)], checkpoint_path=save_checkpoint_path,
                  checkpoint_state=lambda: {"model": model.state_dict(), "optimizer": optimizer.state_dict(),
                                            "best_model_path": best_model_path, "last_model_path": last_model_path},
                  best_metric=best_metric, epochs_since_best=epochs_since_best)

    # test split: the best model, with the substitution matrix and (given a plot_target) the frame-level confusion matrix written
    # to results_dir as the reference's closing run_test does (its plots are not part of this engine)
    test_dataloader = loader(test_seq_dict, seed + 2)
    best_model = TrainableDeepSpeech2(num_classes=len(vocabulary), **model_params)
    best_model.load_state_dict(torch.load(best_model_path if os.path.exists(best_model_path) else last_model_path, map_location="cpu"))
    best_model.to(device)
    info_test = run_test(best_model, test_dataloader, metrics, target, feature=feature, use_voicing=use_voicing, device=device,
                         criterion=loss_fn, decoder=decoder, plot_target=plot_target, save_dir=results_dir)
    with open(os.path.join(results_dir, "info_test.json"), "w") as f:
        json.dump(info_test, f, indent=2)
    mlflow_call("log_metrics", {f"test_{m}": v for m, v in info_test.items()}, step=0)
    return {"history": history, "test": info_test, "results_dir": results_dir}


if __name__ == "__main__":
    run_cli(main, "phoneme_recognition")
