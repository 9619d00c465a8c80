####################################################################################################
#
# Test the DeepSpeech2 phoneme recogniser (reference test_phoneme_recognition.py) on the MI355X engine:
#   python test_phoneme_recognition.py --config cfg.yaml
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras
# `datadir: synthetic` (SyntheticPhonemeRecognitionDataset, sized by `synthetic:` and `seq_dict`'s
# `num_sentences`; the trainer's test split, seed + 2) and `seed`.  Loads state_dict_filepath into the
# frozen DeepSpeech2 and runs the test pass with best-path CTC decoding: edit distance and word
# information lost per batch, and, accumulated on the device over the whole split, the substitution
# matrix and the frame-level confusion matrix against plot_target.  Writes info_test.json,
# substitution_matrix.npy and confusion_matrix.npy to save_dir.  Without a plot_target no confusion
# matrix is written (the reference falls back to `target`, whose CTC form has no frame alignment); the
# reference's plots are not ported.  CTC only (`loss: CE` raises).
#
####################################################################################################
import argparse
import json
import logging
import os
from functools import partial

import torch
import yaml
from torch.utils.data import DataLoader

from artspeech_amd.helpers import set_seeds
from artspeech_amd.phoneme_recognition import BLANK, SIL, UNKNOWN, Criterion, DeepSpeech2, Feature, Target, run_test
from artspeech_amd.phoneme_recognition.datasets import collate_fn
from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost
from artspeech_amd.training import load_json
from train_phoneme_recognition import _make_dataset, build_vocabulary


def main(database_name, datadir, batch_size, seq_dict, vocab_filepath, pretrained, feature, loss, model_params, target,
         state_dict_filepath, plot_target=None, voicing_filepath=None, num_workers=0, save_dir=None, seed=0, synthetic=None):
    criterion = Criterion[loss]
    if criterion != Criterion.CTC:
        raise NotImplementedError(f"test_phoneme_recognition: loss {loss!r} is not supported; only CTC is ported")
    if pretrained:
        raise NotImplementedError("test_phoneme_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    feature = Feature(feature)
    target = Target(target)
    plot_target = Target(plot_target) if plot_target else None

    vocabulary = build_vocabulary(vocab_filepath, criterion)
    voiced_tokens = load_json(voicing_filepath)
    tokens = [k for k, _ in sorted(vocabulary.items(), key=lambda t: t[1])]
    decoder = GreedyCTCDecoder(tokens=tokens, sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN)

    model = DeepSpeech2(num_classes=len(vocabulary), **model_params)
    model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)
    print(f"\nDeepSpeech2 -- {model.total_parameters} parameters\n")

    dataset = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, seed + 2)
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, worker_init_fn=set_seeds,
                            collate_fn=partial(collate_fn, features_names=[feature]))
    metrics = {"edit_distance": EditDistance(decoder), "word_info_lost": WordInfoLost(decoder)}
    info_test = run_test(model=model, dataloader=dataloader, fn_metrics=metrics, decoder=decoder, device=device, feature=feature,
                         target=target, plot_target=plot_target, use_voicing=voicing_filepath is not None, save_dir=save_dir)
    if save_dir is not None:
        with open(os.path.join(save_dir, "info_test.json"), "w") as f:
            json.dump(info_test, f, indent=2)
    return info_test


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    args = parser.parse_args()
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    print(json.dumps(main(**cfg), indent=2))
