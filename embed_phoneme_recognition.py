####################################################################################################
#
# The recogniser's test pass with the t-SNE map of its last hidden features on the MI355X engine:
#   python embed_phoneme_recognition.py --config cfg.yaml
# test_phoneme_recognition.py with one more YAML key: the keyword arguments of main() are that
# script's, in its order, plus `model_features` -- a block of max_items_per_class, seed, groups
# and TSNE keywords (perplexity, max_iter, ...), see run_test.  The reference draws this map,
# model_features.pdf, inside its test_phoneme_recognition.py (phoneme_recognition/__init__.py
# :246-261, :332-399); here it is a pass of its own so that test_phoneme_recognition.py stays as it
# is.  Writes what that script writes (info_test.json, substitution_matrix.npy,
# confusion_matrix.npy) and model_features_tsne.npy (M x 2 float32), model_features_tokens.npy,
# model_features_groups.npy, model_features.json and, with matplotlib, model_features.pdf and its
# legend.  Needs a save_dir and a plot_target.  CTC only (`loss: CE` raises).
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
         state_dict_filepath, plot_target=None, voicing_filepath=None, num_workers=0, save_dir=None, seed=0, synthetic=None,
         model_features=None):
    criterion = Criterion[loss]
    if criterion != Criterion.CTC:
        raise NotImplementedError(f"embed_phoneme_recognition: loss {loss!r} is not supported; only CTC is ported")
    if pretrained:
        raise NotImplementedError("embed_phoneme_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    if save_dir is None or plot_target is None:
        raise ValueError("embed_phoneme_recognition: the feature map needs a save_dir and a plot_target")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    feature = Feature(feature)

    vocabulary = build_vocabulary(vocab_filepath, criterion)
    voiced_tokens = load_json(voicing_filepath)
    tokens = [k for k, _ in sorted(vocabulary.items(), key=lambda t: t[1])]
    decoder = GreedyCTCDecoder(tokens=tokens, sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN)

    model = DeepSpeech2(num_classes=len(vocabulary), **model_params)
    model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)

    dataset = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, seed + 2)
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, worker_init_fn=set_seeds,
                            collate_fn=partial(collate_fn, features_names=[feature]))
    metrics = {"edit_distance": EditDistance(decoder), "word_info_lost": WordInfoLost(decoder)}
    info_test = run_test(model=model, dataloader=dataloader, fn_metrics=metrics, decoder=decoder, device=device, feature=feature,
                         target=Target(target), plot_target=Target(plot_target), use_voicing=voicing_filepath is not None,
                         save_dir=save_dir, model_features=dict(model_features or {}))
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
