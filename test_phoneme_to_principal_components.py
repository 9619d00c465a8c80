####################################################################################################
#
# Test the autoencoder-based phoneme-to-articulation (reference test_phoneme_to_principal_components.py) on the
# MI355X engine:
#   python test_phoneme_to_principal_components.py --config cfg.yaml
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPrincipalComponentsPhonemeToArticulationDataset, sized by `synthetic:` and the sequence dict's
# `num_sentences`), `seed`, and `encoder_type` / `decoder_type` (AE | PCA, as in the trainer: a model trained against PCA
# projections is tested against them).  Writes test_outputs/0/<sentence>/ (contours, phonemes.csv, tract_variables.csv)
# and test_results.json under `save_to`.
#
####################################################################################################
import argparse
import json
import os

import torch
import yaml
from torch.utils.data import DataLoader

from artspeech_amd.helpers import make_indices_dict, set_seeds
from artspeech_amd.phoneme_recognition import DeepSpeech2
from artspeech_amd.phoneme_to_articulation import RNNType
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import pad_sequence_collate_fn
from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import run_phoneme_to_principal_components_test
from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
from artspeech_amd.phoneme_to_articulation.principal_components.models import (DecoderType, EncoderType,
                                                                               PrincipalComponentsArtSpeech)
from artspeech_amd.training import load_json
from train_phoneme_to_principal_components import _make_dataset, build_vocabulary


def main(database_name, datadir, batch_size, seq_dict, indices_dict, vocab_filepath, state_dict_filepath, modelkwargs,
         autoencoder_kwargs, save_to, encoder_state_dict_filepath, decoder_state_dict_filepath, rnn_type="GRU", beta1=1.0,
         beta2=1.0, beta3=1.0, beta4=0.0, recognizer_filepath=None, recognizer_params=None, voicing_filepath=None, num_workers=0,
         TV_to_phoneme_map=None, clip_tails=True, encoder_type="AE", decoder_type="AE", synthetic=None, seed=0):
    device = torch.device("cuda", torch.cuda.current_device())
    vocabulary = build_vocabulary(vocab_filepath)
    voiced_tokens = load_json(voicing_filepath)
    if isinstance(list(indices_dict.values())[0], int):
        indices_dict = make_indices_dict(indices_dict)
    articulators = sorted(indices_dict.keys())

    test_dataset = _make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, TV_to_phoneme_map, clip_tails,
                                 voiced_tokens, synthetic, seed + 2)
    test_dataloader = DataLoader(test_dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                 worker_init_fn=set_seeds, collate_fn=pad_sequence_collate_fn)

    TVs = sorted((TV_to_phoneme_map or {}).keys())
    if recognizer_filepath:
        recognizer = DeepSpeech2(num_classes=len(vocabulary), **(recognizer_params or {}))
        recognizer.load_state_dict(torch.load(recognizer_filepath, map_location=device))
        recognizer.to(device)
        for p in recognizer.parameters():
            p.requires_grad = False
    else:
        recognizer = None
    denorm_fn = {articulator: normalize.inverse for articulator, normalize in test_dataset.normalize.items()}
    loss_fn = AutoencoderLoss2(indices_dict=indices_dict, TVs=TVs, device=device,
                               encoder_state_dict_filepath=encoder_state_dict_filepath,
                               decoder_state_dict_filepath=decoder_state_dict_filepath, denormalize_fn=denorm_fn, beta1=beta1,
                               beta2=beta2, beta3=beta3, beta4=beta4, encoder_cls=EncoderType[encoder_type.upper()].value,
                               decoder_cls=DecoderType[decoder_type.upper()].value, recognizer=recognizer, **autoencoder_kwargs)

    model = PrincipalComponentsArtSpeech(vocab_size=len(vocabulary), indices_dict=indices_dict, rnn=RNNType[rnn_type.upper()],
                                         **modelkwargs)
    model.load_state_dict(torch.load(state_dict_filepath, map_location=device))
    model.to(device)
    print(f"\nPrincipalComponentsArtSpeech -- {model.total_parameters} parameters\n")

    test_outputs_dir = os.path.join(save_to, "test_outputs")
    os.makedirs(test_outputs_dir, exist_ok=True)
    info_test = run_phoneme_to_principal_components_test(epoch=0, model=model, dataloader=test_dataloader, criterion=loss_fn,
                                                         outputs_dir=test_outputs_dir, decode_transform=loss_fn.decode,
                                                         device=device)
    with open(os.path.join(save_to, "test_results.json"), "w") as f:
        json.dump(info_test, f)
    return info_test


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="cfg_filepath")
    return parser.parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    with open(args.cfg_filepath) as f:
        cfg = yaml.safe_load(f.read())
    print(main(**cfg))
