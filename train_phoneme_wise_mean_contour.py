####################################################################################################
#
# Train the phoneme-wise mean contour phoneme-to-articulation (reference train_phoneme_wise_mean_contour.py) on
# the MI355X engine:
#   python train_phoneme_wise_mean_contour.py --config cfg.yaml [--mlflow URI --experiment NAME --run_id ID --run_name NAME]
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticSegmentedArtSpeechDataset, sized by `synthetic:` and the sequence dicts' `num_sentences`), `seed`,
# `results_dir`, `frac` (the per-token sample of the forward pass, the reference's hard-coded 0.1; 1.0 uses every
# stored frame) and `batch_size` (sentences per evaluation launch).  "Training" tabulates every training frame on
# the device; writes phoneme_wise_articulators.csv (the reference's table file) and phoneme_wise_articulators.pt
# (the model's state_dict), then evaluates the test split: test_outputs/, test_results.json, test_results.csv.
#
####################################################################################################
import csv
import json
import logging
import os

import torch

from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import ArtSpeechDataset
from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import (
    PhonemeWiseMeanContour,
    SyntheticSegmentedArtSpeechDataset,
    test,
    train,
)
from artspeech_amd import training
from artspeech_amd.settings import UNKNOWN
from artspeech_amd.training import cli_parser, mlflow_call, results_paths, run_cli, synthetic_size


def build_vocabulary(vocab_filepath):
    """{token: index}: <unk> first, then the JSON list (reference :40-45); without a file, the synthetic vocabulary of
    train_phoneme_to_articulation.py (<blank>, <unk>, 43 phoneme names)."""
    return training.build_vocabulary(vocab_filepath, (UNKNOWN,)) if vocab_filepath is not None else training.build_vocabulary(None)


def make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, clip_tails, synthetic, seed):
    if datadir == "synthetic":
        n, cfg = synthetic_size(seq_dict, synthetic, "num_sentences", 16)
        return SyntheticSegmentedArtSpeechDataset(n, vocabulary, articulators, seed=seed, database_name=database_name, **cfg)
    from artspeech_amd.helpers import sequences_from_dict
    return ArtSpeechDataset(datadir, database_name, sequences_from_dict(datadir, seq_dict), vocabulary, articulators,
                            clip_tails=clip_tails)


def write_results(test_results, articulators, results_dir):
    """test_results.json and the one-row test_results.csv of the reference (:90-106)"""
    test_results_filepath = os.path.join(results_dir, "test_results.json")
    with open(test_results_filepath, "w") as f:
        json.dump(test_results, f)
    results_item = {"loss": test_results["loss"]}
    for articulator in articulators:
        results_item[f"x_corr_{articulator}"] = test_results[articulator]["x_corr"]
        results_item[f"y_corr_{articulator}"] = test_results[articulator]["y_corr"]
    df_filepath = os.path.join(results_dir, "test_results.csv")
    with open(df_filepath, "w", newline="") as f:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(results_item.keys())
        writer.writerow([repr(float(v)) for v in results_item.values()])
    return test_results_filepath, df_filepath


def main(database_name, datadir, train_seq_dict, test_seq_dict, vocab_filepath, articulators, state_dict_filepath=None,
         clip_tails=True, weighted=False, synthetic=None, seed=0, results_dir=None, frac=0.1, batch_size=32):
    device = torch.device("cuda", torch.cuda.current_device())
    results_dir, = results_paths(results_dir, "artspeech_mean_contour_", ())
    vocabulary = build_vocabulary(vocab_filepath)

    if state_dict_filepath is None:
        train_dataset = make_dataset(datadir, database_name, train_seq_dict, vocabulary, articulators, clip_tails, synthetic, seed)
        save_to = os.path.join(results_dir, "phoneme_wise_articulators.csv")
        model = train(train_dataset, save_to=save_to, weighted=weighted, device=device)
        mlflow_call("log_artifact", save_to)
        state_dict_path = os.path.join(results_dir, "phoneme_wise_articulators.pt")
        torch.save(model.state_dict(), state_dict_path)
        mlflow_call("log_artifact", state_dict_path)
    elif state_dict_filepath.endswith((".pt", ".pth")):
        model = PhonemeWiseMeanContour().load_state_dict(torch.load(state_dict_filepath, map_location="cpu"), device)
        mlflow_call("log_artifact", state_dict_filepath)
    else:
        model = PhonemeWiseMeanContour.from_csv(state_dict_filepath, vocabulary, device)
        mlflow_call("log_artifact", state_dict_filepath)
    logging.info("Finished training phoneme wise mean contour")

    test_dataset = make_dataset(datadir, database_name, test_seq_dict, vocabulary, articulators, clip_tails, synthetic, seed + 2)
    test_outputs_dir = os.path.join(results_dir, "test_outputs")
    os.makedirs(test_outputs_dir, exist_ok=True)
    test_results = test(test_dataset, model, test_outputs_dir, weighted=weighted, frac=frac, batch_size=batch_size, device=device)
    mlflow_call("log_artifact", test_outputs_dir)
    for path in write_results(test_results, test_dataset.articulators, results_dir):
        mlflow_call("log_artifact", path)
    return {"results_dir": results_dir, "num_stored_frames": int(model.bank.shape[0]), **test_results}


def parse_args(argv=None):
    return cli_parser("phoneme_wise_mean_contour", checkpoint=False).parse_args(argv)


if __name__ == "__main__":
    print(run_cli(main, "phoneme_wise_mean_contour", checkpoint=False))
