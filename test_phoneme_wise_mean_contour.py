####################################################################################################
#
# Test the phoneme-wise mean contour phoneme-to-articulation (reference test_phoneme_wise_mean_contour.py) on the
# MI355X engine:
#   python test_phoneme_wise_mean_contour.py --config cfg.yaml
# The YAML keys are the keyword arguments of main() (the reference's).  `state_dict_filepath` is the table file of
# the reference's (or this) trainer, or the trainer's phoneme_wise_articulators.pt.  Extras: `datadir: synthetic`
# (SyntheticSegmentedArtSpeechDataset, `synthetic:` options, `seed`), `frac` (the per-token sample of the forward
# pass, the reference's hard-coded 0.1) and `batch_size`.  Writes test_outputs/, test_results.json and
# test_results.csv under `save_to`.
#
####################################################################################################
import argparse
import os

import torch
import yaml

from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import PhonemeWiseMeanContour, test
from train_phoneme_wise_mean_contour import build_vocabulary, make_dataset, write_results


def main(database_name, datadir, seq_dict, vocab_filepath, articulators, state_dict_filepath, save_to, clip_tails=True,
         weighted=False, synthetic=None, seed=0, frac=0.1, batch_size=32):
    device = torch.device("cuda", torch.cuda.current_device())
    vocabulary = build_vocabulary(vocab_filepath)
    test_dataset = make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, clip_tails, synthetic, seed + 2)

    if state_dict_filepath.endswith((".pt", ".pth")):
        model = PhonemeWiseMeanContour().load_state_dict(torch.load(state_dict_filepath, map_location="cpu"), device)
    else:
        model = PhonemeWiseMeanContour.from_csv(state_dict_filepath, vocabulary, device)
    print("Finished loading data frame")

    test_outputs_dir = os.path.join(save_to, "test_outputs")
    os.makedirs(test_outputs_dir, exist_ok=True)
    test_results = test(test_dataset, model, test_outputs_dir, weighted=weighted, frac=frac, batch_size=batch_size, device=device)
    write_results(test_results, test_dataset.articulators, save_to)
    return test_results


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    return parser.parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    print(main(**cfg))
