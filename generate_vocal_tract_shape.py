####################################################################################################
#
# Synthesise vocal-tract shapes on the MI355X engine (reference generate_vocal_tract_shape_v2.py and
# generate_vocal_tract_shape.py):
#   python generate_vocal_tract_shape.py --config cfg.yaml
# The YAML keys are the keyword arguments of main().  From v2's main: method (encoder_decoder,
# mean_contour, autoencoder), state_dict_filepath, vocab_filepath, articulators, save_to, model_params,
# aux_state_dict_filepath, aux_model_params and datadir (the autoencoder method reads its
# normalization_statistics/<articulator>_{mean,std}.npy there).  The sentences come from
#   sentences       [{name, phonemes_filepath}], each file in target_sequence.txt format
#   alignments_dir  every <index>_phonemes.txt that align_phoneme_recognition.py wrote
#   datadir: synthetic (with synthetic: {num_sentences, min_len, max_len, max_duration} and seed)
# in place of the reference's TextGrids.  batch_size (32) sentences take one forward pass and one
# contour-smoothing launch; regularize_outputs (true, the reference's default) with degree, n_ctrl,
# smoothing, n_out; upper_incisor_filepath: an optional (2, N) .npy written as every frame's
# upper-incisor contour when the articulators lack one; save_frames (true); air_column (false) with
# n_wall (100): one vocal-tract-tube launch per batch, this project's own definition of the reference's
# generate_vocal_tract_tube (artspeech_amd/phoneme_to_articulation/vocal_tract_tube.py).  Writes to save_to:
#   <name>/target_sequence.txt, <name>/contours.npy (T, A, 2, n_out)
#   <name>/inference_contours/%04d_<articulator>.npy   numbered from 1, the layout
#                          scripts/shape_to_air_column.py and load_raw_contours read
#   <name>/air_column/%04d.npy   with air_column: (2 walls, 2, n_wall) float64, internal wall first
#   <name>/xarticul/%04d.txt     with air_column: both walls times the data set's RES as Xarticul points
#   synthesis.json         sentences, frames, parameters, counts of flagged contours (and walls)
# Not written: the jpg / pdf / avi renderings.
#
####################################################################################################
import json
import logging

import numpy as np
import torch

from artspeech_amd.phoneme_to_articulation.synthesis import (METHODS, build_model, read_sentences, synthesize, synthetic_sentences,
                                                             write_summary)
from artspeech_amd.settings import DATASET_CONFIG, UNKNOWN
from artspeech_amd.training import build_vocabulary, run_cli


def main(method, state_dict_filepath, articulators, save_to, vocab_filepath=None, model_params=None, aux_state_dict_filepath=None,
         aux_model_params=None, datadir=None, database_name=None, sentences=None, alignments_dir=None, synthetic=None, seed=0,
         batch_size=32, regularize_outputs=True, degree=3, n_ctrl=12, smoothing=1e-3, n_out=None, upper_incisor_filepath=None,
         save_frames=True, air_column=False, n_wall=100):
    if method not in METHODS:
        raise ValueError(f"Unavailable method '{method}' (one of {', '.join(METHODS)})")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    articulators = sorted(articulators)
    vocabulary = build_vocabulary(vocab_filepath)
    if method == "mean_contour" and vocab_filepath is not None:
        # the mean-contour scripts' vocabulary (<unk> alone in front of the file's tokens): the method itself goes by token
        # strings, but seeded sentences must draw the tokens that the seeded training sentences drew
        vocabulary = build_vocabulary(vocab_filepath, (UNKNOWN,))
    model = build_model(method, vocabulary, articulators, state_dict_filepath, model_params, aux_state_dict_filepath,
                        aux_model_params, datadir, seed, device)
    if sentences is None and alignments_dir is None and datadir == "synthetic":
        todo = synthetic_sentences(vocabulary, articulators, seed=seed + 2, **(synthetic or {}))   # the test split's seed
    else:
        todo = read_sentences(sentences, alignments_dir)
    upper_incisor = None
    if upper_incisor_filepath is not None:
        upper_incisor = np.load(upper_incisor_filepath).astype(np.float32)
        if upper_incisor.ndim != 2 or upper_incisor.shape[0] != 2:
            raise ValueError(f"{upper_incisor_filepath}: expected a (2, N) contour, got {upper_incisor.shape}")
    info = synthesize(model, todo, vocabulary, articulators, save_to, batch_size, regularize_outputs, degree, n_ctrl, smoothing,
                      n_out, upper_incisor, save_frames, air_column, n_wall,
                      DATASET_CONFIG[database_name].RES if air_column and database_name is not None else 1.0)
    info["parameters"] = {"method": method, "batch_size": batch_size, "regularize_outputs": regularize_outputs, "degree": degree,
                          "n_ctrl": n_ctrl, "smoothing": smoothing, "n_out": n_out, "articulators": articulators}
    if air_column:
        info["parameters"]["n_wall"] = n_wall
    write_summary(save_to, info)
    return info


if __name__ == "__main__":
    info = run_cli(main, "vocal_tract_shape_synthesis", checkpoint=False)
    print(json.dumps({k: info[k] for k in ("frames", "flagged_contours", "parameters")}, indent=2))
