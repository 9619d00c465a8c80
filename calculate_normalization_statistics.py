####################################################################################################
#
# Per-articulator normalisation statistics of the principal-components method (reference
# scripts/calculate_normalization_statistics.py) on the MI355X engine:
#   python calculate_normalization_statistics.py --config cfg.yaml
# The YAML keys are the reference's: database_name, datadir, save_to, sequences_dict, articulators, num_samples.
# The frames' raw contours are read once, prepared (tails clipped, upper-incisor frame) in one launch and
# reduced per articulator by one more (fp64 accumulation, one rounding); <save_to>/<articulator>_mean.npy and
# <articulator>_std.npy, each (2, N) float32, are what the principal-components datasets read from
# <datadir>/normalization_statistics/.  With `num_samples` the frames are drawn by random.Random(seed): the
# reference's draw is unseeded, so which frames it takes is not pinned.  Extras: `datadir: synthetic`
# (SyntheticRawContours, sized by sequences_dict's / `synthetic:`'s num_frames) and `seed`.
#
####################################################################################################
import logging
import os
import random

import numpy as np
import torch

from artspeech_amd.helpers import sequences_from_dict
from artspeech_amd.phoneme_to_articulation import (
    SyntheticRawContours,
    contour_statistics,
    load_raw_contours,
    prepare_contours,
)
from artspeech_amd.settings import DATASET_CONFIG
from artspeech_amd.training import mlflow_call, run_cli, synthetic_size


def _collect_frames(database_name, datadir, sequences_dict):
    """[(subject, sequence, frame_id)] of every frame of the sequences, in the collector's order"""
    try:
        from database_collector import DATABASE_COLLECTORS  # the reference's collectors
    except ImportError as exc:
        raise ImportError("walking a real corpus needs the reference's database_collector on PYTHONPATH; "
                          "use `datadir: synthetic` without it") from exc
    sentences = DATABASE_COLLECTORS[database_name](datadir).collect_data(sequences_from_dict(datadir, sequences_dict))
    return [(s["subject"], s["sequence"], frame_id) for s in sentences for frame_id in s["frame_ids"]]


def _load_frames(datadir, frames, articulators, dataset_config):
    """raw (F, A, N, 2), refs (F, 3, N, 2) of the frames, read sequence by sequence in the order given"""
    raws, refs, start = [], [], 0
    while start < len(frames):
        stop = start
        while stop < len(frames) and frames[stop][:2] == frames[start][:2]:
            stop += 1
        raw, ref = load_raw_contours(datadir, *frames[start][:2], [f[2] for f in frames[start:stop]], articulators,
                                     norm_value=dataset_config.RES)
        raws.append(raw)
        refs.append(ref)
        start = stop
    return torch.cat(raws), torch.cat(refs)


def main(database_name, datadir, save_to, sequences_dict, articulators, num_samples=None, seed=0, synthetic=None, **kwargs):
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    dataset_config = DATASET_CONFIG[database_name]
    if datadir == "synthetic":
        n, options = synthetic_size(sequences_dict, synthetic, "num_frames", 512)
        data = SyntheticRawContours(n, articulators, seed=seed, **options)
        chosen = list(range(len(data)))
        if num_samples is not None:
            chosen = random.Random(seed).sample(chosen, num_samples)
        raw, refs = data.raw[chosen], data.refs[chosen]
    else:
        frames = _collect_frames(database_name, datadir, sequences_dict)
        if num_samples is not None:
            frames = random.Random(seed).sample(frames, num_samples)
        raw, refs = _load_frames(datadir, frames, articulators, dataset_config)

    # clip_tails=True is the default of prepare_articulator_array, which the reference's script leaves alone
    targets, _, _ = prepare_contours(raw.to(device), refs.to(device), articulators, dataset_config)
    os.makedirs(save_to, exist_ok=True)
    for i, articulator in enumerate(articulators):
        mean, std = contour_statistics(targets[:, i])
        for what, value in (("mean", mean), ("std", std)):
            path = os.path.join(save_to, f"{articulator}_{what}.npy")
            np.save(path, value.cpu().numpy())
            mlflow_call("log_artifact", path)
    return {"save_to": save_to, "num_frames": int(raw.shape[0]), "articulators": list(articulators)}


if __name__ == "__main__":
    print(run_cli(main, "normalization_statistics", checkpoint=False))
