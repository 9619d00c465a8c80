####################################################################################################
#
# Fit the per-articulator PCA of the principal-components method (reference train_articulatory_PCA.py) on the
# MI355X engine:
#   python train_articulatory_PCA.py --config cfg.yaml [--mlflow URI --experiment NAME --run_id ID --run_name NAME]
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPrincipalComponentsAutoencoderDataset, sized by `synthetic:` and the sequence dicts' `num_frames`)
# and `results_dir`.  The training split is uploaded once and fitted in one call, in the order the reference's
# shuffling DataLoader would visit it; the test split is reconstructed and scored frame by frame.  Writes
# best_encoders.pt / best_decoders.pt (what train_phoneme_to_principal_components.py loads with encoder_type /
# decoder_type PCA), reconstruction_errors.csv and reconstruction_errors_agg.csv like the reference; its pickled
# sklearn objects (<articulator>_pca.pkl) have no counterpart here.
#
####################################################################################################
import csv
import logging
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from artspeech_amd.helpers import sequences_from_dict
from artspeech_amd.phoneme_to_articulation.metrics import MeanP2CPDistance
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import (
    PrincipalComponentsAutoencoderDataset2,
    SyntheticPrincipalComponentsAutoencoderDataset,
)
from artspeech_amd.phoneme_to_articulation.principal_components.pca import MultiArticulatorPCA
from artspeech_amd.settings import DATASET_CONFIG
from artspeech_amd.training import mlflow_call, results_paths, run_cli, synthetic_size


def _make_dataset(datadir, database_name, seq_dict, articulators, clip_tails, synthetic, seed):
    if datadir == "synthetic":
        n, cfg = synthetic_size(seq_dict, synthetic, "num_frames", 256)
        return SyntheticPrincipalComponentsAutoencoderDataset(n, articulators, seed=seed, database_name=database_name, **cfg)
    return PrincipalComponentsAutoencoderDataset2(database_name=database_name, datadir=datadir,
                                                  sequences=sequences_from_dict(datadir, seq_dict), articulators=articulators,
                                                  clip_tails=clip_tails)


def _collect(dataset, num_workers):
    """(frame names, frames (N, A, F)) of a dataset, in dataset order"""
    names, frames = [], []
    for frame_names, inputs, _, _ in DataLoader(dataset, batch_size=1024, shuffle=False, num_workers=num_workers):
        names.extend(frame_names)
        frames.append(inputs)
    return names, torch.cat(frames).float()


def main(database_name, datadir, batch_size, train_seq_dict, test_seq_dict, model_params, num_workers=0, clip_tails=True, seed=0,
         synthetic=None, results_dir=None, **kwargs):
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    results_dir, best_encoders_path, best_decoders_path = results_paths(results_dir, "artspeech_pca_",
                                                                       ("best_encoders.pt", "best_decoders.pt"))
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    articulators_indices_dict = model_params["indices_dict"]
    articulators = sorted(articulators_indices_dict.keys())
    dataset_config = DATASET_CONFIG[database_name]

    # the fit: every articulator's chain of batches in one call, rows in the order of DataLoader(shuffle=True, generator=gen)
    train_dataset = _make_dataset(datadir, database_name, train_seq_dict, articulators, clip_tails, synthetic, seed)
    _, train_frames = _collect(train_dataset, num_workers)
    order = torch.randperm(len(train_frames), generator=gen)
    pca = MultiArticulatorPCA(articulators_indices_dict, batch_size)
    pca.fit(train_frames.to(device), order.to(device))

    # the test split, reconstructed and scored per frame
    test_dataset = _make_dataset(datadir, database_name, test_seq_dict, articulators, clip_tails, synthetic, seed + 2)
    frame_names, test_frames = _collect(test_dataset, num_workers)
    test_order = torch.randperm(len(test_frames), generator=gen)
    frame_names = [frame_names[i] for i in test_order.tolist()]
    targets = test_frames[test_order].to(device)
    outputs = pca.inverse_transform(pca.transform(targets))
    num_frames, n_articulators, features = targets.shape
    targets = targets.reshape(num_frames, n_articulators, 2, features // 2).clone()
    outputs = outputs.reshape(num_frames, n_articulators, 2, features // 2).clone()
    for i, articulator in enumerate(articulators):
        denorm_fn = test_dataset.normalize[articulator].inverse
        outputs[:, i] = denorm_fn(outputs[:, i])
        targets[:, i] = denorm_fn(targets[:, i])
    p2cp_fn = MeanP2CPDistance(reduction="none")
    data_p2cp = (p2cp_fn(outputs.permute(0, 1, 3, 2).contiguous(), targets.permute(0, 1, 3, 2).contiguous())
                 * dataset_config.PIXEL_SPACING * dataset_config.RES).cpu().numpy()

    encoders_dict, decoders_dict = pca.state_dicts()
    torch.save(encoders_dict, best_encoders_path)
    mlflow_call("log_artifact", best_encoders_path)
    torch.save(decoders_dict, best_decoders_path)
    mlflow_call("log_artifact", best_decoders_path)

    df_errors_filepath = os.path.join(results_dir, "reconstruction_errors.csv")
    with open(df_errors_filepath, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(["subject", "sequence", "frame"] + articulators)
        for name, row in zip(frame_names, data_p2cp):
            writer.writerow(name.split("_") + [repr(float(v)) for v in row])
    mlflow_call("log_artifact", df_errors_filepath)

    aggregates = {"mean": data_p2cp.mean(axis=0), "std": data_p2cp.std(axis=0, ddof=1) if num_frames > 1 else np.full(n_articulators, np.nan),
                  "median": np.median(data_p2cp, axis=0), "min": data_p2cp.min(axis=0), "max": data_p2cp.max(axis=0)}
    df_errors_agg_filepath = os.path.join(results_dir, "reconstruction_errors_agg.csv")
    with open(df_errors_agg_filepath, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(["index"] + articulators)
        for name, row in aggregates.items():
            writer.writerow([name] + [repr(float(v)) for v in row])
    mlflow_call("log_artifact", df_errors_agg_filepath)
    return {"results_dir": results_dir, "num_train_frames": int(pca.n_samples_seen_), "num_test_frames": int(num_frames),
            "p2cp_mm": {a: float(v) for a, v in zip(articulators, aggregates["mean"])},
            "explained_variance_ratio": {a: float(v.sum()) for a, v in pca.explained_variance_ratio_.items()}}


if __name__ == "__main__":
    print(run_cli(main, "articulatory_pca"))
