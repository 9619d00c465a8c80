####################################################################################################
#
# Test the multi-articulator autoencoder of the principal-components method (reference
# test_principal_components_autoencoder.py) on the MI355X engine:
#   python test_principal_components_autoencoder.py --config cfg.yaml
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPrincipalComponentsAutoencoderDataset, sized by `synthetic:` and the sequence dict's `num_frames`) and `seed`.
# Like the reference's __main__, main() (test loss + latent covariance per articulator, test_results.json) is followed by
# evaluate_autoencoder(): latent_space.csv, reconstruction_errors.npy / .csv / _agg.csv and nomograms.npy under `save_to`.
# The plots (covariance heat maps, nomograms, latent histograms) are not produced; the arrays behind them are.
#
####################################################################################################
import argparse
import csv
import json
import os

import numpy as np
import torch
import yaml
from torch.utils.data import DataLoader

from artspeech_amd.helpers import make_indices_dict, set_seeds
from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import (PCEvalState, denorm_tables, median_rows,
                                                                                   pc_shapes_eval,
                                                                                   run_multiart_autoencoder_test)
from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
from artspeech_amd.phoneme_to_articulation.principal_components.models.autoencoder import MultiArticulatorAutoencoder
from artspeech_amd.settings import DATASET_CONFIG
from train_principal_components_autoencoder import _make_dataset


def _resolve_indices(model_params):
    model_params = dict(model_params)
    indices_dict = model_params["indices_dict"]
    if isinstance(list(indices_dict.values())[0], int):
        model_params["indices_dict"] = make_indices_dict(indices_dict)
    return model_params


def _load_autoencoder(model_params, encoders_filepath, decoders_filepath, device):
    autoencoder = MultiArticulatorAutoencoder(**model_params)
    autoencoder.encoders.load_state_dict(torch.load(encoders_filepath, map_location=device))
    autoencoder.decoders.load_state_dict(torch.load(decoders_filepath, map_location=device))
    autoencoder.to(device)
    autoencoder.eval()
    print(f"\nMultiArticulatorAutoencoder -- {autoencoder.total_parameters} parameters\n")
    return autoencoder


def _write_csv(path, header, rows):
    with open(path, "w", newline="") as f:
        writer = csv.writer(f, lineterminator="\n")   # pandas.DataFrame.to_csv(index=False) layout
        writer.writerow(header)
        writer.writerows(rows)


def nomogram_latents(latent_size):
    """(L * 21, L): row i * 21 + j is zero except component i at np.arange(-1, 1.01, 0.1)[j] (reference :43-50)."""
    pc_range = torch.from_numpy(np.arange(-1, 1.01, 0.1)).float()
    latents = torch.zeros(latent_size, len(pc_range), latent_size)
    for i in range(latent_size):
        latents[i, :, i] = pc_range
    return latents.reshape(-1, latent_size)


def evaluate_autoencoder(database_name, datadir, dataset_config, batch_size, sequences_dict, model_params, encoders_filepath,
                         decoders_filepath, save_to, num_workers=0, clip_tails=True, synthetic=None, seed=0):
    """The reference's evaluate_autoencoder (:92-208).  Per batch: the autoencoder, one as_pc_shapes_eval launch (denormalise
    + MeanP2CPDistance in mm) and one as_pc_eval_accumulate; the per-frame errors and latents stay on the device for the whole
    split, the median comes from one sort at the end, and the host reads once.  nomograms.npy (L, 21, A, 2, N) holds the
    denormalised decoder outputs the reference's nomogram plots draw."""
    os.makedirs(os.path.join(save_to, "plots"), exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())
    model_params = _resolve_indices(model_params)
    articulators = sorted(model_params["indices_dict"].keys())
    dataset = _make_dataset(datadir, database_name, sequences_dict, articulators, clip_tails, synthetic, seed + 2)
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, worker_init_fn=set_seeds, num_workers=num_workers)
    autoencoder = _load_autoencoder(model_params, encoders_filepath, decoders_filepath, device)
    latent_size = autoencoder.latent_size
    to_mm = dataset_config.PIXEL_SPACING * dataset_config.RES
    mean, std = denorm_tables(dataset.normalize, articulators, device)

    state = PCEvalState(device, n_articulators=len(articulators))
    frame_names, all_p2cp, all_latents = [], [], []
    with torch.no_grad():
        for names, inputs, _, _ in dataloader:
            inputs = inputs.to(device)
            reconstructions, latents = autoencoder(inputs)
            _, _, p2cp_mm = pc_shapes_eval(reconstructions, inputs, mean, std, to_mm=to_mm, pred=False, tgt=False)
            state.update(p2cp_mm=p2cp_mm)
            all_p2cp.append(p2cp_mm)
            all_latents.append(latents)
            frame_names.extend(name.split("_") for name in names)
        errors = torch.cat(all_p2cp)
        stats = state.error_stats()
        agg = torch.stack([stats["mean"], stats["std"], median_rows(errors), stats["min"], stats["max"]]).cpu().numpy()
        # nomograms: all L * 21 latent rows through the decoders and the denormalisation in one pass
        shapes = autoencoder.decoders(nomogram_latents(latent_size).to(device))
        nomograms, _, _ = pc_shapes_eval(shapes, shapes, mean, std, tgt=False, p2cp=False)
    errors = errors.cpu().numpy()
    latents = torch.cat(all_latents).cpu().numpy()

    _write_csv(os.path.join(save_to, "latent_space.csv"), [str(i) for i in range(1, latent_size + 1)], latents.tolist())
    np.save(os.path.join(save_to, "reconstruction_errors.npy"), errors)
    _write_csv(os.path.join(save_to, "reconstruction_errors.csv"), ["subject", "sequence", "frame"] + articulators,
               [name + row for name, row in zip(frame_names, errors.tolist())])
    _write_csv(os.path.join(save_to, "reconstruction_errors_agg.csv"), ["index"] + articulators,
               [[name] + row for name, row in zip(["mean", "std", "median", "min", "max"], agg.tolist())])
    np.save(os.path.join(save_to, "plots", "nomograms.npy"),
            nomograms.reshape(latent_size, -1, *nomograms.shape[1:]).cpu().numpy())


def main(database_name, datadir, encoders_filepath, decoders_filepath, batch_size, model_params, seq_dict, save_to, num_workers=0,
         clip_tails=True, synthetic=None, seed=0):
    device = torch.device("cuda", torch.cuda.current_device())
    dataset_config = DATASET_CONFIG[database_name]
    model_params = _resolve_indices(model_params)
    articulators_indices_dict = model_params["indices_dict"]
    articulators = sorted(articulators_indices_dict.keys())
    test_dataset = _make_dataset(datadir, database_name, seq_dict, articulators, clip_tails, synthetic, seed + 2)
    test_dataloader = DataLoader(test_dataset, batch_size=batch_size, shuffle=False, worker_init_fn=set_seeds,
                                 num_workers=num_workers)
    best_autoencoder = _load_autoencoder(model_params, encoders_filepath, decoders_filepath, device)
    plots_dir = os.path.join(save_to, "plots")
    os.makedirs(os.path.join(save_to, "test_outputs"), exist_ok=True)
    os.makedirs(plots_dir, exist_ok=True)
    loss_fn = RegularizedLatentsMSELoss2(indices_dict=articulators_indices_dict, alpha=0.1)
    info_test = run_multiart_autoencoder_test(epoch=0, model=best_autoencoder, dataloader=test_dataloader, criterion=loss_fn,
                                              dataset_config=dataset_config, plots_dir=plots_dir,
                                              indices_dict=articulators_indices_dict, device=device)
    with open(os.path.join(save_to, "test_results.json"), "w") as f:
        json.dump(info_test, f)
    return info_test


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="cfg_filepath")
    return parser.parse_args(argv)


def run(cfg):
    """The reference's __main__: main(**cfg), then evaluate_autoencoder on the same configuration."""
    info_test = main(**cfg)
    evaluate_autoencoder(cfg["database_name"], cfg["datadir"], DATASET_CONFIG[cfg["database_name"]], cfg["batch_size"],
                         cfg["seq_dict"], cfg["model_params"], cfg["encoders_filepath"], cfg["decoders_filepath"], cfg["save_to"],
                         num_workers=cfg.get("num_workers", 0), clip_tails=cfg.get("clip_tails", True),
                         synthetic=cfg.get("synthetic"), seed=cfg.get("seed", 0))
    return info_test


if __name__ == "__main__":
    args = parse_args()
    with open(args.cfg_filepath) as f:
        cfg = yaml.safe_load(f.read())
    print(run(cfg))
