####################################################################################################
#
# Train the multi-articulator autoencoder of the principal-components method (reference
# train_principal_components_autoencoder.py) on the MI355X engine:
#   python train_principal_components_autoencoder.py --config cfg.yaml [--mlflow URI --experiment NAME
#          --run_id ID --run_name NAME --checkpoint checkpoint.pt]
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPrincipalComponentsAutoencoderDataset, sized by `synthetic:` and the sequence dicts' `num_frames`)
# and `results_dir`.  Writes best_encoders.pt / best_decoders.pt, last_encoders.pt / last_decoders.pt and
# checkpoint.pt like the reference, and ends with run_multiart_autoencoder_test on the test split (loss + p2cp_mm).
#
####################################################################################################
import argparse
import logging
import os
import random
import shutil
import tempfile

import numpy as np
import torch
import yaml
from torch.optim import Adam
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.utils.data import DataLoader

from artspeech_amd.helpers import make_indices_dict, sequences_from_dict, set_seeds
from artspeech_amd.phoneme_to_articulation.metrics import MeanP2CPDistance
from artspeech_amd.phoneme_to_articulation.principal_components import run_autoencoder_epoch
from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import run_multiart_autoencoder_test
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import (
    PrincipalComponentsAutoencoderDataset2,
    SyntheticPrincipalComponentsAutoencoderDataset,
)
from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
from artspeech_amd.phoneme_to_articulation.principal_components.models.autoencoder import MultiArticulatorAutoencoder
from artspeech_amd.settings import DATASET_CONFIG, TRAIN, VALID

try:  # mlflow is optional here (absent from the MI355X image): same flags, no-op logging
    import mlflow
except ImportError:
    mlflow = None


def _mlflow(fn, *args, **kwargs):
    if mlflow is not None:
        return getattr(mlflow, fn)(*args, **kwargs)


def reconstruction_error(outputs, targets, denorm_fn_dict, px_space=1, res=1):
    """Mean over articulators of the mean P2CP distance (mm) between denormalised outputs and targets (reference :40-64);
    works on copies (the reference denormalises the batch tensors in place)."""
    p2cp_fn = MeanP2CPDistance(reduction="mean")
    batch_size, num_articulators, n_features = outputs.shape
    outputs = outputs.detach().clone().reshape(batch_size, num_articulators, 2, n_features // 2)
    targets = targets.detach().clone().reshape(batch_size, num_articulators, 2, n_features // 2)
    p2cps = []
    for i, (_, denorm_fn) in enumerate(denorm_fn_dict.items()):
        outputs[:, i, :] = denorm_fn(outputs[:, i, :])
        targets[:, i, :] = denorm_fn(targets[:, i, :])
        p2cp = p2cp_fn(outputs[:, i, :].permute(0, 2, 1), targets[:, i, :].permute(0, 2, 1))
        p2cps.append((p2cp * px_space * res).item())
    return torch.tensor(np.mean(p2cps))


def _make_dataset(datadir, database_name, seq_dict, articulators, clip_tails, synthetic, seed):
    if datadir == "synthetic":
        cfg = dict(synthetic or {})
        n = (seq_dict or {}).get("num_frames", cfg.pop("num_frames", 256))
        cfg.pop("num_frames", None)
        return SyntheticPrincipalComponentsAutoencoderDataset(n, articulators, seed=seed, database_name=database_name, **cfg)
    return PrincipalComponentsAutoencoderDataset2(database_name=database_name, datadir=datadir,
                                                  sequences=sequences_from_dict(datadir, seq_dict), articulators=articulators,
                                                  clip_tails=clip_tails)


def main(database_name, datadir, n_epochs, batch_size, patience, learning_rate, weight_decay, train_seq_dict, valid_seq_dict,
         test_seq_dict, model_params, alpha, num_workers=0, clip_tails=True, state_dict_fpath=None, checkpoint_filepath=None,
         seed=0, synthetic=None, results_dir=None):
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    results_dir = results_dir or RESULTS_DIR
    os.makedirs(results_dir, exist_ok=True)
    best_encoders_path = os.path.join(results_dir, "best_encoders.pt")
    best_decoders_path = os.path.join(results_dir, "best_decoders.pt")
    last_encoders_path = os.path.join(results_dir, "last_encoders.pt")
    last_decoders_path = os.path.join(results_dir, "last_decoders.pt")
    save_checkpoint_path = os.path.join(results_dir, "checkpoint.pt")

    model_params = dict(model_params)
    indices_dict = model_params["indices_dict"]
    if isinstance(list(indices_dict.values())[0], int):
        indices_dict = make_indices_dict(indices_dict)
        model_params["indices_dict"] = indices_dict
    articulators = sorted(indices_dict.keys())

    autoencoder = MultiArticulatorAutoencoder(**model_params)
    if state_dict_fpath is not None:
        autoencoder.load_state_dict(torch.load(state_dict_fpath, map_location=device))
    autoencoder.to(device)
    print(f"\nMultiArticulatorAutoencoder -- {autoencoder.total_parameters} parameters\n")
    # the reference logs `model.total_parameters` here, an undefined name (NameError): the autoencoder's count is meant
    _mlflow("log_param", "num_network_params", autoencoder.total_parameters)

    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    dataset_config = DATASET_CONFIG[database_name]

    def loader(seq_dict, shuffle, ds_seed):
        ds = _make_dataset(datadir, database_name, seq_dict, articulators, clip_tails, synthetic, ds_seed)
        return ds, DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, worker_init_fn=set_seeds,
                              generator=gen)

    train_dataset, train_dataloader = loader(train_seq_dict, True, seed)
    _, valid_dataloader = loader(valid_seq_dict, True, seed + 1)

    loss_fn = RegularizedLatentsMSELoss2(indices_dict=indices_dict, alpha=alpha)
    optimizer = Adam(autoencoder.parameters(), lr=learning_rate, weight_decay=weight_decay)
    scheduler = ReduceLROnPlateau(optimizer, factor=0.1, patience=10, min_lr=learning_rate / 1000)
    denorm_fn_dict = {articulator: denorm_fn.inverse for articulator, denorm_fn in train_dataset.normalize.items()}
    metrics = {"p2cp_mm": lambda outputs, targets: reconstruction_error(
        outputs, targets, denorm_fn_dict=denorm_fn_dict, px_space=dataset_config.PIXEL_SPACING, res=dataset_config.RES)}

    best_metric = np.inf
    epochs_since_best = 0
    epochs = range(1, n_epochs + 1)
    if checkpoint_filepath is not None:
        checkpoint = torch.load(checkpoint_filepath, map_location=device)
        autoencoder.load_state_dict(checkpoint["model"])
        optimizer.load_state_dict(checkpoint["optimizer"])
        scheduler.load_state_dict(checkpoint["scheduler"])
        epoch = checkpoint["epoch"] + 1
        epochs = range(epoch, n_epochs + 1)
        best_metric = checkpoint["best_metric"]
        epochs_since_best = checkpoint["epochs_since_best"]
        logging.info(f"Loaded checkpoint -- training from epoch {epoch}, best metric {best_metric} "
                     f"seen {epochs_since_best} epochs ago.")

    history = []
    for epoch in epochs:
        info_train = run_autoencoder_epoch(phase=TRAIN, epoch=epoch, model=autoencoder, dataloader=train_dataloader,
                                           optimizer=optimizer, criterion=loss_fn, device=device)
        _mlflow("log_metrics", {f"train_{m}": v for m, v in info_train.items()}, step=epoch)
        info_valid = run_autoencoder_epoch(phase=VALID, epoch=epoch, model=autoencoder, dataloader=valid_dataloader,
                                           optimizer=optimizer, criterion=loss_fn, fn_metrics=metrics, device=device)
        _mlflow("log_metrics", {f"valid_{m}": v for m, v in info_valid.items()}, step=epoch)
        history.append({"epoch": epoch, "train": info_train, "valid": info_valid})

        if info_valid["p2cp_mm"] < best_metric:
            best_metric = info_valid["p2cp_mm"]
            epochs_since_best = 0
            torch.save(autoencoder.encoders.state_dict(), best_encoders_path)
            torch.save(autoencoder.decoders.state_dict(), best_decoders_path)
            _mlflow("log_artifact", best_encoders_path)
            _mlflow("log_artifact", best_decoders_path)
        else:
            epochs_since_best += 1
        torch.save(autoencoder.encoders.state_dict(), last_encoders_path)
        torch.save(autoencoder.decoders.state_dict(), last_decoders_path)
        _mlflow("log_artifact", last_encoders_path)
        _mlflow("log_artifact", last_decoders_path)
        checkpoint = {"epoch": epoch, "model": autoencoder.state_dict(), "optimizer": optimizer.state_dict(),
                      "scheduler": scheduler.state_dict(), "best_metric": float(best_metric), "epochs_since_best": epochs_since_best,
                      "best_encoders_path": best_encoders_path, "best_decoders_path": best_decoders_path,
                      "last_encoders_path": last_encoders_path, "last_decoders_path": last_decoders_path}
        torch.save(checkpoint, save_checkpoint_path)
        _mlflow("log_artifact", save_checkpoint_path)
        print(f"\nFinished training epoch {epoch}\nBest metric: {best_metric}, Epochs since best: {epochs_since_best}\n")
        if epochs_since_best > patience:
            break

    # test split: the best encoders / decoders through the test harness, as the reference does (:298): the
    # latent covariance per articulator goes to results_dir
    _, test_dataloader = loader(test_seq_dict, False, seed + 2)
    best_autoencoder = MultiArticulatorAutoencoder(**model_params)
    best_autoencoder.encoders.load_state_dict(torch.load(best_encoders_path, map_location=device))
    best_autoencoder.decoders.load_state_dict(torch.load(best_decoders_path, map_location=device))
    best_autoencoder.to(device)
    info_test = run_multiart_autoencoder_test(epoch=0, model=best_autoencoder, dataloader=test_dataloader, criterion=loss_fn,
                                              dataset_config=dataset_config, plots_dir=results_dir, indices_dict=indices_dict,
                                              fn_metrics=metrics, device=device)
    _mlflow("log_metrics", {f"test_{m}": v for m, v in info_test.items()}, step=0)
    return {"history": history, "test": info_test, "results_dir": results_dir}


TMP_DIR = tempfile.mkdtemp(prefix="artspeech_pc_ae_")
RESULTS_DIR = os.path.join(TMP_DIR, "results")

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    parser.add_argument("--mlflow", dest="mlflow_tracking_uri", default=None)
    parser.add_argument("--experiment", dest="experiment_name", default="multiarticulator_autoencoder")
    parser.add_argument("--run_id", dest="run_id", default=None)
    parser.add_argument("--run_name", dest="run_name", default=None)
    parser.add_argument("--checkpoint", dest="checkpoint_filepath", default=None)
    args = parser.parse_args()
    seed = 0
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    if mlflow is not None and args.mlflow_tracking_uri is not None:
        mlflow.set_tracking_uri(args.mlflow_tracking_uri)
        mlflow.set_experiment(args.experiment_name)
    try:
        main(**cfg, checkpoint_filepath=args.checkpoint_filepath, seed=seed)
    finally:
        shutil.rmtree(TMP_DIR, ignore_errors=True)
