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
import logging

import numpy as np
import torch
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
from artspeech_amd.training import fit, load_checkpoint, mlflow_call, results_paths, run_cli, synthetic_size


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
        n, cfg = synthetic_size(seq_dict, synthetic, "num_frames", 256)
        return SyntheticPrincipalComponentsAutoencoderDataset(n, articulators, seed=seed, database_name=database_name, **cfg)
    return PrincipalComponentsAutoencoderDataset2(database_name=database_name, datadir=datadir,
                                                  sequences=sequences_from_dict(datadir, seq_dict), articulators=articulators,
                                                  clip_tails=clip_tails)


def main(database_name, datadir, n_epochs, batch_size, patience, learning_rate, weight_decay, train_seq_dict, valid_seq_dict,
         test_seq_dict, model_params, alpha, num_workers=0, clip_tails=True, state_dict_fpath=None, checkpoint_filepath=None,
         seed=0, synthetic=None, results_dir=None):
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    (results_dir, best_encoders_path, best_decoders_path, last_encoders_path, last_decoders_path,
     save_checkpoint_path) = results_paths(results_dir, "artspeech_pc_ae_", ("best_encoders.pt", "best_decoders.pt", "last_encoders.pt",
                                                                              "last_decoders.pt", "checkpoint.pt"))

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
    mlflow_call("log_param", "num_network_params", autoencoder.total_parameters)

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

    # the scheduler is built and saved but never stepped, as in the reference
    first_epoch, best_metric, epochs_since_best, _ = load_checkpoint(checkpoint_filepath, autoencoder, optimizer, scheduler,
                                                                     map_location=device)
    encoders, decoders = autoencoder.encoders.state_dict, autoencoder.decoders.state_dict
    history = fit(range(first_epoch, n_epochs + 1),
                  lambda epoch: run_autoencoder_epoch(phase=TRAIN, epoch=epoch, model=autoencoder, dataloader=train_dataloader,
                                                      optimizer=optimizer, criterion=loss_fn, device=device),
                  lambda epoch: run_autoencoder_epoch(phase=VALID, epoch=epoch, model=autoencoder, dataloader=valid_dataloader,
                                                      optimizer=optimizer, criterion=loss_fn, fn_metrics=metrics, device=device),
                  metric="p2cp_mm", patience=patience, best_files=[(best_encoders_path, encoders), (best_decoders_path, decoders)],
                  last_files=[(last_encoders_path, encoders), (last_decoders_path, decoders)], checkpoint_path=save_checkpoint_path,
                  checkpoint_state=lambda: {"model": autoencoder.state_dict(), "optimizer": optimizer.state_dict(),
                                            "scheduler": scheduler.state_dict(), "best_encoders_path": best_encoders_path,
                                            "best_decoders_path": best_decoders_path, "last_encoders_path": last_encoders_path,
                                            "last_decoders_path": last_decoders_path},
                  best_metric=best_metric, epochs_since_best=epochs_since_best)

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
    mlflow_call("log_metrics", {f"test_{m}": v for m, v in info_test.items()}, step=0)
    return {"history": history, "test": info_test, "results_dir": results_dir}


if __name__ == "__main__":
    run_cli(main, "multiarticulator_autoencoder")
