####################################################################################################
#
# Train the autoencoder-based phoneme-to-articulation method (reference
# train_phoneme_to_principal_components.py) on the MI355X engine:
#   python train_phoneme_to_principal_components.py --config cfg.yaml [--mlflow URI --experiment NAME
#          --run_id ID --run_name NAME --checkpoint checkpoint.pt]
# The YAML keys are the keyword arguments of main() (the reference's), plus the extras `datadir: synthetic`
# (SyntheticPrincipalComponentsPhonemeToArticulationDataset, sized by `synthetic:` and the sequence dicts'
# `num_sentences`) and `results_dir`.  The frozen encoder / decoder come from train_principal_components_autoencoder.py
# (best_encoders.pt / best_decoders.pt).  Writes best_model.pt, last_model.pt and checkpoint.pt like the reference and
# ends with run_phoneme_to_principal_components_test on the test split (loss + p2cp_mean).
#
####################################################################################################
import logging

import numpy as np
import torch
from torch.optim import Adam
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.utils.data import DataLoader

from artspeech_amd.helpers import make_indices_dict, sequences_from_dict, set_seeds
from artspeech_amd.phoneme_recognition import DeepSpeech2
from artspeech_amd.phoneme_to_articulation import RNNType
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import (
    PrincipalComponentsPhonemeToArticulationDataset2,
    SyntheticPrincipalComponentsPhonemeToArticulationDataset,
    pad_sequence_collate_fn,
)
from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import run_phoneme_to_principal_components_test
from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
from artspeech_amd.phoneme_to_articulation.principal_components.metrics import DecoderMeanP2CPDistance2
from artspeech_amd.phoneme_to_articulation.principal_components.models import (DecoderType, EncoderType,
                                                                               PrincipalComponentsArtSpeech)
from artspeech_amd.settings import DATASET_CONFIG, TRAIN, VALID
from artspeech_amd.training import (build_vocabulary, fit, load_checkpoint, load_json, mlflow_call, results_paths, run_cli,
                                    synthetic_size)


def run_epoch(phase, epoch, model, dataloader, optimizer, criterion, scheduler=None, fn_metrics=None, device=None):
    """One epoch over pad_sequence_collate_fn batches (reference :59-141): criterion(outputs, targets, reference_arrays,
    lengths, critical_masks, voicing) = AutoencoderLoss2; fn_metrics(outputs, targets, lengths)."""
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    training = phase == TRAIN
    model.train(training)
    losses = []
    metrics_values = {name: [] for name in fn_metrics}
    for _, inputs, targets, len_inputs, _, critical_masks, reference_arrays, _, voicing in dataloader:
        inputs = inputs.to(device)
        targets = targets.to(device)
        reference_arrays = reference_arrays.to(device)
        voicing = voicing.to(device)
        optimizer.zero_grad()
        with torch.set_grad_enabled(training):
            outputs = model(inputs, len_inputs)
            loss = criterion(outputs, targets, reference_arrays, len_inputs, critical_masks, voicing)
            if training:
                loss.backward()
                optimizer.step()
                if scheduler is not None:
                    scheduler.step()
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].append(fn_metric(outputs, targets, len_inputs).item())
            losses.append(loss.item())
    info = {"loss": float(np.mean(losses))}
    info.update({name: float(np.mean(values)) for name, values in metrics_values.items()})
    return info


def _make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, TV_to_phoneme_map, clip_tails, voiced_tokens,
                  synthetic, seed):
    if datadir == "synthetic":
        n, cfg = synthetic_size(seq_dict, synthetic, "num_sentences", 32)
        return SyntheticPrincipalComponentsPhonemeToArticulationDataset(n, vocabulary, articulators, TV_to_phoneme_map, seed=seed,
                                                                        database_name=database_name, voiced_tokens=voiced_tokens,
                                                                        **cfg)
    return PrincipalComponentsPhonemeToArticulationDataset2(database_name, datadir, sequences_from_dict(datadir, seq_dict),
                                                            vocabulary, articulators, TV_to_phoneme_map, clip_tails=clip_tails,
                                                            voiced_tokens=voiced_tokens)


def main(database_name, datadir, num_epochs, batch_size, patience, learning_rate, weight_decay, train_seq_dict, valid_seq_dict,
         test_seq_dict, indices_dict, vocab_filepath, modelkwargs, autoencoder_kwargs, encoder_state_dict_filepath,
         decoder_state_dict_filepath, encoder_type="AE", decoder_type="AE", rnn_type="GRU", beta1=1.0, beta2=1.0, beta3=1.0,
         beta4=0.0, rescale_factor=1.0, recognizer_filepath=None, recognizer_params=None, voicing_filepath=None,
         TV_to_phoneme_map=None, clip_tails=True, num_workers=0, state_dict_filepath=None, checkpoint_filepath=None, seed=0,
         synthetic=None, results_dir=None):
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    dataset_config = DATASET_CONFIG[database_name]
    results_dir, best_model_path, last_model_path, save_checkpoint_path = results_paths(results_dir, "artspeech_pc_")

    vocabulary = build_vocabulary(vocab_filepath)
    voiced_tokens = load_json(voicing_filepath)
    if isinstance(list(indices_dict.values())[0], int):
        indices_dict = make_indices_dict(indices_dict)
    articulators = sorted(indices_dict.keys())

    model = PrincipalComponentsArtSpeech(vocab_size=len(vocabulary), indices_dict=indices_dict, rnn=RNNType[rnn_type.upper()],
                                         **modelkwargs)
    if state_dict_filepath is not None:
        model.load_state_dict(torch.load(state_dict_filepath, map_location=device))
    model.to(device)
    print(f"\nPrincipalComponentsArtSpeech -- {model.total_parameters} parameters\n")
    mlflow_call("log_param", "num_network_params", model.total_parameters)

    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    def loader(seq_dict, shuffle, ds_seed):
        ds = _make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, TV_to_phoneme_map, clip_tails,
                           voiced_tokens, synthetic, ds_seed)
        return ds, DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, worker_init_fn=set_seeds,
                              collate_fn=pad_sequence_collate_fn, generator=gen)

    train_dataset, train_dataloader = loader(train_seq_dict, True, seed)
    _, valid_dataloader = loader(valid_seq_dict, True, seed + 1)

    TVs = sorted((TV_to_phoneme_map or {}).keys())
    if recognizer_filepath:   # frozen: the recognition term differentiates through its input only (reference :267-276)
        recognizer = DeepSpeech2(num_classes=len(vocabulary), **(recognizer_params or {}))
        recognizer.load_state_dict(torch.load(recognizer_filepath, map_location=device))
        recognizer.to(device)
        for p in recognizer.parameters():
            p.requires_grad = False
    else:
        recognizer = None
    denorm_fn = {articulator: normalize.inverse for articulator, normalize in train_dataset.normalize.items()}
    encoder_cls = EncoderType[encoder_type.upper()].value
    decoder_cls = DecoderType[decoder_type.upper()].value
    loss_fn = AutoencoderLoss2(indices_dict=indices_dict, TVs=TVs, device=device,
                               encoder_state_dict_filepath=encoder_state_dict_filepath,
                               decoder_state_dict_filepath=decoder_state_dict_filepath, denormalize_fn=denorm_fn, beta1=beta1,
                               beta2=beta2, beta3=beta3, beta4=beta4, rescale_factor=rescale_factor, encoder_cls=encoder_cls,
                               decoder_cls=decoder_cls, recognizer=recognizer, **autoencoder_kwargs)
    optimizer = Adam(model.parameters(), lr=learning_rate, weight_decay=weight_decay)
    scheduler = ReduceLROnPlateau(optimizer, factor=0.1, patience=10)
    fn_metrics = {"p2cp_mean": DecoderMeanP2CPDistance2(
        dataset_config=dataset_config, decoder_state_dict_filepath=decoder_state_dict_filepath, indices_dict=indices_dict,
        autoencoder_kwargs=autoencoder_kwargs, device=device, decoder_cls=decoder_cls,
        denorm_fns={articulator: train_dataset.normalize[articulator].inverse for articulator in articulators})}

    first_epoch, best_metric, epochs_since_best, _ = load_checkpoint(checkpoint_filepath, model, optimizer, scheduler,
                                                                     map_location=device)
    history = fit(range(first_epoch, num_epochs + 1),
                  lambda epoch: run_epoch(phase=TRAIN, epoch=epoch, model=model, dataloader=train_dataloader, optimizer=optimizer,
                                          criterion=loss_fn, device=device),
                  lambda epoch: run_epoch(phase=VALID, epoch=epoch, model=model, dataloader=valid_dataloader, optimizer=optimizer,
                                          criterion=loss_fn, device=device, fn_metrics=fn_metrics),
                  metric="p2cp_mean", patience=patience, best_files=[(best_model_path, model.state_dict)],
                  last_files=[(last_model_path, model.state_dict)], checkpoint_path=save_checkpoint_path,
                  checkpoint_state=lambda: {"model": model.state_dict(), "optimizer": optimizer.state_dict(),
                                            "scheduler": scheduler.state_dict(), "best_model_path": best_model_path,
                                            "last_model_path": last_model_path},
                  best_metric=best_metric, epochs_since_best=epochs_since_best, plateau=scheduler)

    # test split: the best model through the test harness, as the reference does (:455), without the per-sentence dumps
    _, test_dataloader = loader(test_seq_dict, False, seed + 2)
    best_model = PrincipalComponentsArtSpeech(vocab_size=len(vocabulary), indices_dict=indices_dict,
                                              rnn=RNNType[rnn_type.upper()], **modelkwargs)
    best_model.load_state_dict(torch.load(best_model_path, map_location=device))
    best_model.to(device)
    info_test = run_phoneme_to_principal_components_test(epoch=0, model=best_model, dataloader=test_dataloader, criterion=loss_fn,
                                                         fn_metrics=fn_metrics, device=device)
    mlflow_call("log_metrics", {f"test_{m}": v for m, v in info_test.items()}, step=0)
    return {"history": history, "test": info_test, "results_dir": results_dir}


if __name__ == "__main__":
    run_cli(main, "phoneme_to_principal_components")
