####################################################################################################
#
# Train the model-free phoneme-to-articulation network on MI355X
#
# Entry point kept from the reference (train_phoneme_to_articulation.py): same CLI
#   python train_phoneme_to_articulation.py --config cfg.yaml [--mlflow URI --experiment NAME
#          --run_id ID --run_name NAME --checkpoint PATH]
# same YAML keys (= the keyword arguments of main()), same run_epoch() contract, same checkpoint dict.
# Extras: `datadir: synthetic` trains on SyntheticArtSpeechDataset; launched under torchrun
# (one process per GPU) every global batch is sharded by utterance and the flat gradient buffer is
# all-reduced over RCCL before the optimizer step; `loss: p2cp` trains on the mean point-to-closest-point distance (the
# reference's MeanP2CPDistance, metrics.py:27-46, the figure the model is selected and reported by) instead of the
# Euclidean distance.
#
####################################################################################################
import json
import logging
import os

import numpy as np
import torch
import torch.distributed as dist
from torch.optim import Adam
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.utils.data import DataLoader

from artspeech_amd import distributed as dp
from artspeech_amd.helpers import make_padding_mask, set_seeds
from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import (
    ArtSpeechDataset,
    HBMResidentDataset,
    SyntheticArtSpeechDataset,
    pad_sequence_collate_fn,
)
from artspeech_amd.phoneme_to_articulation.encoder_decoder.evaluation import run_test
from artspeech_amd.phoneme_to_articulation.encoder_decoder.metrics import P2CPDistance
from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
from artspeech_amd.phoneme_to_articulation.metrics import (EuclideanDistance, MeanP2CPDistance, masked_euclidean_loss,
                                                            masked_p2cp_loss)
from artspeech_amd.settings import DATASET_CONFIG, TRAIN, VALID
from artspeech_amd.training import (build_vocabulary, fit, load_checkpoint, mlflow_call, results_paths, run_cli,
                                    synthetic_size)


def _world():
    return (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)


def run_epoch(phase, epoch, model, dataloader, optimizer, criterion, fn_metrics=None, scheduler=None, device=None):
    """One pass over `dataloader` (reference :45-121).  Returns {"loss": mean, metric_name: mean, ...}."""
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    training = phase == TRAIN
    model.train() if training else model.eval()
    rank, world = _world()

    losses = []
    metrics_values = {name: [] for name in fn_metrics}
    # reduction "none" (the training configuration): criterion + mask + mean collapse into one kernel
    fused = None
    if isinstance(criterion, (EuclideanDistance, MeanP2CPDistance)) and getattr(torch, criterion.reduction_name, None) is None:
        fused = masked_euclidean_loss if isinstance(criterion, EuclideanDistance) else masked_p2cp_loss
    deferred = hasattr(model, "check_tokens")   # token-id check next to the loop's own loss.item() instead of a sync per forward
    keep_defer = getattr(model, "defer_token_check", False)
    if deferred:
        model.defer_token_check = True          # for this loop only: restored below, whatever happens
    try:
        info = _run_epoch_batches(phase, model, dataloader, optimizer, criterion, fn_metrics, scheduler, device, training, rank, world,
                                  losses, metrics_values, fused, deferred)
        if deferred:
            model.check_tokens()                # the normal path only: never over an error of the loop
        return info
    finally:
        if deferred:
            model.defer_token_check = keep_defer
            model._pending_ws = []              # nothing stays pending; after an error the flag words are dropped unread


def _run_epoch_batches(phase, model, dataloader, optimizer, criterion, fn_metrics, scheduler, device, training, rank, world, losses,
                       metrics_values, fused, deferred):
    for _, sentence, targets, lengths, _, _, _, _ in dataloader:
        n_valid_global = int(lengths.sum())
        if world > 1:  # every rank sees the same global batch (same sampler seed) and keeps its shard
            sentence, targets, lengths, n_valid_global = dp.shard_batch(sentence, targets, lengths, rank, world)
        sentence, targets = sentence.to(device), targets.to(device)
        optimizer.zero_grad()
        with torch.set_grad_enabled(training):
            outputs = model(sentence, lengths)
            if fused is not None:  # criterion + padding mask + mean in one kernel; shard losses sum to the global mean
                loss = fused(outputs, targets, lengths, n_valid_global=n_valid_global)
            else:      # the reference's expression (:86-90)
                loss = criterion(outputs, targets[:, :outputs.shape[1]])
                padding_mask = make_padding_mask(lengths)
                bs, max_len, num_articulators, features = loss.shape
                loss = loss.view(bs * max_len, num_articulators, features)
                loss = loss[padding_mask.view(bs * max_len).to(device)].mean()
            if training:
                loss.backward()
                if world > 1:
                    dp.all_reduce_flat(model.flat.grad)
                optimizer.step()
                if scheduler is not None:
                    scheduler.step()
            step_loss = loss.detach().clone()
            if world > 1:
                dp.all_reduce_flat(step_loss)
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].append(fn_metric(outputs, targets, lengths).item())
            losses.append(step_loss.item())
            if deferred:
                model.check_tokens()   # IndexError like nn.Embedding (reference models.py:135) for ids outside the vocabulary
    info = {"loss": float(np.mean(losses))}
    info.update({name: float(np.mean(vals)) for name, vals in metrics_values.items()})
    return info


def _make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, clip_tails, synthetic, seed):
    if datadir == "synthetic":
        n, cfg = synthetic_size(seq_dict, synthetic, "num_sentences", 64)
        return SyntheticArtSpeechDataset(n, vocabulary, articulators, seed=seed, database_name=database_name, **cfg)
    from artspeech_amd.helpers import sequences_from_dict
    return ArtSpeechDataset(datadir, database_name, sequences_from_dict(datadir, seq_dict), vocabulary, articulators,
                            clip_tails=clip_tails)


def main(datadir, database_name, num_epochs, batch_size, patience, learning_rate, weight_decay, train_seq_dict,
         valid_seq_dict, test_seq_dict, vocab_filepath, articulators, model_kwargs=None, num_workers=0, clip_tails=True,
         state_dict_filepath=None, checkpoint_filepath=None, seed=0, synthetic=None, results_dir=None, hbm_resident=False,
         loss="euclidean"):
    criteria = {"euclidean": EuclideanDistance, "p2cp": MeanP2CPDistance}
    if loss not in criteria:   # before the device is touched
        raise ValueError(f"loss must be 'euclidean' or 'p2cp', got {loss!r}")
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        backend = os.environ.get("ARTSPEECH_DIST_BACKEND", "nccl")  # "gloo": rehearsal with several ranks on one GPU
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) if backend == "nccl" else 0)
        dist.init_process_group(backend)
    rank, world = _world()
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}' (rank {rank}/{world})")
    results_dir, best_model_path, last_model_path, save_checkpoint_path = results_paths(results_dir, "artspeech_")

    vocabulary = build_vocabulary(vocab_filepath)

    model = ArtSpeech(len(vocabulary), len(articulators), **(model_kwargs or {}))
    if state_dict_filepath is not None:
        model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)
    dp.broadcast_parameters(model)
    if rank == 0:
        print(f"\nArtSpeech -- {model.total_parameters} parameters\n")
    mlflow_call("log_param", "num_network_params", model.total_parameters)

    loss_fn = criteria[loss](reduction="none")
    optimizer = Adam(model.parameters(), lr=learning_rate, weight_decay=weight_decay)
    scheduler = ReduceLROnPlateau(optimizer, factor=0.1, patience=10)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    def loader(seq_dict, shuffle, ds_seed):
        ds = _make_dataset(datadir, database_name, seq_dict, vocabulary, articulators, clip_tails, synthetic, ds_seed)
        if hbm_resident:   # YAML key `hbm_resident: true`: the data set lives in HBM, batches are collated on the device
            ds = HBMResidentDataset(ds, device)
            return DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=0, collate_fn=ds.collate, generator=gen)
        return DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, worker_init_fn=set_seeds,
                          collate_fn=pad_sequence_collate_fn, generator=gen)

    train_dataloader = loader(train_seq_dict, True, seed)
    valid_dataloader = loader(valid_seq_dict, False, seed + 1)
    fn_metrics = {"p2cp_mean": P2CPDistance(dataset_config=DATASET_CONFIG[database_name])}

    first_epoch, best_metric, epochs_since_best, checkpoint = load_checkpoint(checkpoint_filepath, model, optimizer, scheduler)
    best_model_path = checkpoint.get("best_model_path", best_model_path)   # a resumed run keeps writing where it started
    last_model_path = checkpoint.get("last_model_path", last_model_path)
    # the LR schedule follows the validation LOSS (:290), model selection follows p2cp_mean (:292-298)
    fit(range(first_epoch, num_epochs + 1),
        lambda epoch: run_epoch(TRAIN, epoch, model, train_dataloader, optimizer, loss_fn, device=device),
        lambda epoch: run_epoch(VALID, epoch, model, valid_dataloader, optimizer, loss_fn, fn_metrics=fn_metrics, device=device),
        metric="p2cp_mean", patience=patience, best_files=[(best_model_path, model.state_dict)],
        last_files=[(last_model_path, model.state_dict)], checkpoint_path=save_checkpoint_path,
        checkpoint_state=lambda: {"model": model.state_dict(), "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict(),
                                  "best_model_path": best_model_path, "last_model_path": last_model_path},
        best_metric=best_metric, epochs_since_best=epochs_since_best, plateau=scheduler, rank=rank)

    results = None
    if rank == 0:
        test_dataloader = loader(test_seq_dict, False, seed + 2)
        if os.path.exists(best_model_path):
            model.load_state_dict(torch.load(best_model_path, map_location="cpu"))
        results = run_test(epoch=0, model=model, dataloader=test_dataloader, criterion=loss_fn,
                           outputs_dir=os.path.join(results_dir, "test_outputs"), articulators=sorted(articulators),
                           device=device)
        with open(os.path.join(results_dir, "test_results.json"), "w") as f:
            json.dump(results, f, indent=1)
    if world > 1:
        dist.barrier()
    return results


if __name__ == "__main__":
    run_cli(main, "phoneme_to_articulation")
