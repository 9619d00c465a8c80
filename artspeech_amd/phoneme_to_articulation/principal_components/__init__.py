"""Principal-components method (reference phoneme_to_articulation/principal_components): the recurrent phoneme -> latent
components model (models/rnn.py), the multi-articulator autoencoders and their losses on the C ABI, and the autoencoder's
epoch loop (``run_autoencoder_epoch``, reference __init__.py:8-66)."""
import numpy as np
import torch

from ...settings import TRAIN


def run_autoencoder_epoch(phase, epoch, model, dataloader, optimizer, criterion, scheduler=None, fn_metrics=None, device=None):
    """One epoch of MultiArticulatorAutoencoder training / evaluation over (frame_names, inputs, sample_weights, phonemes)
    batches: criterion(outputs, latents, inputs, sample_weights) (RegularizedLatentsMSELoss2).  Returns {"loss": mean,
    metric: mean, ...} like the reference."""
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    training = phase == TRAIN
    model.train(training)
    losses = []
    metrics_values = {name: [] for name in fn_metrics}
    for _, inputs, sample_weights, _ in dataloader:
        inputs = inputs.to(device)
        sample_weights = sample_weights.to(device)
        optimizer.zero_grad()
        with torch.set_grad_enabled(training):
            outputs, latents = model(inputs)
            loss = criterion(outputs, latents, inputs, sample_weights)
            if training:
                loss.backward()
                optimizer.step()
                if scheduler is not None:
                    scheduler.step()
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].append(fn_metric(outputs, inputs).item())
        losses.append(loss.item())
    info = {"loss": float(np.mean(losses))}
    info.update({name: float(np.mean(values)) for name, values in metrics_values.items()})
    return info
