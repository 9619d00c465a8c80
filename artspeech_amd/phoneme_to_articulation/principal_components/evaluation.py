"""Test loops of the principal-components method on MI355X (reference
phoneme_to_articulation/principal_components/evaluation.py:183-443) and the device pieces they and the autoencoder's evaluation
share: ``pc_shapes_eval`` (denormalise + upper-incisor injection + MeanP2CPDistance in mm, one launch, csrc/pc_eval.hip) and
``PCEvalState`` (running fp64 statistics of a split, updated on the device with no host read per batch).

The plots of the reference (heat maps of the covariance, per-frame contour plots) are not produced: seaborn and matplotlib are
not part of this engine; the arrays behind them are written."""
import os

import numpy as np
import torch

from ... import _lib
from ...tract_variables import REQUIRED_ARTICULATORS, UPPER_INCISOR
from .. import save_outputs
from ..encoder_decoder.evaluation import _write_tract_variables

MAX_LATENT = 64   # as_pc_eval_accumulate's limit (k_max of the PCA)


def denorm_tables(normalize_dict, articulators, device):
    """(mean, std), each (A, 2, N) float32 on ``device``: the Normalize statistics of the articulators in the given order,
    uploaded once per run (Normalize.inverse clones and uploads both at every call)."""
    mean = torch.stack([normalize_dict[a].mean.float() for a in articulators]).to(device).contiguous()
    std = torch.stack([normalize_dict[a].std.float() for a in articulators]).to(device).contiguous()
    return mean, std


def _lengths_dev(lengths, device):
    return torch.as_tensor(lengths, dtype=torch.int32).to(device).contiguous()


def pc_shapes_eval(shapes, targets, mean, std, to_mm=1.0, lengths=None, reference=None, ref_idx=-1, pred=True, tgt=True, p2cp=True):
    """shapes (*lead, A, 2 N) normalised predictions, targets (*lead, A, 2, N) (or (*lead, A, 2 N)) normalised, mean / std
    (A, 2, N) -> (pred_out, tgt_out (*lead, A + (ref_idx >= 0), 2, N), p2cp_mm (*lead, A)); an output not asked for is None.
    With ``lengths`` (B,) the leading shape is (B, T) and the frames t >= lengths[b] come out as zeros.  ``reference``
    (*lead, 1, 2, N) is copied in at channel ``ref_idx``.  The inputs are not modified."""
    _lib.require_gpu(shapes, "shapes")
    A, N = mean.shape[0], mean.shape[2]
    lead = tuple(shapes.shape[:-2])
    rows = int(np.prod(lead)) if lead else 1
    if tuple(shapes.shape[-2:]) != (A, 2 * N) or targets.numel() != rows * A * 2 * N:
        raise ValueError(f"pc_shapes_eval: shapes {tuple(shapes.shape)} / targets {tuple(targets.shape)} do not match the "
                         f"statistics ({A}, 2, {N})")
    dev = shapes.device
    s = shapes.detach().contiguous().float()
    t = targets.detach().to(dev).contiguous().float()
    T, len_dev = 0, None
    if lengths is not None:
        if len(lead) != 2 or len(lengths) != lead[0]:
            raise ValueError("pc_shapes_eval: lengths need (B, T, A, 2 N) shapes")
        T, len_dev = lead[1], _lengths_dev(lengths, dev)
    ref = None
    if ref_idx >= 0:
        ref = reference.detach().to(dev).contiguous().float()
        if ref.numel() != rows * 2 * N:
            raise ValueError(f"pc_shapes_eval: reference {tuple(reference.shape)} is not (*lead, 1, 2, {N})")
    C = A + (1 if ref_idx >= 0 else 0)
    pred_out = torch.empty((*lead, C, 2, N), dtype=torch.float32, device=dev) if pred else None
    tgt_out = torch.empty((*lead, C, 2, N), dtype=torch.float32, device=dev) if tgt else None
    p2cp_mm = torch.empty((*lead, A), dtype=torch.float32, device=dev) if p2cp else None
    _lib.call("as_pc_shapes_eval", s, t, mean, std, len_dev, T, ref, int(ref_idx), rows, A, N, float(to_mm), pred_out, tgt_out, p2cp_mm)
    return pred_out, tgt_out, p2cp_mm


class PCEvalState:
    """Running statistics of a split on the device: per-articulator count / mean / M2 / min / max of the errors in mm and count
    / mean / co-moments of the latents, fp64, merged batch by batch (Chan) by as_pc_eval_accumulate."""

    def __init__(self, device, n_articulators=0, latent_size=0):
        self.A, self.L = int(n_articulators), int(latent_size)
        self.errors = torch.zeros(5, self.A, dtype=torch.float64, device=device) if self.A else None
        self.latents = torch.zeros(1 + self.L + self.L * self.L, dtype=torch.float64, device=device) if self.L else None

    def update(self, p2cp_mm=None, latents=None, lengths=None):
        """p2cp_mm (*lead, A) and / or latents (*lead, L); with ``lengths`` (B,) the leading shape is (B, T)."""
        first = p2cp_mm if p2cp_mm is not None else latents
        _lib.require_gpu(first, "p2cp_mm / latents")
        lead = tuple(first.shape[:-1])
        rows = int(np.prod(lead)) if lead else 1
        if p2cp_mm is not None:
            if self.errors is None or p2cp_mm.shape[-1] != self.A or tuple(p2cp_mm.shape[:-1]) != lead:
                raise ValueError(f"PCEvalState.update: p2cp_mm {tuple(p2cp_mm.shape)} does not match {self.A} articulators")
            p2cp_mm = p2cp_mm.detach().contiguous().float()
        if latents is not None:
            if self.latents is None or latents.shape[-1] != self.L or tuple(latents.shape[:-1]) != lead:
                raise ValueError(f"PCEvalState.update: latents {tuple(latents.shape)} do not match latent size {self.L}")
            latents = latents.detach().contiguous().float()
        T, len_dev = 0, None
        if lengths is not None:
            if len(lead) != 2 or len(lengths) != lead[0]:
                raise ValueError("PCEvalState.update: lengths need (B, T, ...) inputs")
            T, len_dev = lead[1], _lengths_dev(lengths, first.device)
        _lib.call("as_pc_eval_accumulate", p2cp_mm, self.A, self.errors, latents, self.L, self.latents, rows, len_dev, T)

    def covariance(self):
        """(L, L) fp64 on the device: M2 / (n - 1), torch.cov of the concatenated latents."""
        return self.latents[1 + self.L:].view(self.L, self.L) / (self.latents[0] - 1)

    def latent_mean(self):
        return self.latents[1:1 + self.L]

    def error_stats(self):
        """{"count", "mean", "std" (ddof = 1, pandas), "min", "max"}: (A,) fp64 on the device."""
        count, mean, m2, lo, hi = self.errors
        return {"count": count, "mean": mean, "std": torch.sqrt(m2 / (count - 1)), "min": lo, "max": hi}


def median_rows(errors):
    """(frames, A) -> (A,) fp64: pandas' median (the mean of the two middle values for an even count); one sort, at the end of
    a split."""
    srt = torch.sort(errors.double(), dim=0).values
    n = srt.shape[0]
    return (srt[(n - 1) // 2] + srt[n // 2]) / 2


def run_multiart_autoencoder_test(epoch, model, dataloader, criterion, dataset_config, outputs_dir=None, plots_dir=None,
                                  indices_dict=None, fn_metrics=None, device=None):
    """Test pass of MultiArticulatorAutoencoder (reference :183-280).  Returns {"loss": mean of the per-batch losses}; the
    reference evaluates ``fn_metrics`` and drops the values, here their means are added to the dict (nothing is added when
    ``fn_metrics`` is None).  The loss sum and the latent co-moments accumulate on the device; one host read after the loop.
    With ``plots_dir``: covariance_matrix.npy, or covariance_matrix_{articulator}.npy per entry of ``indices_dict``
    (cov[indices][:, indices] of the covariance of all latents, float32 like torch.cov's).  The heat-map images are not produced
    (seaborn is not part of this engine).  ``outputs_dir`` asks for the per-frame matplotlib plots and raises."""
    if outputs_dir is not None:
        raise NotImplementedError("run_multiart_autoencoder_test: outputs_dir asks for per-frame contour plots (matplotlib and "
                                  "the MRI data stack), which this engine does not produce")
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    model.eval()
    latent_size = model.latent_size
    if latent_size > MAX_LATENT:
        raise RuntimeError(f"run_multiart_autoencoder_test: latent size {latent_size} exceeds {MAX_LATENT}")
    state = PCEvalState(device, latent_size=latent_size)
    loss_sum = torch.zeros((), dtype=torch.float64, device=device)
    n_batches = 0
    metrics_values = {name: [] for name in fn_metrics}
    for _, inputs, sample_weights, _ in dataloader:
        inputs = inputs.to(device)
        sample_weights = sample_weights.to(device)
        with torch.no_grad():
            outputs, latents = model(inputs)
            loss_sum += criterion(outputs, latents, inputs, sample_weights).double()
            for name, fn_metric in fn_metrics.items():
                metrics_values[name].extend(float(v) for v in torch.as_tensor(fn_metric(outputs, inputs)).flatten())
            state.update(latents=latents)
        n_batches += 1
    if n_batches == 0:
        raise ValueError("run_multiart_autoencoder_test: empty dataloader")
    cov = state.covariance().float().cpu()
    if plots_dir:
        os.makedirs(plots_dir, exist_ok=True)
        if indices_dict is None:
            np.save(os.path.join(plots_dir, "covariance_matrix.npy"), cov.numpy())
        else:
            for articulator, indices in indices_dict.items():
                np.save(os.path.join(plots_dir, f"covariance_matrix_{articulator}.npy"), cov[indices][:, indices].numpy())
    info = {"loss": float(loss_sum.item() / n_batches)}
    info.update({name: float(np.mean(values)) for name, values in metrics_values.items()})
    return info


def run_phoneme_to_principal_components_test(epoch, model, dataloader, criterion, fn_metrics=None, outputs_dir=None,
                                             decode_transform=None, device=None):
    """Test pass of the phoneme -> components model (reference :283-443).  Returns {"loss", **metrics} (means over the
    batches).  With ``outputs_dir``: per batch the components are decoded (``decode_transform``), denormalised with the upper
    incisor injected at its sorted position when it is not among the articulators (one as_pc_shapes_eval launch),
    ``tract_variables.csv`` is written per sentence when the required articulators are there (and the contours have the 50
    points the tract variables slice), and save_outputs(..., regularize_out=False) dumps the contours.  Unlike the reference and
    DecoderMeanP2CPDistance2, the batch's ``targets`` are not modified."""
    if device is None:
        device = torch.device("cuda")
    fn_metrics = fn_metrics or {}
    model.eval()
    articulators = list(dataloader.dataset.articulators)
    tables = None
    losses = []
    metrics_values = {name: [] for name in fn_metrics}
    for names, inputs, targets, lengths, phonemes, critical_masks, reference_arrays, frames, voicing in dataloader:
        inputs = inputs.to(device)
        targets = targets.to(device)
        reference_arrays = reference_arrays.to(device)
        voicing = voicing.to(device)
        with torch.no_grad():
            outputs = model(inputs, lengths)
            loss = criterion(outputs, targets, reference_arrays, lengths, critical_masks, voicing)
            losses.append(loss)
            for name, fn_metric in fn_metrics.items():
                # the reference's metric denormalises the targets it is given in place: it gets a copy
                metrics_values[name].append(torch.as_tensor(fn_metric(outputs, targets.clone(), lengths)))
            if outputs_dir is None:
                continue
            epoch_outputs_dir = os.path.join(outputs_dir, str(epoch))
            os.makedirs(epoch_outputs_dir, exist_ok=True)
            if tables is None:
                tables = denorm_tables(dataloader.dataset.normalize, articulators, device)
            pred_shapes = decode_transform(outputs)   # (B, T, A, 2 N)
            if UPPER_INCISOR not in articulators:
                tv_articulators = sorted(articulators + [UPPER_INCISOR])
                ref_idx = tv_articulators.index(UPPER_INCISOR)
            else:
                tv_articulators, ref_idx = articulators, -1
            pred_out, tgt_out, _ = pc_shapes_eval(pred_shapes, targets, *tables, lengths=lengths, reference=reference_arrays,
                                                  ref_idx=ref_idx, p2cp=False)
            if all(a in tv_articulators for a in REQUIRED_ARTICULATORS) and pred_out.shape[-1] >= 50:
                _write_tract_variables(epoch_outputs_dir, names, frames, pred_out, tgt_out, lengths, phonemes, tv_articulators)
            save_outputs(names, frames, pred_out, tgt_out, lengths, phonemes, tv_articulators, epoch_outputs_dir,
                         regularize_out=False)
    if not losses:
        raise ValueError("run_phoneme_to_principal_components_test: empty dataloader")
    info = {"loss": float(torch.stack([l.detach().double().reshape(()) for l in losses]).mean().item())}
    info.update({name: float(torch.stack([v.detach().double().reshape(()).to(device) for v in values]).mean().item())
                 for name, values in metrics_values.items()})
    return info
