"""Losses of the principal-components method (reference principal_components/losses.py).

``CriticalLoss`` (:23-99): for every
tract variable the minimum pairwise distance between two predicted articulators per frame, averaged over the frames where
the constriction is critical.  The reference materialises ``cdist`` (bs, T, N, N) per variable and takes ``min``; here one
launch of the tract-variable tile kernel (``as_tract_variables_fwd``) yields the minima and their arg-min points for all
variables and frames, and the backward sends the gradient to those two points (what ``torch.min`` / ``cdist`` do).

``AutoencoderLoss2`` (:102-251) and ``RegularizedLatentsMSELoss2`` (:254-285): their masked / weighted mean squared errors are
one pass each of ``as_masked_mse_fwd_bwd`` (loss and gradient together, deterministic sum), the frozen encoder / decoder the
fused multi-articulator MLP kernel.
"""
import torch
import torch.nn as nn

from ... import _lib
from ...phoneme_recognition.deepspeech2 import DeepSpeech2
from .models.autoencoder import Decoder, Encoder, MultiDecoder, MultiEncoder
from .transforms import InputTransform

LOWER_LIP, PHARYNX, SOFT_PALATE, TONGUE = "lower-lip", "pharynx", "soft-palate", "tongue"
UPPER_INCISOR, UPPER_LIP = "upper-incisor", "upper-lip"


class _MinPairDistance(torch.autograd.Function):
    """pairs [frames, 2 * n_tv, 2, N] (channel 2k = first point set of variable k, 2k + 1 = second) -> [frames, n_tv]."""

    @staticmethod
    def forward(ctx, pairs):
        pairs = pairs.contiguous().float()
        frames, channels, _, N = pairs.shape
        n_tv = channels // 2
        dev = pairs.device
        spec = torch.tensor([[[2 * k, 0, N], [2 * k + 1, 0, N], [-1, 0, 0]] for k in range(n_tv)], dtype=torch.int32, device=dev)
        values = torch.empty((frames, n_tv), dtype=torch.float32, device=dev)
        poc1, poc2 = torch.empty((frames, n_tv, 2), dtype=torch.float32, device=dev), torch.empty((frames, n_tv, 2), dtype=torch.float32, device=dev)
        idx = torch.empty((frames, n_tv, 2), dtype=torch.int32, device=dev)
        _lib.call("as_tract_variables_fwd", pairs, frames, channels, N, spec, n_tv, values, poc1, poc2, idx)
        ctx.save_for_backward(values, poc1, poc2, idx)
        ctx.shape = pairs.shape
        return values

    @staticmethod
    def backward(ctx, dvalues):
        values, poc1, poc2, idx = ctx.saved_tensors
        frames, channels, _, N = ctx.shape
        n_tv = channels // 2
        unit = (poc1 - poc2) / values.unsqueeze(-1)                      # d|p - q| / dp  (NaN at zero distance, like the reference)
        g = dvalues.unsqueeze(-1) * unit                                 # [frames, n_tv, 2]
        grad = torch.zeros((frames, n_tv, 2, 2, N), dtype=torch.float32, device=values.device)  # [f, k, set, xy, point]
        index = idx.long().view(frames, n_tv, 2, 1, 1).expand(frames, n_tv, 2, 2, 1)
        src = torch.stack([g, -g], dim=2).unsqueeze(-1)                  # [f, k, set, xy, 1]
        grad.scatter_(4, index, src)
        return grad.view(frames, channels, 2, N)


class CriticalLoss(nn.Module):
    TV_TO_ARTICULATOR_MAP = {"LA": [LOWER_LIP, UPPER_LIP], "TTCD": [TONGUE, UPPER_INCISOR], "TBCD": [TONGUE, UPPER_INCISOR],
                             "VEL": [SOFT_PALATE, PHARYNX]}

    def __init__(self, TVs, articulators, denormalize_fn=None):
        super().__init__()
        self.TVs = sorted(TVs)
        self.inject_reference = UPPER_INCISOR not in articulators
        if UPPER_INCISOR not in articulators:
            articulators = sorted(articulators + [UPPER_INCISOR])
        self.articulators_indices = {articulator: i for i, articulator in enumerate(articulators)}
        self.denorm_fn = denormalize_fn

    def forward(self, output_shapes, target_shapes, reference_arrays, critical_mask):
        """output_shapes / target_shapes (bs, T, n_articulators, 2, N), reference_arrays (bs, T, 1, 2, N) (the upper incisor,
        injected when it is not predicted), critical_mask (bs, n_TVs, T) -> scalar."""
        if len(self.TVs) == 0:
            return torch.tensor(0, device=target_shapes.device, dtype=torch.float)
        _lib.require_gpu(output_shapes, "output_shapes")
        if self.inject_reference:
            ref_index = self.articulators_indices[UPPER_INCISOR]
            output_shapes = torch.cat([output_shapes[:, :, :ref_index], reference_arrays.to(output_shapes.device),
                                       output_shapes[:, :, ref_index:]], dim=2)
        bs, seq_len, _, _, num_samples = target_shapes.shape
        sets = []
        for TV in self.TVs:
            for articulator in self.TV_TO_ARTICULATOR_MAP[TV]:
                array = output_shapes[..., self.articulators_indices[articulator], :, :]
                if self.denorm_fn and articulator != UPPER_INCISOR:
                    array = self.denorm_fn[articulator](array)
                sets.append(array)
        pairs = torch.stack(sets, dim=2).reshape(bs * seq_len, 2 * len(self.TVs), 2, num_samples)
        critical = _MinPairDistance.apply(pairs).view(bs, seq_len, len(self.TVs)).permute(0, 2, 1)  # (bs, n_TVs, T)
        return critical[critical_mask.to(critical.device) == 1].mean()


class _MaskedMSEFn(torch.autograd.Function):
    """scale * sum_r w_r sum_f (a - b)^2 over rows [rows][feat]; w_r = [t < lengths[b]] (row r = b * T + t) and / or
    row_weights[r].  The gradient w.r.t. a is written in the same pass; b is a target (no gradient)."""

    @staticmethod
    def forward(ctx, a, b, lengths_dev, T, row_weights, scale):
        _lib.require_gpu(a, "a")
        a, b = a.contiguous().float(), b.contiguous().float()
        if a.shape != b.shape:
            raise ValueError(f"shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        rows = a.shape[0] * a.shape[1] if lengths_dev is not None else a.shape[0]   # (B, T, ...) or (rows, ...)
        feat = a.numel() // rows
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        grad = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        partial = torch.empty(_lib.call("as_masked_mse_partials"), dtype=torch.float32, device=a.device)
        w = None if row_weights is None else row_weights.contiguous().float()
        _lib.call("as_masked_mse_fwd_bwd", a, b, rows, feat, lengths_dev, int(T), w, float(scale), loss, grad, partial)
        if grad is not None:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return grad * dloss, None, None, None, None, None


def masked_mse(a, b, lengths):
    """mean of (a - b)^2 over the valid frames (t < lengths[b]) of a, b (B, T, ...) and all their features: the
    ``loss[padding_mask].mean()`` of AutoencoderLoss2 (losses.py:215-225).  lengths: host sequence / CPU tensor."""
    lengths_cpu = torch.as_tensor(lengths, dtype=torch.int32).cpu()
    B, T = a.shape[0], a.shape[1]
    valid = int(lengths_cpu.sum())
    feat = a.numel() // (B * T)
    return _MaskedMSEFn.apply(a, b, lengths_cpu.to(a.device, non_blocking=True), T, None, 1.0 / (valid * feat))


class AutoencoderLoss2(nn.Module):
    """AutoencoderLoss adapted to several articulators (reference :102-251): beta1 * latent MSE (output_pcs against the frozen
    encoder's tanh latents of the targets) + beta2 * shape MSE (the frozen decoder on rescale_factor * output_pcs against the
    targets) + beta3 * CriticalLoss on the decoded shapes, means over the valid frames, + beta4 * the phoneme-recognition term
    when a ``recognizer`` (this engine's frozen DeepSpeech2) is given: the MSE, over the valid frames, between the scorer's
    features of the decoded shapes and of the targets (reference :226-243, including its raw ``.view`` of the (B, T, A, 2, N)
    shapes as (B, 2, A * N, T)).  The scorer runs in eval mode (no dropout); the reference leaves it in training mode."""

    def __init__(self, indices_dict, TVs, in_features, hidden_features, encoder_state_dict_filepath,
                 decoder_state_dict_filepath, device, encoder_cls=Encoder, decoder_cls=Decoder, denormalize_fn=None,
                 beta1=1.0, beta2=1.0, beta3=1.0, beta4=0.0, rescale_factor=1.0, recognizer=None, **kwargs):
        super().__init__()
        if recognizer is not None:
            if not isinstance(recognizer, DeepSpeech2):
                raise NotImplementedError("AutoencoderLoss2: the recognizer must be this engine's DeepSpeech2 (the only scorer "
                                          f"with an input gradient here), got {type(recognizer).__name__}")
            recognizer.eval()
        self.beta1, self.beta2, self.beta3, self.beta4 = self.normalize_betas([beta1, beta2, beta3, beta4])
        encoder = MultiEncoder(indices_dict, in_features, hidden_features, encoder_cls=encoder_cls)
        encoder.load_state_dict(torch.load(encoder_state_dict_filepath, map_location=device))
        self.encode = InputTransform(transform=encoder, device=device, activation=torch.tanh)
        decoder = MultiDecoder(indices_dict, in_features, hidden_features, decoder_cls=decoder_cls)
        decoder.load_state_dict(torch.load(decoder_state_dict_filepath, map_location=device))
        self.decode = InputTransform(transform=decoder, device=device)
        self.rescale_factor = rescale_factor
        articulators = sorted(indices_dict.keys())
        self.critical = CriticalLoss(TVs, articulators, denormalize_fn)
        self.recognizer = recognizer

    @staticmethod
    def normalize_betas(betas):
        return betas

    def forward(self, output_pcs, target_shapes, reference_arrays, lengths, critical_mask, voicing=None):
        """output_pcs (B, T, n_pcs), target_shapes (B, T, n_articulators, 2, N), reference_arrays (B, T, 1, 2, N),
        lengths (B,) on the host, critical_mask (B, n_TVs, T) -> scalar."""
        _lib.require_gpu(output_pcs, "output_pcs")
        bs, seq_len, num_articulators, _, num_samples = target_shapes.shape
        with torch.no_grad():
            target_pcs = self.encode.transform._forward(
                target_shapes.reshape(bs * seq_len, num_articulators, 2 * num_samples), tanh=True)
        target_pcs = target_pcs.reshape(bs, seq_len, -1)
        output_shapes = self.decode.transform(output_pcs, scale=self.rescale_factor)
        output_shapes = output_shapes.reshape(bs, seq_len, num_articulators, 2, num_samples)
        latent_loss = masked_mse(output_pcs, target_pcs, lengths)
        reconstruction_loss = masked_mse(output_shapes, target_shapes, lengths)
        critical_loss = self.critical(output_shapes, target_shapes, reference_arrays, critical_mask)
        if self.recognizer is None:
            return self.beta1 * latent_loss + self.beta2 * reconstruction_loss + self.beta3 * critical_loss
        recognition_loss = self._recognition(output_shapes, target_shapes, lengths, voicing)
        return self.beta1 * latent_loss + self.beta2 * reconstruction_loss + self.beta3 * critical_loss + self.beta4 * recognition_loss

    def _recognition(self, output_shapes, target_shapes, lengths, voicing):
        bs, seq_len, n_art, chann, n_samples = target_shapes.shape
        self.recognizer.eval()   # (a .train() of this module reaches the registered recognizer; the scorer is eval-only)
        with torch.no_grad():
            _, target_features = self.recognizer(target_shapes.contiguous().view(bs, chann, n_art * n_samples, seq_len), voicing,
                                                 return_features=True)
        _, output_features = self.recognizer(output_shapes.contiguous().view(bs, chann, n_art * n_samples, seq_len), voicing,
                                             return_features=True)
        return masked_mse(output_features, target_features, lengths)


class RegularizedLatentsMSELoss2(nn.Module):
    """mean over (bs, A, F) of sample_weights[bs] * (outputs - target)^2 + alpha * the off-diagonal squared covariance of
    each articulator's latents (reference :254-285).  The reference builds the covariance term through torch.tensor([...]),
    which detaches it: it counts in the value, never in the gradient.  Kept so (on the device, no host sync)."""

    def __init__(self, alpha, indices_dict):
        super().__init__()
        self.alpha = alpha
        self.indices_dict = indices_dict

    def forward(self, outputs, latents, target, sample_weights=None):
        _lib.require_gpu(outputs, "outputs")
        rows = outputs.shape[0]
        scale = 1.0 / outputs.numel()
        mse = _MaskedMSEFn.apply(outputs.reshape(rows, -1), target.reshape(rows, -1), None, 0, sample_weights, scale)
        with torch.no_grad():
            terms = []
            for _, indices in self.indices_dict.items():
                if len(indices) > 1:
                    cov = torch.cov(latents.T[indices])
                    terms.append(cov.square().sum() - cov.diag().square().sum())
            cov_loss = torch.stack(terms).sum() if terms else torch.zeros((), device=outputs.device)
        return mse + self.alpha * cov_loss
