"""Metric of the principal-components method (reference principal_components/metrics.py:11-61): the mean point-to-closest-
point distance in mm between the frozen decoder's shapes of the predicted components and the targets, over valid frames."""
import torch
import torch.nn as nn

from ..metrics import MeanP2CPDistance
from .models.autoencoder import Decoder, MultiDecoder
from .transforms import InputTransform


class DecoderMeanP2CPDistance2(nn.Module):
    def __init__(self, dataset_config, decoder_state_dict_filepath, indices_dict, autoencoder_kwargs, denorm_fns, device,
                 decoder_cls=Decoder):
        super().__init__()
        self.articulators = sorted(indices_dict.keys())
        self.dataset_config = dataset_config
        self.to_mm = self.dataset_config.RES * self.dataset_config.PIXEL_SPACING
        decoder = MultiDecoder(indices_dict, decoder_cls=decoder_cls, **autoencoder_kwargs)
        decoder.load_state_dict(torch.load(decoder_state_dict_filepath, map_location=device))
        self.decode = InputTransform(transform=decoder, device=device)
        self.mean_p2cp = MeanP2CPDistance(reduction="none")
        self.denorm_fns = denorm_fns

    def forward(self, outputs, targets, lengths):
        """outputs (B, T, n_components), targets (B, T, A, 2, N), lengths (B,) -> scalar mm.  Like the reference, the
        caller's ``targets`` are denormalised IN PLACE (a visible side effect the trainer's loop does not mind)."""
        bs, seq_len, num_articulators, _, num_samples = targets.shape
        with torch.no_grad():
            outputs_shapes = self.decode(outputs).reshape(bs, seq_len, num_articulators, 2, num_samples)
            for i, articulator in enumerate(self.articulators):
                outputs_shapes[..., i, :, :] = self.denorm_fns[articulator](outputs_shapes[..., i, :, :])
                targets[..., i, :, :] = self.denorm_fns[articulator](targets[..., i, :, :])
            p2cp = self.mean_p2cp(outputs_shapes.transpose(-1, -2), targets.transpose(-1, -2))   # (B, T, A)
            p2cp_mm = p2cp * self.to_mm
            p2cp_mm = torch.cat([p2cp_mm[i, :l, :] for i, l in enumerate(lengths)])
            return p2cp_mm.mean()
