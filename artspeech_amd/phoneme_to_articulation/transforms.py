"""Normalize of the phoneme_to_articulation package (reference phoneme_to_articulation/transforms.py:1-35)."""


class Normalize:
    def __init__(self, mean, std):
        """mean, std: tensors of shape (N, M)."""
        self.mean = mean
        self.std = std

    def __call__(self, x):
        """(x - mean) / std, x (*, N, M)."""
        mean = self.mean.clone().to(x.device)
        std = self.std.clone().to(x.device)
        return (x - mean) / std

    def inverse(self, x_norm):
        """x_norm * std + mean, x_norm (*, N, M)."""
        mean = self.mean.clone().to(x_norm.device)
        std = self.std.clone().to(x_norm.device)
        return (x_norm * std) + mean
