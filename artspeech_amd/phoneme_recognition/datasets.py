"""Data of the phoneme recogniser (reference ``phoneme_recognition/datasets.py``, ``synthetic_shapes.py``): the collate function
(:253-302), a seeded synthetic data set with the reference's item layout (synthetic_shapes.py:146-158), and the real-data class,
which needs the reference's MRI data stack and raises without it."""
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import Dataset

_NEEDS_DATA_STACK = ("needs the reference's real-data stack (database_collector.DATABASE_COLLECTORS, vt_shape_gen / vt_tools and "
                     "the air-column / mel-spectrogram feature extraction), which this engine does not vendor; use datadir: synthetic")


class PhonemeRecognitionDataset(Dataset):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"PhonemeRecognitionDataset {_NEEDS_DATA_STACK}")


class SyntheticPhonemeRecognitionDataset(Dataset):
    """num_sentences seeded utterances over vocabulary ({token: index}; the first ``num_special`` indices -- blank and unknown --
    never occur).  Every token has a prototype frame (seeded by prototype_seed, the same for every split) of the vocal-tract feature (2, n_articulators * n_samples); a
    sentence is a random token sequence in which each token holds for 2 to 6 frames (between min_len and max_len frames in all),
    its frames the token's prototype plus Gaussian noise of scale ``noise``.  Items carry the reference's keys: ``vocal_tract``
    (2, A*N, T) and ``air_column`` (2, 2N, T) with their lengths, ``articulatory_target`` (the per-frame tokens), ``voicing``
    (1 where the frame's token is in voiced_tokens) and ``ctc_target = unique_consecutive(articulatory_target)``."""

    def __init__(self, num_sentences, vocabulary, n_articulators=10, n_samples=50, min_len=20, max_len=120, noise=0.3, seed=0,
                 voiced_tokens=None, num_special=2, prototype_seed=0):
        self.vocabulary = vocabulary
        self.num_sentences, self.min_len, self.max_len, self.noise = num_sentences, min_len, max_len, noise
        self.voiced = set(voiced_tokens or [])
        self.names = {i: tok for tok, i in vocabulary.items()}
        self.token_ids = sorted(i for i in vocabulary.values() if i >= num_special)
        V = max(vocabulary.values()) + 1
        gp = torch.Generator().manual_seed(prototype_seed)   # shared by every split: the splits differ in their sentences only
        self.prototypes = torch.randn(V, 2, n_articulators * n_samples, generator=gp)
        self.air_prototypes = torch.randn(V, 2, 2 * n_samples, generator=gp)
        g = torch.Generator().manual_seed(seed)
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return self.num_sentences

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self._seeds[index])
        T = int(torch.randint(self.min_len, self.max_len + 1, (1,), generator=g))
        ids = torch.tensor(self.token_ids)
        frames = []
        while len(frames) < T:
            tok = int(ids[torch.randint(0, len(ids), (1,), generator=g)])
            frames += [tok] * int(torch.randint(2, 7, (1,), generator=g))
        sentence = torch.tensor(frames[:T], dtype=torch.long)
        vt = self.prototypes[sentence] + self.noise * torch.randn(T, *self.prototypes.shape[1:], generator=g)   # (T, 2, A*N)
        air = self.air_prototypes[sentence] + self.noise * torch.randn(T, *self.air_prototypes.shape[1:], generator=g)
        voicing = torch.tensor([self.names[int(t)] in self.voiced for t in sentence], dtype=torch.float)
        ctc_target = torch.unique_consecutive(sentence)
        return {
            "air_column": air.permute(1, 2, 0).contiguous(),
            "air_column_length": T,
            "vocal_tract": vt.permute(1, 2, 0).contiguous(),
            "vocal_tract_length": T,
            "articulatory_target": sentence,
            "articulatory_target_length": T,
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


def collate_fn(batch, features_names):
    """Reference :253-302: features (C, D, T) padded with -1 along time into (B, C, D, T); articulatory targets, voicing and CTC
    targets padded with -1; lengths as int64 tensors."""
    from . import Feature, Target
    out = {}
    for feature_name in features_names:
        feats = pad_sequence([item[feature_name.value].permute(2, 0, 1) for item in batch], batch_first=True, padding_value=-1)
        out[feature_name.value] = feats.permute(0, 2, 3, 1)
        out[f"{feature_name.value}_length"] = torch.tensor([item[f"{feature_name.value}_length"] for item in batch], dtype=torch.long)
    if Feature.MELSPEC in features_names:
        out[Target.ACOUSTIC.value] = pad_sequence([item[Target.ACOUSTIC.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{Target.ACOUSTIC.value}_length"] = torch.tensor([item[f"{Target.ACOUSTIC.value}_length"] for item in batch],
                                                              dtype=torch.long)
    for tgt in (Target.ARTICULATORY, Target.CTC):
        out[tgt.value] = pad_sequence([item[tgt.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{tgt.value}_length"] = torch.tensor([item[f"{tgt.value}_length"] for item in batch], dtype=torch.long)
    out["voicing"] = pad_sequence([item["voicing"] for item in batch], batch_first=True, padding_value=-1)
    return out
