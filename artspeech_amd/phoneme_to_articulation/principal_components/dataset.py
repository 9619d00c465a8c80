"""Data of the principal-components method (reference principal_components/dataset.py): the collate function of the
phoneme -> components trainer (:224-263), seeded synthetic stand-ins for the two datasets with the reference's item layouts and
``.normalize`` dicts, and the real-data classes, which need the reference's MRI data stack (``database_collector``,
``vt_shape_gen`` / ``vt_tools``) and raise without it."""
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import Dataset

from ..transforms import Normalize
from ...settings import DATASET_CONFIG, UNKNOWN

# per-phoneme sample weights of the autoencoder's frames (reference :13-25)
phoneme_weights = {"l": 3, "d": 3, "t": 3, "n": 3, "k": 3, "g": 3, "#": 0.1, "-": 0.1, "ih": 0.1, "yh": 0.1, "uh": 0.1}

_NEEDS_DATA_STACK = ("needs the reference's real-data stack (database_collector.DATABASE_COLLECTORS and "
                     "phoneme_to_articulation.InputLoaderMixin with vt_shape_gen / vt_tools), which this engine does not "
                     "vendor; use datadir: synthetic")


def _normalizers(articulators, n_samples, g):
    """{articulator: Normalize(mean (2, N), std (2, N))}: seeded statistics of the size of the real ones (normalised contours)."""
    return {a: Normalize(torch.rand(2, n_samples, generator=g) * 0.5, 0.1 + 0.2 * torch.rand(2, n_samples, generator=g))
            for a in articulators}


class PrincipalComponentsAutoencoderDataset2(Dataset):
    def __init__(self, database_name, datadir, sequences, articulators, clip_tails=True, normalize_data=True):
        raise NotImplementedError(f"PrincipalComponentsAutoencoderDataset2 {_NEEDS_DATA_STACK}")


class PrincipalComponentsPhonemeToArticulationDataset2(Dataset):
    def __init__(self, database_name, datadir, sequences, vocabulary, articulators, TV_to_phoneme_map, num_samples=50,
                 clip_tails=True, voiced_tokens=None):
        raise NotImplementedError(f"PrincipalComponentsPhonemeToArticulationDataset2 {_NEEDS_DATA_STACK}")


def low_rank_frames(num_frames, channels, features, rank, generator):
    """(num_frames, channels, features) float32 frames 0.5 + z diag(0.25 0.7^j) Q^T + 0.002 noise, j < min(rank, features), Q
    orthonormal per channel: a geometric spectrum over a noise floor, so that the leading principal directions are well
    separated.  Drawn and multiplied in float64 and rounded once, so that machines whose float32 matrix products differ in the
    last bit still build the same frames."""
    rank = min(rank, features)
    z = torch.randn(num_frames, channels, rank, generator=generator, dtype=torch.float64)
    q, _ = torch.linalg.qr(torch.randn(channels, features, rank, generator=generator, dtype=torch.float64))
    scale = 0.25 * 0.7 ** torch.arange(rank, dtype=torch.float64)
    noise = torch.randn(num_frames, channels, features, generator=generator, dtype=torch.float64)
    return (0.5 + torch.einsum("nar,afr->naf", z * scale, q) + 0.002 * noise).float()


class SyntheticPrincipalComponentsAutoencoderDataset(Dataset):
    """Frames of the autoencoder's dataset (reference :28-107): item = (frame_name, articulators (A, 2 N) float,
    weight (phoneme_weights of the frame's phoneme), phoneme); contours U(0, 1) like normalised real data, whose principal
    directions are all equivalent, or, with ``rank=r``, low-rank frames with a decaying spectrum (``low_rank_frames``), which a PCA
    can be fitted to."""

    def __init__(self, num_frames, articulators, n_samples=50, seed=0, database_name="artspeech2", phonemes=None, rank=None):
        self.articulators = sorted(articulators)
        self.num_samples = n_samples
        self.dataset_config = DATASET_CONFIG[database_name]
        g = torch.Generator().manual_seed(seed)
        self.normalize = _normalizers(self.articulators, n_samples, g)
        phonemes = phonemes or ["a", "l", "t", "#", "ih", "s", "k", "m"]
        self._phonemes = [phonemes[i] for i in torch.randint(0, len(phonemes), (num_frames,), generator=g).tolist()]
        if rank is None:
            self._frames = torch.rand(num_frames, len(self.articulators), 2 * n_samples, generator=g)
        else:
            self._frames = low_rank_frames(num_frames, len(self.articulators), 2 * n_samples, rank, g)

    def __len__(self):
        return len(self._phonemes)

    def __getitem__(self, index):
        phoneme = self._phonemes[index]
        weight = torch.tensor(phoneme_weights.get(phoneme, 1), dtype=torch.float)
        return f"synthetic_S1_{index:05d}", self._frames[index].clone(), weight, phoneme


class SyntheticPrincipalComponentsPhonemeToArticulationDataset(Dataset):
    """Sentences of the phoneme -> components dataset (reference :110-221): item = (sentence_name, tokens (T,) long,
    targets (T, A, 2, N), phonemes, critical_mask (n_TVs, T) int, reference_arrays (T, 1, 2, N), frame_ids, voicing (T,));
    tokens uniform in [2, V), contours U(0, 1), lengths uniform in [min_len, max_len]."""

    def __init__(self, num_sentences, vocabulary, articulators, TV_to_phoneme_map=None, n_samples=50, min_len=20, max_len=200,
                 seed=0, database_name="artspeech2", voiced_tokens=None):
        self.vocabulary = vocabulary
        self.articulators = sorted(articulators)
        self.num_samples = n_samples
        self.dataset_config = DATASET_CONFIG[database_name]
        self.TV_to_phoneme_map = TV_to_phoneme_map or {}
        self.voiced_tokens = voiced_tokens or []
        self._tokens_by_id = {i: t for t, i in vocabulary.items()}
        g = torch.Generator().manual_seed(seed)
        self.normalize = _normalizers(self.articulators, n_samples, g)
        self._lengths = torch.randint(min_len, max_len + 1, (num_sentences,), generator=g).tolist()
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return len(self._lengths)

    def __getitem__(self, index):
        length = self._lengths[index]
        g = torch.Generator().manual_seed(self._seeds[index])
        low = min(2, len(self.vocabulary) - 1)
        numerized = torch.randint(low, len(self.vocabulary), (length,), generator=g, dtype=torch.long)
        targets = torch.rand(length, len(self.articulators), 2, self.num_samples, generator=g)
        reference_arrays = torch.rand(length, 1, 2, self.num_samples, generator=g)
        tokens = [self._tokens_by_id.get(int(i), UNKNOWN) for i in numerized]
        if len(self.TV_to_phoneme_map) > 0:
            critical_mask = torch.stack([torch.tensor([int(p in self.TV_to_phoneme_map[TV]) for p in tokens], dtype=torch.int)
                                         for TV in sorted(self.TV_to_phoneme_map.keys())])
        else:
            critical_mask = torch.zeros(size=(0, length))
        voicing = torch.tensor([p in self.voiced_tokens for p in tokens], dtype=torch.float)
        frame_ids = [f"{i:04d}" for i in range(length)]
        return f"synthetic_{index:05d}", numerized, targets, tokens, critical_mask, reference_arrays, frame_ids, voicing


def pad_sequence_collate_fn(batch):
    """8-field items -> (sentence_ids, tokens (B, T), targets (B, T, A, 2, N), lengths (B,) int32 descending, phonemes,
    critical_masks (B, n_TVs, T), reference_arrays (B, T, 1, 2, N), frame_ids, voicing (B, T) padded with -1), every
    per-utterance field in the order of descending length (a stable sort, like the reference's torch.sort on CPU)."""
    lengths = torch.tensor([len(item[1]) for item in batch], dtype=torch.int)
    lengths_sorted, order = lengths.sort(descending=True)
    order_list = order.tolist()

    def padded(field, **kw):
        return pad_sequence([item[field] for item in batch], batch_first=True, **kw)[order]

    critical = pad_sequence([item[4].T for item in batch], batch_first=True)[order].permute(0, 2, 1)
    voicing = pad_sequence([batch[i][7] for i in order_list], batch_first=True, padding_value=-1)
    return ([batch[i][0] for i in order_list], padded(1), padded(2), lengths_sorted, [batch[i][3] for i in order_list],
            critical, padded(5), [batch[i][6] for i in order_list], voicing)
