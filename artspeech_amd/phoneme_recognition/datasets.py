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


class SyntheticAcousticRecognitionDataset(Dataset):
    """num_sentences seeded utterances of synthetic speech over vocabulary, for ``feature: melspec``.  Every token has a prototype
    of three sinusoids (frequencies between 200 Hz and 0.45 sample_rate and amplitudes seeded by prototype_seed, the same for every
    split); a sentence of min_seconds to max_seconds is a random token sequence in which each token is held for 60 to 200 ms,
    and its waveform is the tokens' prototypes over their intervals plus white noise of scale ``noise``.  Items carry the
    waveform (``waveform`` (n,) float32, ``waveform_length``, ``audio_duration`` = n / sample_rate) and the reference's label keys:
    ``phonemes_with_time`` [(token name, start, end) in seconds] with ``phoneme_tokens`` (their ids), ``articulatory_target``
    (the token of every frame at ``framerate``) with ``voicing``, and ``ctc_target = unique_consecutive`` of the token
    sequence.  No spectrogram: the features of a batch are computed on the device by ``acoustic_collate_fn``; with the
    attribute ``melspectrogram`` set, items carry that transform (key ``melspectrogram``) and ``collate_fn(batch, [Feature.MELSPEC])``
    does the same."""

    def __init__(self, num_sentences, vocabulary, sample_rate=16000, min_seconds=0.5, max_seconds=2.0, framerate=50, noise=0.01,
                 seed=0, voiced_tokens=None, num_special=2, prototype_seed=0):
        self.vocabulary = vocabulary
        self.num_sentences, self.sample_rate, self.framerate, self.noise = num_sentences, sample_rate, framerate, noise
        self.min_samples, self.max_samples = int(round(min_seconds * sample_rate)), int(round(max_seconds * sample_rate))
        self.voiced = set(voiced_tokens or [])
        self.names = {i: tok for tok, i in vocabulary.items()}
        self.token_ids = sorted(i for i in vocabulary.values() if i >= num_special)
        V = max(vocabulary.values()) + 1
        gp = torch.Generator().manual_seed(prototype_seed)   # shared by every split
        self.melspectrogram = None   # features.MelSpectrogram that collate_fn launches on this data set's batches (set by the owner)
        self.frequencies = 200.0 + (0.45 * sample_rate - 200.0) * torch.rand(V, 3, generator=gp, dtype=torch.float64)
        self.amplitudes = (0.1 + 0.3 * torch.rand(V, 3, generator=gp, dtype=torch.float64))
        g = torch.Generator().manual_seed(seed)
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return self.num_sentences

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self._seeds[index])
        sr = self.sample_rate
        n = int(torch.randint(self.min_samples, self.max_samples + 1, (1,), generator=g))
        ids = torch.tensor(self.token_ids)
        lo, hi = max(1, int(0.06 * sr)), max(2, int(0.2 * sr))
        tokens, bounds, at = [], [0], 0
        while at < n:
            tokens.append(int(ids[torch.randint(0, len(ids), (1,), generator=g)]))
            at = min(n, at + int(torch.randint(lo, hi + 1, (1,), generator=g)))
            bounds.append(at)
        time = torch.arange(n, dtype=torch.float64) / sr
        token_of_sample = torch.repeat_interleave(torch.tensor(tokens), torch.tensor(bounds).diff())
        phase = 2.0 * torch.pi * self.frequencies[token_of_sample] * time[:, None]                       # (n, 3)
        signal = (self.amplitudes[token_of_sample] * torch.sin(phase)).sum(dim=1)
        waveform = (signal + self.noise * torch.randn(n, generator=g, dtype=torch.float64)).float()
        duration = n / sr
        phonemes_with_time = [(self.names[tok], bounds[i] / sr, bounds[i + 1] / sr) for i, tok in enumerate(tokens)]
        T = max(1, int(duration * self.framerate))
        centres = ((torch.arange(T, dtype=torch.float64) + 0.5) / self.framerate * sr).long().clamp(max=n - 1)
        sentence = token_of_sample[centres]
        voicing = torch.tensor([self.names[int(t)] in self.voiced for t in sentence], dtype=torch.float)
        ctc_target = torch.unique_consecutive(torch.tensor(tokens, dtype=torch.long))
        item = {} if self.melspectrogram is None else {"melspectrogram": self.melspectrogram}
        return {
            **item,
            "waveform": waveform,
            "waveform_length": n,
            "audio_duration": duration,
            "phonemes_with_time": phonemes_with_time,
            "phoneme_tokens": tokens,
            "articulatory_target": sentence,
            "articulatory_target_length": T,
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


def acoustic_target(phonemes_with_time, tokens, melspec_length, audio_duration):
    """Reference :213-220: zeros of melspec_length; per (phoneme, start, end) the frames
    [int(start L / duration), int(end L / duration)) take the phoneme's token (tokens[i] for the i-th interval)."""
    target = torch.zeros(melspec_length, dtype=torch.long)
    for (_, start_time, end_time), token in zip(phonemes_with_time, tokens):
        start_spec = int((start_time * melspec_length) / audio_duration)
        end_spec = int((end_time * melspec_length) / audio_duration)
        target[start_spec:end_spec] = token
    return target


def acoustic_collate_fn(batch, melspectrogram, device=None, vocabulary=None, unknown_token="<unk>"):
    """The reference's collate_fn(batch, [Feature.MELSPEC]) for items that carry waveforms: the waveforms are padded and uploaded
    once, ``melspectrogram.log_mel_batch`` (features.MelSpectrogram) computes the (B, 2, n_mels, T) log-mel batch with its -1
    padding on the device, and the acoustic targets follow from the frame counts.  Same keys, dtypes and padding as collate_fn;
    ``melspec`` is on the device.  With ``vocabulary`` the token of an interval is ``vocabulary.get(phoneme, unknown)`` as in the
    reference (:215), for any item with ``phonemes_with_time``; without it the item's own ``phoneme_tokens`` are taken.  It
    launches a kernel, so it runs in the main process: the DataLoader gets num_workers=0 (a worker process raises)."""
    if torch.utils.data.get_worker_info() is not None:
        raise ValueError("acoustic_collate_fn computes its features on the device while collating: num_workers must be 0")
    from . import Feature, Target
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("artspeech_amd: acoustic_collate_fn computes the mel spectrogram on an MI355X device; there is no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    waves = pad_sequence([item["waveform"] for item in batch], batch_first=True, padding_value=0.0)
    lengths = torch.tensor([item["waveform_length"] for item in batch], dtype=torch.long)
    feats, feat_lengths = melspectrogram.log_mel_batch(waves.to(device), lengths, channels=2)
    out = {Feature.MELSPEC.value: feats, f"{Feature.MELSPEC.value}_length": feat_lengths}
    def tokens(item):
        if vocabulary is None:
            return item["phoneme_tokens"]
        return [vocabulary.get(phoneme, vocabulary[unknown_token]) for phoneme, _, _ in item["phonemes_with_time"]]

    targets = [acoustic_target(item["phonemes_with_time"], tokens(item), int(L), item["audio_duration"])
               for item, L in zip(batch, feat_lengths)]
    out[Target.ACOUSTIC.value] = pad_sequence(targets, batch_first=True, padding_value=-1)
    out[f"{Target.ACOUSTIC.value}_length"] = feat_lengths.clone()
    for tgt in (Target.ARTICULATORY, Target.CTC):
        out[tgt.value] = pad_sequence([item[tgt.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{tgt.value}_length"] = torch.tensor([item[f"{tgt.value}_length"] for item in batch], dtype=torch.long)
    out["voicing"] = pad_sequence([item["voicing"] for item in batch], batch_first=True, padding_value=-1)
    return out


def collate_fn(batch, features_names):
    """Reference :253-302: features (C, D, T) padded with -1 along time into (B, C, D, T); articulatory targets, voicing and CTC
    targets padded with -1; lengths as int64 tensors."""
    from . import Feature, Target
    if Feature.MELSPEC in features_names and "waveform" in batch[0]:   # waveform items: the feature is computed here, on the device
        if list(features_names) != [Feature.MELSPEC] or batch[0].get("melspectrogram") is None:
            raise ValueError("collate_fn: waveform items collate as [Feature.MELSPEC] alone and carry their MelSpectrogram "
                             "(SyntheticAcousticRecognitionDataset.melspectrogram); or call acoustic_collate_fn")
        return acoustic_collate_fn(batch, batch[0]["melspectrogram"])
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
